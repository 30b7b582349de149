// rsx_seg_layout.hpp: where the parts of a segmented route's device-side state lie -- the control block c.seg (SegLayout) and the
// level-1 slots that lie in two arrays (SlotParts).  Part of librsx.so's host side, included by rsx.hip (one translation unit).
// Nothing of HIP and nothing of Ctx is used here: tests/cpp/seg_layout_check.cpp includes this file alone and checks both on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

// ---- the control block of the routes with MSB passes into slots and leaves (Ctx::seg) -------------------------------------------
// [SegCtl, 256 B][per-bucket digit counts][a status region per segmented pass][leaf segments][tiles][btile][redo]
// (the sizes of SegCtl's room, LeafSeg and SegTile: rsx_route_levels.hpp asserts them against the structs of rsx_hybrid.hpp)
constexpr size_t SEG_CTL_BYTES = 256;        // SegCtl, padded: what lies behind it is zeroed apart from it
constexpr size_t SEG_LEAFSEG_BYTES = 16;     // sizeof(LeafSeg)
constexpr size_t SEG_TILE_BYTES = 16;        // sizeof(SegTile)
constexpr size_t SEG_LEAVES = 65536;         // entries of the leaf table and of the redo list: one per (digit, digit) bucket
constexpr size_t SEG_BTILE_WORDS = 260;      // bucket k's tiles are [btile[k], btile[k + 1]): 257 words, padded to 16 bytes

// rows of status words of one segmented pass: the tiles of n keys + `extra_rows` partial ones (seg_extra_rows)
inline uint64_t seg_rows(size_t n, size_t tile, uint64_t extra_rows) { return (n + tile - 1) / tile + extra_rows; }

struct SegLayout {
	uint64_t rows = 0;       // seg_rows: the grid of a segmented pass
	size_t st_bytes = 0;     // one pass's status region: [ticket u32, pad to 256 B][rows x 256 status words u32]
	size_t hist_off = 0;     // [bucket][key bytes - 1][256] u32 digit counts inside the level-1 buckets
	size_t status_off = 0;   // key bytes - 1 status regions
	size_t segtab_off = 0;   // [SEG_LEAVES] LeafSeg
	size_t tiles_off = 0;    // [tile_rows] SegTile
	size_t btile_off = 0;    // [SEG_BTILE_WORDS] u32
	size_t redo_off = 0;     // [SEG_LEAVES] u32: the leaves rsx_leaf16_kernel leaves to rsx_leaf_sort_kernel
	size_t total = 0;        // bytes of the block
	// the status region of segmented pass j (its ticket word), and the status words -- or cursors -- behind the ticket
	size_t status(size_t j) const { return status_off + j * st_bytes; }
	size_t cursors(size_t j) const { return status(j) + 256; }
};

// the layout for n keys of `key_bytes` bytes: pass tiles of `tile` keys, `extra_rows` status rows beyond n / tile, a tile table
// of `tile_rows` entries
inline SegLayout seg_layout_for(size_t key_bytes, size_t n, size_t tile, uint64_t extra_rows, uint64_t tile_rows)
{
	SegLayout l;
	l.rows = seg_rows(n, tile, extra_rows);
	l.st_bytes = 256 + (size_t)l.rows * 256 * 4;
	l.hist_off = SEG_CTL_BYTES;
	l.status_off = l.hist_off + (size_t)256 * (key_bytes - 1) * 256 * sizeof(uint32_t);
	l.segtab_off = l.status_off + (key_bytes - 1) * l.st_bytes;
	l.tiles_off = l.segtab_off + SEG_LEAVES * SEG_LEAFSEG_BYTES;
	l.btile_off = l.tiles_off + (size_t)tile_rows * SEG_TILE_BYTES;
	l.redo_off = l.btile_off + SEG_BTILE_WORDS * sizeof(uint32_t);
	l.total = l.redo_off + SEG_LEAVES * sizeof(uint32_t);
	return l;
}

// ---- level-1 slots in two parts ---------------------------------------------------------------------------------------------------
// The 256 level-1 slots of a sort without a histogram, `cap1` elements each: the first `lo` in the caller's spare buffer, the
// others in the library's scratch array (blind_enqueue, pairs_blind_enqueue).  The level-1 pass is given ONE base -- the lower of
// the two arrays -- and the 32-bit element offsets from it of slot 0 of either part: slot d < lo begins at base + (off_lo + d x cap1)
// elements, slot d >= lo at base + (off_hi + d x cap1), where off_hi names a VIRTUAL slot 0, lo slots before the scratch array (`hi`:
// its address, what the level-2 pass reads the scratch part through).  Every element a pass may touch -- the dump area of a tile
// behind the last slot included -- must lie within 2^32 elements of the base: fits32().  lo == 0: everything in scratch.
struct SlotParts {
	uintptr_t base = 0, hi = 0;
	uint32_t off_lo = 0, off_hi = 0;
	uint64_t span = 0;   // elements from the base to the end of what the farther part may touch
	SlotParts(const void *spare, const void *scratch, uint32_t lo, uint32_t cap1, size_t elem_bytes, size_t tile)
	{
		const uintptr_t lo_a = lo ? (uintptr_t)spare : (uintptr_t)scratch;
		const uintptr_t hi_a = (uintptr_t)scratch - (size_t)lo * cap1 * elem_bytes;
		base = lo_a < hi_a ? lo_a : hi_a;
		hi = hi_a;
		span = (uint64_t)((lo_a < hi_a ? hi_a - lo_a : lo_a - hi_a) / elem_bytes) + (uint64_t)257 * cap1 + tile;
		off_lo = (uint32_t)((lo_a - base) / elem_bytes);
		off_hi = (uint32_t)((hi_a - base) / elem_bytes);
	}
	bool fits32() const { return span < ((uint64_t)1 << 32); }
};

}   // namespace
