// rsx_partition_shape.hpp: the arithmetic of rsx_sort_partition*'s scatter route (rsx_partition.hpp) -- the shares of
// the grid, the bin-major scan over the workgroups' rows of counts, what the caller's offsets read out of the scanned bin
// totals, and the choice between the two ranking forms.  The search itself is rsx_locate_shape.hpp's, unchanged.  Nothing of HIP
// and nothing of Ctx is used here: every function is __host__ __device__ under hipcc and plain C++ otherwise;
// tests/cpp/partition_shape_check.cpp includes this file alone and checks it on the CPU against serial loops.
#pragma once

#include "rsx_locate_shape.hpp"

namespace rsx {

// The count and place kernels: a tile is PARTITION_TILE keys (eight per thread), a workgroup owns a contiguous share of the keys in
// memory order -- at least PARTITION_SHARE_TILES whole tiles, and there are at most PARTITION_MAX_WGS shares (one workgroup per CU).
// At most PARTITION_MAX_EDGES distinct edges, so at most PARTITION_MAX_BINS parts: a bin number is one byte.
enum : u32 { PARTITION_MAX_EDGES = 255, PARTITION_MAX_BINS = 256, PARTITION_THREADS = 1024, PARTITION_KPT = 8, PARTITION_TILE = 8192,
             PARTITION_SHARE_TILES = 2, PARTITION_MAX_WGS = 256, PARTITION_WAVES = 16, PARTITION_BALLOT_PARTS_DEFAULT = 7 };

// ---- the shares ---------------------------------------------------------------------------------------------------------------
// `head` keys lie in front of the first 16-byte boundary of the keys.  The keys behind it are cut into whole tiles; share w owns
// the tiles [w * share_tiles, (w + 1) * share_tiles).  The head belongs to the FIRST share and what lies behind the last whole tile
// to the LAST one (unlike locate's grid, where workgroup 0 takes both: here a share must be one contiguous range in memory order,
// or the placement would not be stable).
struct PartitionGrid {
	u64 head, tiles, share_tiles;
	u32 wgs;
};
RSX_LOCATE_HD u64 partition_head(u64 addr, u32 key_bytes, u64 n)
{
	const u64 head = ((16u - (u32)(addr & 15u)) & 15u) / key_bytes;
	return head < n ? head : n;
}
RSX_LOCATE_HD PartitionGrid partition_grid(u64 n, u64 head)
{
	PartitionGrid g;
	g.head = head < n ? head : n;
	g.tiles = (n - g.head) / PARTITION_TILE;
	const u64 even = (g.tiles + PARTITION_MAX_WGS - 1u) / PARTITION_MAX_WGS;
	g.share_tiles = even > PARTITION_SHARE_TILES ? even : (u64)PARTITION_SHARE_TILES;
	const u64 wgs = (g.tiles + g.share_tiles - 1u) / g.share_tiles;
	g.wgs = (u32)(wgs ? wgs : 1u);
	return g;
}
// share w of the grid over n keys is [partition_share_lo, partition_share_hi)
RSX_LOCATE_HD u64 partition_share_lo(const PartitionGrid &g, u32 w) { return w == 0 ? 0 : g.head + (u64)w * g.share_tiles * PARTITION_TILE; }
RSX_LOCATE_HD u64 partition_share_hi(const PartitionGrid &g, u32 w, u64 n)
{
	return w + 1u >= g.wgs ? n : g.head + (u64)(w + 1u) * g.share_tiles * PARTITION_TILE;
}

// ---- the scan -----------------------------------------------------------------------------------------------------------------
// rows[w][b], w < wgs, b < bins: the keys of share w that fall in bin b.  The output lists the bins in ascending order and inside
// a bin the shares in ascending order: the start of (b, w) is the keys of the bins below b plus those of bin b in the shares below w.
RSX_LOCATE_HD u64 partition_bin_total(const u64 *rows, u32 wgs, u32 bins, u32 b)
{
	u64 sum = 0;
	for (u32 w = 0; w < wgs; ++w)
		sum += rows[(u64)w * bins + b];
	return sum;
}
// starts[w][b] = base + the keys of bin b in the shares below w (`base`: the keys of the bins below b)
RSX_LOCATE_HD void partition_bin_starts(const u64 *rows, u32 wgs, u32 bins, u32 b, u64 base, u64 *starts)
{
	u64 run = base;
	for (u32 w = 0; w < wgs; ++w) {
		starts[(u64)w * bins + b] = run;
		run += rows[(u64)w * bins + b];
	}
}

// ---- the caller's offsets -----------------------------------------------------------------------------------------------------
// The kernels split by the number e of DISTINCT edges at or below (BELOW: below) a key, 0 .. D; the caller's bin of such a key is
// cum[e], the number of the m edges there (cum[0] = 0 < cum[1] < .. < cum[D] = m: rsx_locate_shape.hpp).  offsets[j], j in
// 0 .. m + 1, is the number of keys whose bin is below j: the keys of the distinct bins e with cum[e] < j -- the first
// partition_offset_entry(cum, D, j) of them (D + 1: all of them).  Repeated edges skip values of j: those parts are empty.
RSX_LOCATE_HD u32 partition_offset_entry(const u64 *cum, u32 D, u64 j)
{
	u32 lo = 0, hi = D + 1u;   // the first e in 0 .. D with cum[e] >= j
	while (lo < hi) {
		const u32 mid = (lo + hi) / 2u;
		if (cum[mid] < j)
			lo = mid + 1u;
		else
			hi = mid;
	}
	return lo;
}

// ---- the ranking form ---------------------------------------------------------------------------------------------------------
// 1: one ballot per bin (few parts: every lane of a wave would meet in a handful of LDS cells); 2: per-wave cells in LDS, the
// lanes of one bin found by one ballot per bit of the bin number.  `seam`: RSX_PARTITION_BALLOT_PARTS.
RSX_LOCATE_HD u32 partition_rank_form(u32 bins, u32 seam) { return bins <= seam ? 1u : 2u; }
// the bits of a bin number below `bins`
RSX_LOCATE_HD u32 partition_bin_bits(u32 bins)
{
	u32 b = 0;
	while (((u32)1 << b) < bins)
		++b;
	return b;
}

}  // namespace rsx
