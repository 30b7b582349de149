// rsx_join_shape.hpp: the arithmetic of rsx_sort_join* and rsx_join_pairs* (rsx_join.hpp) -- the route rule, the
// size of the table, the grids, and the bookkeeping of the expansion: the pairs are cut into output tiles, the rows into row
// tiles, and a workgroup finds, for every pair position of its output tile, the row tile, the row and the place inside the row's
// run.  Nothing of HIP and nothing of Ctx is used here: every function is __host__ __device__ under hipcc and plain C++
// otherwise; tests/cpp/join_shape_check.cpp includes this file alone and runs a model of the expansion built from it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RSX_JOIN_HD __host__ __device__ inline
#else
#define RSX_JOIN_HD inline
#endif

namespace rsx {

typedef unsigned long long u64;
typedef unsigned int u32;

// rsx_join_info.route and the bit of `flags` (RSX_JOIN_* of rsx.h)
enum : u32 { JOIN_TRIVIAL = 0, JOIN_TABLE = 1, JOIN_SEARCH = 2, JOIN_MERGE = 3 };
enum : u32 { JOIN_LEFT = 1 };
// the expansion: a workgroup of JOIN_THREADS threads per output tile of JOIN_EXPAND_TILE pairs; the rows' counts are summed and
// scanned by tiles of JOIN_ROW_TILE rows (JOIN_ROW_TILE / JOIN_THREADS rows per thread); at most JOIN_EXPAND_MAX_WGS workgroups,
// each taking every gridDim-th output tile
enum : u32 { JOIN_THREADS = 256, JOIN_ROW_TILE = 1024, JOIN_EXPAND_TILE = 4096, JOIN_EXPAND_MAX_WGS = 1u << 20 };
// the table route: at most 2^16 packed values (rsx_rankdata_count16_kernel's), at most eight runs of varying bits
enum : u32 { JOIN_TABLE_MAX_BITS = 16, JOIN_TABLE_MAX_RUNS = 8 };

// ---- the routes ---------------------------------------------------------------------------------------------------------------
RSX_JOIN_HD u32 join_popcount(u64 x)
{
	u32 c = 0;
	for (; x; x &= x - 1)
		++c;
	return c;
}
// the runs of contiguous set bits of the mask of varying bits
RSX_JOIN_HD u32 join_mask_runs(u64 vary)
{
	return join_popcount(vary & ~(vary << 1));
}
// direct addressing: what rsx_rankdata_count16_kernel takes of the RIGHT keys -- at most 16 varying bits in at most eight runs, and
// counts that fit 32 bits
RSX_JOIN_HD bool join_table_ok(u64 vary, u64 m)
{
	return join_popcount(vary) <= JOIN_TABLE_MAX_BITS && join_mask_runs(vary) <= JOIN_TABLE_MAX_RUNS && m < ((u64)1 << 32);
}
// [counts: 65536 u32][offsets: 65537 u64], one-byte keys [counts: 256 u64 + 256 bytes of flags][offsets: 258 u64]
RSX_JOIN_HD u64 join_table_bytes(u32 key_bytes)
{
	return key_bytes == 1 ? 256u * 8u + 256u + 258u * 8u : 65536u * 4u + 65537u * 8u;
}
// the offsets a probe reads: 512 KiB, or 1 KiB for one-byte keys (rsx_join_info.table_bytes)
RSX_JOIN_HD u64 join_table_read_bytes(u32 key_bytes) { return key_bytes == 1 ? 1024u : 65536u * 8u; }
// Sort the left side too (MERGE) instead of searching the left keys as they come (SEARCH)?  A search of a key that comes in no
// order is about log2(m) dependent reads, the upper ones of which hit a cache while the sorted right keys fit one; sorted left
// keys search neighbouring places, at the price of a pairs sort of n and a scatter.  DESIGN.md 4p has the rows this rule is
// taken from (profiles/join/join_probe.txt, 2^26 and 2^28 left rows): with 4 MiB of sorted right keys and more MERGE won every
// row (by 1.03x at the least, by 3.8x to 5.1x from 64 MiB on), with 256 KiB SEARCH did.  Nothing between was measured, and nothing
// below 2^26 left rows: MERGE from JOIN_MERGE_MIN_RIGHT_BYTES of right keys on, for at least JOIN_MERGE_MIN_LEFT left rows.
enum : u64 { JOIN_MERGE_MIN_LEFT = (u64)1 << 22, JOIN_MERGE_MIN_RIGHT_BYTES = (u64)1 << 22 };
RSX_JOIN_HD bool join_use_merge(u64 n, u64 m, u32 key_bytes)
{
	return n >= JOIN_MERGE_MIN_LEFT && m * key_bytes >= JOIN_MERGE_MIN_RIGHT_BYTES;
}
// `force`: RSX_JOIN_FORCE (2, 3: that route; else by the rule), `table`: the table route is open and the right keys fit it
RSX_JOIN_HD u32 join_route(bool table, u32 force, u64 n, u64 m, u32 key_bytes)
{
	if (force == JOIN_SEARCH || force == JOIN_MERGE)
		return force;
	if (table)
		return JOIN_TABLE;
	return join_use_merge(n, m, key_bytes) ? (u32)JOIN_MERGE : (u32)JOIN_SEARCH;
}

// the grid of the searches and of the scatter: workgroups of 256 threads, one item per thread and step, at most 2^16 workgroups
RSX_JOIN_HD u32 join_search_grid(u64 n)
{
	const u64 wgs = (n + 255u) / 256u;
	return (u32)(wgs < 1 ? 1 : wgs > 65536u ? (u64)65536u : wgs);
}

// ---- the expansion ------------------------------------------------------------------------------------------------------------
// the pairs a row yields: its matches, and under LEFT one pair (i, all ones) where it has none
RSX_JOIN_HD u64 join_row_pairs(u64 count, bool left) { return count ? count : (left ? 1u : 0u); }
RSX_JOIN_HD u64 join_tiles(u64 items, u64 tile) { return (items + tile - 1) / tile; }
RSX_JOIN_HD u32 join_expand_grid(u64 out_tiles) { return (u32)(out_tiles < 1 ? 1 : out_tiles > JOIN_EXPAND_MAX_WGS ? (u64)JOIN_EXPAND_MAX_WGS : out_tiles); }

// excl[0 .. T]: the exclusive scan of the row tiles' pairs, excl[T] = all pairs.  The row tile that holds pair p < excl[T]: the
// LAST t with excl[t] <= p (tiles without pairs share their successor's entry and are never found)
template <typename Excl> RSX_JOIN_HD u64 join_find_tile(Excl excl, u64 T, u64 p)
{
	u64 lo = 0, hi = T;   // the answer lies in [lo, hi)
	while (hi - lo > 1) {
		const u64 mid = lo + (hi - lo) / 2;
		if (excl[mid] <= p)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}
// incl[0 .. rows): the inclusive scan of one row tile's pairs.  The row that holds the tile's pair `rel` < incl[rows - 1]: the
// FIRST r with incl[r] > rel (rows without pairs are never found)
template <typename Incl> RSX_JOIN_HD u32 join_find_row(Incl incl, u32 rows, u64 rel)
{
	u32 lo = 0, hi = rows;   // the answer lies in [lo, hi)
	while (hi - lo > 1) {
		const u32 mid = lo + (hi - lo) / 2;
		if (incl[mid - 1] > rel)
			hi = mid;
		else
			lo = mid;
	}
	return lo;
}
// An output tile [p0, p1) is written segment by segment, a segment being its part inside one row tile.  The segment that begins
// at pair p (p0 <= p < p1) lies in row tile t = join_find_tile(p) and ends at min(p1, excl[t + 1]).
struct JoinSegment {
	u64 tile;     // the row tile
	u64 first;    // excl[tile]: the pairs in front of the row tile
	u64 end;      // one past the segment's last pair
};
template <typename Excl> RSX_JOIN_HD JoinSegment join_segment(Excl excl, u64 T, u64 p, u64 p1)
{
	JoinSegment s;
	s.tile = join_find_tile(excl, T, p);
	s.first = excl[s.tile];
	const u64 next = excl[s.tile + 1];
	s.end = next < p1 ? next : p1;
	return s;
}

}  // namespace rsx
