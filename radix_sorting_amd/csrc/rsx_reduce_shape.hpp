// rsx_reduce_shape.hpp: the arithmetic of rsx_sort_reduce* (rsx_reduce.hpp) -- the bytes of a cell, how many copies
// of the cells a workgroup keeps in its LDS and where their parts lie, the widest table that fits, the table in device memory,
// the shares of the sweep, and the seam rule of the sort route: which tiles' records the run that is open at the end of a tile
// is combined from.  Nothing of HIP and nothing of Ctx is used here: every function is __host__ __device__ under hipcc and plain
// C++ otherwise; tests/cpp/reduce_shape_check.cpp includes this file alone and checks it on the CPU against brute force.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RSX_REDUCE_HD __host__ __device__ inline
#else
#define RSX_REDUCE_HD inline
#endif

namespace rsx {

typedef unsigned long long u64;
typedef unsigned int u32;

// the bits of `ops` (RSX_REDUCE_* of rsx.h) and, beside them in the kernels' flags, "4-byte integer values are sign-extended"
enum : u32 { REDUCE_SUM = 1, REDUCE_MIN = 2, REDUCE_MAX = 4, REDUCE_OPS = 7, REDUCE_SIGNED = 8 };
// One workgroup of REDUCE_THREADS threads per CU; its copies of the cells take at most REDUCE_LDS_BUDGET bytes, one copy at most
// REDUCE_LDS_ONE (2^12 cells of 28 bytes); at most REDUCE_MAX_SETS copies.  A share is at least REDUCE_SHARE_STEPS steps per thread.
enum : u32 { REDUCE_THREADS = 1024, REDUCE_MAX_WGS = 256, REDUCE_LDS_BUDGET = 131072, REDUCE_LDS_ONE = 114688, REDUCE_MAX_SETS = 32,
             REDUCE_LDS_MAX_BITS = 12, REDUCE_GLOBAL_MAX_BITS = 24, REDUCE_SHARE_STEPS = 16 };

// ---- a cell ---------------------------------------------------------------------------------------------------------------
// a u32 count and, where wanted, a 64-bit sum, a minimum and a maximum of the value's width
RSX_REDUCE_HD u32 reduce_cell_bytes(u32 ops, u32 val_bytes)
{
	return 4u + ((ops & REDUCE_SUM) ? 8u : 0u) + ((ops & REDUCE_MIN) ? val_bytes : 0u) + ((ops & REDUCE_MAX) ? val_bytes : 0u);
}

RSX_REDUCE_HD u32 reduce_floor_pow2(u32 x)
{
	u32 p = 1;
	while (p * 2u <= x && p * 2u != 0u)
		p *= 2u;
	return x ? p : 0u;
}

// R: as many copies of 2^vbits cells as fit the budget, a power of two, at most REDUCE_MAX_SETS (`forced`: RSX_REDUCE_REPLICAS,
// brought down to a power of two that fits); 0: not even one copy fits
RSX_REDUCE_HD u32 reduce_replicas(u32 vbits, u32 cell_bytes, u32 forced)
{
	if (vbits > REDUCE_LDS_MAX_BITS)
		return 0;
	const u64 one = ((u64)1 << vbits) * cell_bytes;
	if (one > REDUCE_LDS_ONE)
		return 0;
	u64 fit = REDUCE_LDS_BUDGET / one;
	fit = fit > REDUCE_MAX_SETS ? (u64)REDUCE_MAX_SETS : fit;
	const u32 r = reduce_floor_pow2((u32)fit);
	return forced && forced < r ? reduce_floor_pow2(forced) : r;
}

// the largest V of which one copy of the cells fits a workgroup's LDS
RSX_REDUCE_HD u32 reduce_lds_fit_bits(u32 cell_bytes)
{
	u32 v = 0;
	while (v < REDUCE_LDS_MAX_BITS && ((u64)2 << v) * cell_bytes <= REDUCE_LDS_ONE)
		++v;
	return v;
}

// ---- the workgroup's LDS: R copies of [sums: C u64][minima: C values][maxima: C values][counts: C u32], parts that are not
// wanted left out; every part is 8-byte aligned where it holds 8-byte words (C is even: vbits >= 1)
struct ReduceLds {
	u32 sum_off, min_off, max_off, cnt_off, stride, sets, bytes;
};
RSX_REDUCE_HD ReduceLds reduce_lds(u32 vbits, u32 ops, u32 val_bytes, u32 forced)
{
	const u32 C = 1u << vbits;
	ReduceLds l;
	l.sum_off = 0;
	l.min_off = l.sum_off + ((ops & REDUCE_SUM) ? 8u * C : 0u);
	l.max_off = l.min_off + ((ops & REDUCE_MIN) ? val_bytes * C : 0u);
	l.cnt_off = l.max_off + ((ops & REDUCE_MAX) ? val_bytes * C : 0u);
	l.stride = (l.cnt_off + 4u * C + 7u) & ~7u;
	l.sets = reduce_replicas(vbits, reduce_cell_bytes(ops, val_bytes), forced);
	l.bytes = l.sets * l.stride;
	return l;
}

// ---- the table in device memory: [counts: C u64][sums: C u64][minima: C values][maxima: C values], all parts always there
RSX_REDUCE_HD u64 reduce_table_bytes(u32 vbits, u32 val_bytes) { return ((u64)1 << vbits) * (16u + 2u * val_bytes); }

// ---- the sweep --------------------------------------------------------------------------------------------------------------
// A thread takes `elems` = max(16 / key bytes, 16 / value bytes) elements per step: whole 16-byte vectors of both arrays.
RSX_REDUCE_HD u32 reduce_step_elems(u32 key_bytes, u32 val_bytes)
{
	const u32 a = 16u / key_bytes, b = 16u / val_bytes;
	return a > b ? a : b;
}
// workgroups: one per REDUCE_SHARE_STEPS steps of every thread, at least one, at most one per CU
RSX_REDUCE_HD u32 reduce_grid(u64 n, u32 elems)
{
	const u64 wgs = n / elems / ((u64)REDUCE_THREADS * REDUCE_SHARE_STEPS);
	return (u32)(wgs < 1 ? 1 : wgs > REDUCE_MAX_WGS ? (u64)REDUCE_MAX_WGS : wgs);
}
// the counts of a workgroup's copy are 32 bits wide: its share (and workgroup 0's head and tail) must stay below 2^32 elements
RSX_REDUCE_HD bool reduce_share_fits(u64 n, u32 grid) { return (n + grid - 1) / grid + 64u < ((u64)1 << 32); }

// ---- the seams of the sort route ----------------------------------------------------------------------------------------------
// The sorted array is cut into tiles.  A tile with a head leaves two records: its lead (the elements before its first head) and
// its tail (the elements from its last head on: a run that is still open at the tile's end); a tile without a head is all lead.
// The run that is open at the end of tile t is its tail and the leads of the tiles t + 1 .. reduce_seam_last(t) -- up to and
// including the first one that has a head, or the last tile.
template <typename HasHead> RSX_REDUCE_HD u64 reduce_seam_last(u64 t, u64 tiles, HasHead has_head)
{
	u64 e = t;
	while (e + 1 < tiles) {
		++e;
		if (has_head(e))
			break;
	}
	return e;
}

}  // namespace rsx
