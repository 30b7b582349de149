// reduce_shape_check.cpp -- the arithmetic of rsx_sort_reduce* (radix_sorting_amd/csrc/rsx_reduce_shape.hpp) on the CPU: the bytes
// of a cell, the copies that fit a workgroup's LDS and where their parts lie, the widest table that fits, the grid, and the seam
// rule of the sort route against a brute-force reduction of the runs of random sorted arrays.  No GPU and no library: the header
// alone.  Built by `make cpp`, run by tests/test_reduce_shape_cpu.py.  Prints "reduce_shape_check OK" and returns 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radix_sorting_amd/csrc/rsx_reduce_shape.hpp"

using namespace rsx;

static int failures = 0;
#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			if (failures < 20)                                              \
				std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			++failures;                                                     \
		}                                                                   \
	} while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
	return rng_state;
}

// every ops mask x value width x V x forced: the layout against a byte map (no part overlaps another, every part aligned, all
// inside `bytes`), the copies against a linear search
static void check_lds()
{
	for (u32 ops = 0; ops < 8; ++ops)
		for (u32 vb = 4; vb <= 8; vb += 4) {
			const u32 cb = reduce_cell_bytes(ops, vb);
			CHECK(cb == 4 + ((ops & 1) ? 8 : 0) + ((ops & 2) ? vb : 0) + ((ops & 4) ? vb : 0));
			u32 fit = 0;
			for (u32 v = 0; v <= REDUCE_LDS_MAX_BITS; ++v)
				if ((((u64)1 << v) * cb) <= REDUCE_LDS_ONE)
					fit = v;
			CHECK(reduce_lds_fit_bits(cb) == fit);
			CHECK(fit == REDUCE_LDS_MAX_BITS);   // 2^12 cells of at most 28 bytes are what REDUCE_LDS_ONE was sized for
			for (u32 v = 1; v <= REDUCE_LDS_MAX_BITS + 1; ++v)
				for (u32 forced = 0; forced <= 33; ++forced) {
					const u32 r = reduce_replicas(v, cb, forced);
					if (v > REDUCE_LDS_MAX_BITS) {
						CHECK(r == 0);
						continue;
					}
					// brute force: the largest power of two, at most 32 (and at most `forced`), whose copies fit the budget
					u32 want = 0;
					for (u32 p = 1; p <= REDUCE_MAX_SETS; p *= 2)
						if ((u64)p * (((u64)1 << v) * cb) <= REDUCE_LDS_BUDGET && (!forced || p <= forced))
							want = p;
					CHECK(r == want);
					CHECK(r >= 1 && (r & (r - 1)) == 0);
					const ReduceLds l = reduce_lds(v, ops, vb, forced);
					const u32 C = 1u << v;
					CHECK(l.sets == r && l.bytes == l.sets * l.stride && l.bytes <= REDUCE_LDS_BUDGET + 8 * REDUCE_MAX_SETS);
					CHECK(l.stride % 8 == 0 && l.stride >= C * cb && l.stride < C * cb + 8);
					std::vector<unsigned char> map(l.stride, 0);
					auto claim = [&](u32 off, u32 each, bool on) {
						if (!on)
							return;
						CHECK(off % each == 0);
						for (u32 b = off; b < off + each * C; ++b) {
							CHECK(b < l.stride && !map[b]);
							if (b < l.stride)
								map[b] = 1;
						}
					};
					claim(l.sum_off, 8, ops & REDUCE_SUM);
					claim(l.min_off, vb, ops & REDUCE_MIN);
					claim(l.max_off, vb, ops & REDUCE_MAX);
					claim(l.cnt_off, 4, true);
				}
		}
	// the budget holds with the padding of the stride: the largest copy
	CHECK(reduce_lds(12, 7, 8, 0).bytes == 4096 * 28 && reduce_lds(12, 7, 8, 0).sets == 1);
	CHECK(reduce_lds(8, 1, 4, 0).sets == 32 && reduce_lds(8, 1, 4, 0).bytes == 32 * 256 * 12);
	CHECK(reduce_lds(8, 1, 4, 1).sets == 1 && reduce_lds(8, 1, 4, 5).sets == 4);
	for (u32 ops = 0; ops < 8; ++ops)
		for (u32 vb = 4; vb <= 8; vb += 4)
			for (u32 v = 1; v <= 12; ++v)
				CHECK(reduce_lds(v, ops, vb, 0).bytes <= REDUCE_LDS_BUDGET);
	CHECK(reduce_table_bytes(12, 4) == 4096 * 24 && reduce_table_bytes(24, 8) == ((u64)32 << 24));
}

static void check_grid()
{
	CHECK(reduce_step_elems(1, 4) == 16 && reduce_step_elems(1, 8) == 16 && reduce_step_elems(4, 4) == 4 && reduce_step_elems(8, 4) == 4 &&
	      reduce_step_elems(8, 8) == 2 && reduce_step_elems(2, 8) == 8 && reduce_step_elems(4, 8) == 4);
	for (u32 e : {2u, 4u, 8u, 16u})
		for (u64 n : {(u64)0, (u64)1, (u64)77, (u64)1 << 16, ((u64)1 << 20) + 3, (u64)1 << 28, (u64)1 << 34, (u64)1 << 41}) {
			const u32 g = reduce_grid(n, e);
			CHECK(g >= 1 && g <= REDUCE_MAX_WGS);
			// every workgroup but the only one has at least REDUCE_SHARE_STEPS steps per thread
			if (g > 1)
				CHECK(n / e / g >= (u64)REDUCE_THREADS * REDUCE_SHARE_STEPS);
			if (g < REDUCE_MAX_WGS)
				CHECK(n / e < (u64)(g + 1) * REDUCE_THREADS * REDUCE_SHARE_STEPS);
			CHECK(reduce_share_fits(n, g) == ((n + g - 1) / g + 64 < ((u64)1 << 32)));
		}
	CHECK(reduce_share_fits((u64)1 << 34, 256) && !reduce_share_fits((u64)1 << 41, 256) && !reduce_share_fits((u64)1 << 32, 1));
}

// A sorted array of `n` keys cut into tiles of `tile`: per tile the records the runs kernel leaves, then every run that is open at
// a tile's end combined by the seam rule -- the sums of ALL runs against a plain loop over the array.  Sums of a run that ends
// inside the tile it began in are the tile's own; the check is that lead / tail / seam together cover every element once.
static void check_seams(u64 n, u64 tile, u32 distinct)
{
	std::vector<u32> key(n);
	std::vector<u64> val(n);
	for (u64 i = 0; i < n; ++i) {
		key[i] = (u32)(rnd() % distinct);
		val[i] = rnd() >> 8;
	}
	std::sort(key.begin(), key.end());
	std::vector<u64> want;   // per run
	for (u64 i = 0; i < n; ++i) {
		if (i == 0 || key[i] != key[i - 1])
			want.push_back(0);
		want.back() += val[i];
	}
	const u64 tiles = (n + tile - 1) / tile;
	std::vector<u64> heads(tiles, 0), before(tiles, 0), lead(tiles, 0), tail(tiles, 0);
	std::vector<u64> got(want.size(), 0);
	std::vector<int> written(want.size(), 0);
	u64 g = 0;   // heads so far
	for (u64 t = 0; t < tiles; ++t) {
		before[t] = g;
		u64 open = 0;
		bool seen = false;
		for (u64 i = t * tile; i < std::min(n, (t + 1) * tile); ++i) {
			if (i == 0 || key[i] != key[i - 1]) {
				if (seen) {           // a run inside the tile: written by the runs kernel
					got[g - 1] = open;
					++written[g - 1];
				} else {
					lead[t] = open;
				}
				seen = true;
				++heads[t];
				++g;
				open = 0;
			}
			open += val[i];
		}
		if (seen)
			tail[t] = open;
		else
			lead[t] = open;
	}
	CHECK(g == want.size());
	for (u64 t = 0; t < tiles; ++t) {
		if (!heads[t])
			continue;
		const u64 last = reduce_seam_last(t, tiles, [&](u64 e) { return heads[e] != 0; });
		CHECK(last >= t && last < tiles);
		// brute force: the tile in which the first head behind tile t lies, or the last tile
		u64 bf = tiles - 1;
		for (u64 e = t + 1; e < tiles; ++e)
			if (heads[e]) {
				bf = e;
				break;
			}
		CHECK(last == bf);
		u64 s = tail[t];
		for (u64 e = t + 1; e <= last; ++e)
			s += lead[e];
		const u64 run = before[t] + heads[t] - 1;
		got[run] = s;
		++written[run];
	}
	for (size_t r = 0; r < want.size(); ++r) {
		CHECK(written[r] == 1);
		CHECK(got[r] == want[r]);
	}
}

int main()
{
	check_lds();
	check_grid();
	for (u64 tile : {(u64)1, (u64)2, (u64)7, (u64)64})
		for (u32 distinct : {1u, 2u, 5u, 40u, 100000u})
			for (u64 n : {(u64)1, (u64)2, tile - 1, tile, tile + 1, 3 * tile, 3 * tile + 5, (u64)1000, (u64)4099})
				if (n)
					check_seams(n, tile, distinct);
	if (failures) {
		std::printf("reduce_shape_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("reduce_shape_check OK\n");
	return 0;
}
