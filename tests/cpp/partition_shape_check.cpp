// partition_shape_check.cpp -- the arithmetic of rsx_sort_partition*'s scatter route (radix_sorting_amd/csrc/rsx_partition_shape.hpp)
// on the CPU: the shares of the grid, the bin-major scan against a serial loop, the read-out of the caller's offsets for repeated
// edges against a brute-force count, the ranking form and the bits of a bin number.  No GPU and no library: the header alone.
// Built by `make cpp`, run by tests/test_partition_shape_cpu.py.  Prints "partition_shape_check OK" and returns 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radix_sorting_amd/csrc/rsx_partition_shape.hpp"

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

// the shares cover [0, n) exactly once, in order; the head lies in the first and the tail in the last; every other boundary is a
// whole number of tiles behind the head; no share but the last is smaller than the smallest share
static void check_grid(u64 n, u64 head)
{
	const PartitionGrid g = partition_grid(n, head);
	const u64 S = (u64)PARTITION_SHARE_TILES * PARTITION_TILE;
	CHECK(g.wgs >= 1 && g.wgs <= PARTITION_MAX_WGS);
	CHECK(g.head == std::min(head, n));
	CHECK(g.share_tiles >= PARTITION_SHARE_TILES);
	u64 at = 0;
	for (u32 w = 0; w < g.wgs; ++w) {
		const u64 lo = partition_share_lo(g, w), hi = partition_share_hi(g, w, n);
		CHECK(lo == at);
		CHECK(hi >= lo && hi <= n);
		if (n)
			CHECK(hi > lo);
		if (w)
			CHECK((lo - g.head) % PARTITION_TILE == 0 && lo >= g.head);
		if (w + 1 < g.wgs)
			CHECK(hi - lo >= S && hi - lo <= g.head + g.share_tiles * PARTITION_TILE);
		else
			CHECK(hi - lo < g.head + (g.share_tiles + 1) * PARTITION_TILE);   // the last: its tiles, the tail (less than a tile), perhaps the head
		at = hi;
	}
	CHECK(at == n);
	CHECK(partition_share_lo(g, 0) == 0 && partition_share_hi(g, g.wgs - 1, n) == n);
}

static void check_grids()
{
	const u64 T = PARTITION_TILE, S = (u64)PARTITION_SHARE_TILES * PARTITION_TILE, W = PARTITION_MAX_WGS;
	std::vector<u64> sizes = {0, 1, 2, 3, 15, 16, 17, 63, 64, 65};
	for (u64 seam : {T, 2 * T, S, 2 * S, 3 * S, W * S, W * S + T, 2 * W * S, 3 * W * S, (u64)1 << 32, ((u64)1 << 32) + T, (u64)1 << 36})
		for (int d = -17; d <= 17; ++d)
			sizes.push_back(seam + (u64)(int64_t)d);
	for (u64 n : sizes)
		for (u64 head : {(u64)0, (u64)1, (u64)3, (u64)7, (u64)15})
			check_grid(n, head);
	for (int i = 0; i < 20000; ++i)
		check_grid(rnd() % (((u64)1 << (10 + rnd() % 28)) + 1), rnd() % 16);
	// the head by address and key size
	CHECK(partition_head(0x1000, 4, 100) == 0 && partition_head(0x1004, 4, 100) == 3 && partition_head(0x1004, 4, 2) == 2);
	CHECK(partition_head(0x1008, 8, 100) == 1 && partition_head(0x100F, 1, 100) == 1 && partition_head(0x1002, 2, 100) == 7);
	// one share while there are at most PARTITION_SHARE_TILES whole tiles, two from one tile more on
	CHECK(partition_grid(S + T - 1, 0).wgs == 1 && partition_grid(S + T, 0).wgs == 2 && partition_grid(S + T + 2, 3).wgs == 1);
	CHECK(partition_grid(W * S, 0).wgs == W && partition_grid(W * S, 0).share_tiles == PARTITION_SHARE_TILES);
	CHECK(partition_grid(W * S + T, 0).share_tiles == PARTITION_SHARE_TILES + 1);
}

// starts and totals against one serial loop in output order: bins ascending, inside a bin the shares ascending
static void check_scan(u32 wgs, u32 bins, u64 most)
{
	std::vector<u64> rows((size_t)wgs * bins), starts((size_t)wgs * bins, ~(u64)0), want((size_t)wgs * bins);
	for (u64 &r : rows)
		r = most ? rnd() % (most + 1) : 0;
	u64 run = 0;
	std::vector<u64> base(bins), total(bins);
	for (u32 b = 0; b < bins; ++b) {
		base[b] = run;
		for (u32 w = 0; w < wgs; ++w) {
			want[(size_t)w * bins + b] = run;
			run += rows[(size_t)w * bins + b];
		}
		total[b] = run - base[b];
	}
	for (u32 b = 0; b < bins; ++b) {
		CHECK(partition_bin_total(rows.data(), wgs, bins, b) == total[b]);
		partition_bin_starts(rows.data(), wgs, bins, b, base[b], starts.data());
	}
	CHECK(starts == want);
}

// offsets[j] = #{ i : bin[i] < j } for keys whose bins are cum[e]: repeated edges give empty parts
static void check_offsets(const std::vector<u64> &edges_sorted, const std::vector<u64> &per_distinct_bin)
{
	const u64 m = edges_sorted.size();
	std::vector<u64> cum;   // cum[d] = the position of the first occurrence of the d-th distinct edge; cum[D] = m
	for (u64 i = 0; i < m; ++i)
		if (locate_is_head<u64>(i, edges_sorted[i], i ? edges_sorted[i - 1] : edges_sorted[i]))
			cum.push_back(i);
	cum.push_back(m);
	const u32 D = (u32)cum.size() - 1;
	CHECK(per_distinct_bin.size() == D + 1u);
	std::vector<u64> excl(D + 2, 0);
	for (u32 e = 0; e <= D; ++e)
		excl[e + 1] = excl[e] + per_distinct_bin[e];
	const u64 n = excl[D + 1];
	for (u64 j = 0; j < m + 2; ++j) {
		u64 want = 0;   // brute force: the keys of distinct bin e have the caller's bin cum[e]
		for (u32 e = 0; e <= D; ++e)
			want += cum[e] < j ? per_distinct_bin[e] : 0;
		const u32 e = partition_offset_entry(cum.data(), D, j);
		CHECK(e <= D + 1);
		CHECK(excl[e] == want);
	}
	CHECK(partition_offset_entry(cum.data(), D, 0) == 0 && excl[partition_offset_entry(cum.data(), D, m + 1)] == n);
}

int main()
{
	check_grids();
	for (u32 wgs : {1u, 2u, 3u, 255u, 256u})
		for (u32 bins : {1u, 2u, 3u, 4u, 5u, 64u, 255u, 256u}) {
			check_scan(wgs, bins, 0);
			check_scan(wgs, bins, 1);
			check_scan(wgs, bins, ((u64)1 << 33));
		}
	check_offsets({5}, {3, 4});
	check_offsets({5, 5, 5}, {3, 4});
	check_offsets({1, 2, 2, 2, 7, 9, 9}, {1, 0, 5, 2, 8});
	check_offsets({4, 4}, {0, 0});
	for (int i = 0; i < 300; ++i) {
		std::vector<u64> e(1 + rnd() % 400);
		for (u64 &x : e)
			x = rnd() % 40;
		std::sort(e.begin(), e.end());
		std::vector<u64> d = e;
		d.erase(std::unique(d.begin(), d.end()), d.end());
		std::vector<u64> per(d.size() + 1);
		for (u64 &x : per)
			x = rnd() % 5 ? rnd() % 1000 : 0;
		check_offsets(e, per);
	}
	// the ranking form and the bits of a bin number
	CHECK(partition_rank_form(2, 4) == 1 && partition_rank_form(4, 4) == 1 && partition_rank_form(5, 4) == 2 && partition_rank_form(2, 0) == 2);
	CHECK(partition_rank_form(256, 256) == 1 && partition_rank_form(256, 255) == 2);
	CHECK(partition_bin_bits(1) == 0 && partition_bin_bits(2) == 1 && partition_bin_bits(3) == 2 && partition_bin_bits(4) == 2 && partition_bin_bits(5) == 3);
	CHECK(partition_bin_bits(128) == 7 && partition_bin_bits(129) == 8 && partition_bin_bits(256) == 8);
	CHECK(PARTITION_TILE == PARTITION_THREADS * PARTITION_KPT && PARTITION_TILE <= 65536 && PARTITION_MAX_BINS == PARTITION_MAX_EDGES + 1);
	CHECK(PARTITION_WAVES * 64 == PARTITION_THREADS);
	if (failures) {
		std::printf("partition_shape_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("partition_shape_check OK\n");
	return 0;
}
