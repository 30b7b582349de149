// join_shape_check.cpp -- the arithmetic of rsx_sort_join* / rsx_join_pairs* (radix_sorting_amd/csrc/rsx_join_shape.hpp) on the CPU:
// the route rule at its edges, the table's size, the grids, and a plain C++ model of the expansion built from the header's own
// functions (join_tiles, join_row_pairs, join_segment, join_find_row) over random count arrays against a naive loop.  No GPU and
// no library: the header alone.  Built by `make cpp`, run by tests/test_join_shape_cpu.py.  Prints "join_shape_check OK" and
// returns 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radix_sorting_amd/csrc/rsx_join_shape.hpp"

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

static void check_routes()
{
	// V = 16 / 17 in one run, in eight runs; 8 / 9 runs; m = 2^32 - 1 / 2^32
	CHECK(join_table_ok(0xFFFFull, 1000));
	CHECK(!join_table_ok(0x1FFFFull, 1000));
	CHECK(join_table_ok(0xFFFFull << 48, 1000));
	CHECK(join_table_ok(0x00F0FF0Full, 1000) && join_popcount(0x00F0FF0Full) == 16 && join_mask_runs(0x00F0FF0Full) == 3);
	CHECK(!join_table_ok(0x01F0FF0Full, 1000) && join_popcount(0x01F0FF0Full) == 17);
	const u64 eight = 0x5555ull, nine = 0x15555ull;   // eight / nine runs of one bit
	CHECK(join_mask_runs(eight) == 8 && join_table_ok(eight, 1000));
	CHECK(join_mask_runs(nine) == 9 && join_popcount(nine) == 9 && !join_table_ok(nine, 1000));
	CHECK(join_table_ok(0x0303030303030303ull, 5) && join_mask_runs(0x0303030303030303ull) == 8);
	CHECK(join_table_ok(0xFFull, ((u64)1 << 32) - 1));
	CHECK(!join_table_ok(0xFFull, (u64)1 << 32));
	CHECK(join_table_ok(0, 1) && join_mask_runs(0) == 0);
	CHECK(join_mask_runs(~0ull) == 1 && join_mask_runs(1ull << 63) == 1 && join_mask_runs((1ull << 63) | 1) == 2);
	for (int it = 0; it < 2000; ++it) {
		const u64 v = rnd() & rnd();
		u32 runs = 0, bits = 0;
		for (u32 b = 0; b < 64; ++b) {
			bits += (v >> b) & 1;
			runs += ((v >> b) & 1) && (b == 0 || !((v >> (b - 1)) & 1));
		}
		CHECK(join_popcount(v) == bits && join_mask_runs(v) == runs);
	}
	// a forced route wins over the table, the table over the rule; the rule is join_use_merge's
	for (u32 kb = 1; kb <= 8; kb *= 2)
		for (u64 n : {(u64)1, (u64)5000, JOIN_MERGE_MIN_LEFT - 1, (u64)JOIN_MERGE_MIN_LEFT, (u64)1 << 28})
			for (u64 m : {(u64)1, (u64)3000, JOIN_MERGE_MIN_RIGHT_BYTES / kb - 1, JOIN_MERGE_MIN_RIGHT_BYTES / kb, (u64)1 << 28}) {
				CHECK(join_route(true, 2, n, m, kb) == JOIN_SEARCH && join_route(false, 2, n, m, kb) == JOIN_SEARCH);
				CHECK(join_route(true, 3, n, m, kb) == JOIN_MERGE && join_route(false, 3, n, m, kb) == JOIN_MERGE);
				CHECK(join_route(true, 0, n, m, kb) == JOIN_TABLE && join_route(true, 1, n, m, kb) == JOIN_TABLE);
				const bool merge = n >= JOIN_MERGE_MIN_LEFT && m * kb >= JOIN_MERGE_MIN_RIGHT_BYTES;
				CHECK(join_use_merge(n, m, kb) == merge);
				CHECK(join_route(false, 0, n, m, kb) == (merge ? (u32)JOIN_MERGE : (u32)JOIN_SEARCH));
			}
	CHECK(join_table_read_bytes(1) == 1024 && join_table_read_bytes(2) == 512 * 1024 && join_table_read_bytes(8) == 512 * 1024);
	CHECK(join_table_bytes(1) == 256 * 8 + 256 + 258 * 8 && join_table_bytes(4) == 65536 * 4 + 65537 * 8);
	CHECK(JOIN_ROW_TILE % JOIN_THREADS == 0 && JOIN_EXPAND_TILE % JOIN_THREADS == 0);
	CHECK(join_expand_grid(0) == 1 && join_expand_grid(1) == 1 && join_expand_grid(777) == 777);
	CHECK(join_expand_grid(JOIN_EXPAND_MAX_WGS) == JOIN_EXPAND_MAX_WGS && join_expand_grid((u64)1 << 40) == JOIN_EXPAND_MAX_WGS);
	CHECK(join_search_grid(0) == 1 && join_search_grid(256) == 1 && join_search_grid(257) == 2 && join_search_grid((u64)1 << 40) == 65536);
	CHECK(join_tiles(0, 7) == 0 && join_tiles(7, 7) == 1 && join_tiles(8, 7) == 2);
	CHECK(join_row_pairs(0, false) == 0 && join_row_pairs(0, true) == 1 && join_row_pairs(5, false) == 5 && join_row_pairs(5, true) == 5);
}

// the scanned row-tile sums as rsx_join_rowsums_kernel and rsx_join_scan_kernel leave them
static std::vector<u64> tile_scan(const std::vector<u64> &count, bool left, u64 row_tile)
{
	const u64 n = count.size(), T = join_tiles(n, row_tile);
	std::vector<u64> excl(T + 1, 0);
	for (u64 t = 0; t < T; ++t) {
		u64 sum = 0;
		for (u64 i = t * row_tile; i < std::min(n, (t + 1) * row_tile); ++i)
			sum += join_row_pairs(count[i], left);
		excl[t + 1] = excl[t] + sum;
	}
	return excl;
}

// output tile `o` as rsx_join_expand_kernel walks it: visit(q, row, t) for the pairs q the filter `want` names
template <typename Want, typename Visit>
static void expand_tile(const std::vector<u64> &count, bool left, u64 row_tile, u64 out_tile, const std::vector<u64> &excl, u64 o, Want want, Visit visit)
{
	const u64 n = count.size(), T = join_tiles(n, row_tile), n_pairs = excl[T];
	const u64 p0 = o * out_tile, p1 = std::min(p0 + out_tile, n_pairs);
	u64 p = p0, guard = 0;
	std::vector<u64> incl(row_tile);
	while (p < p1) {
		const JoinSegment seg = join_segment(excl.data(), T, p, p1);
		CHECK(seg.tile < T && seg.first <= p && seg.end > p && seg.end <= p1 && seg.first == excl[seg.tile]);
		if (!(seg.end > p) || ++guard > out_tile + 1)
			return;   // (a model that does not advance is a failure, not a hang)
		const u64 row0 = seg.tile * row_tile;
		const u32 rows = (u32)std::min<u64>(row_tile, n - row0);
		u64 run = 0;
		for (u32 r = 0; r < rows; ++r)
			incl[r] = run += join_row_pairs(count[row0 + r], left);
		CHECK(seg.first + run == excl[seg.tile + 1]);
		for (u64 q = p; q < seg.end; ++q) {
			if (!want(q))
				continue;
			const u64 rel = q - seg.first;
			const u32 r = join_find_row(incl.data(), rows, rel);
			const u64 before = r ? incl[r - 1] : 0;
			CHECK(r < rows && before <= rel && rel < incl[r]);
			visit(q, row0 + r, rel - before);
		}
		p = seg.end;
	}
}

// every pair position exactly once, and as a naive loop over the rows produces them
static void check_expansion(const std::vector<u64> &count, bool left, u64 row_tile, u64 out_tile)
{
	std::vector<u64> want_row, want_t;
	for (u64 i = 0; i < count.size(); ++i)
		for (u64 t = 0; t < join_row_pairs(count[i], left); ++t) {
			want_row.push_back(i);
			want_t.push_back(t);
		}
	const std::vector<u64> excl = tile_scan(count, left, row_tile);
	const u64 n_pairs = excl.back();
	CHECK(n_pairs == want_row.size());
	std::vector<u32> seen(n_pairs, 0);
	const u64 tiles = join_tiles(n_pairs, out_tile);
	for (u64 o = 0; o < tiles; ++o)
		expand_tile(count, left, row_tile, out_tile, excl, o, [](u64) { return true; }, [&](u64 q, u64 row, u64 t) {
			CHECK(q < n_pairs);
			if (q < n_pairs) {
				++seen[q];
				CHECK(row == want_row[q] && t == want_t[q]);
			}
		});
	for (u64 q = 0; q < n_pairs; ++q)
		CHECK(seen[q] == 1);
}

static void check_model()
{
	const u64 tiles[4] = {1, 2, 7, 64};
	for (u64 rt : tiles)
		for (u64 ot : tiles)
			for (int left = 0; left < 2; ++left) {
				// random counts with runs of zeros that span whole row tiles and rows larger than several output tiles
				for (int it = 0; it < 12; ++it) {
					const u64 n = 1 + rnd() % (5 * rt + 3);
					std::vector<u64> count(n);
					for (u64 i = 0; i < n;) {
						const u64 kind = rnd() % 4;
						if (kind == 0) {   // a run of zeros, at least two row tiles long
							for (u64 j = 0, len = 2 * rt + rnd() % (rt + 1); j < len && i < n; ++j)
								count[i++] = 0;
						} else if (kind == 1) {   // one large row
							count[i++] = 3 * ot + 1 + rnd() % (2 * ot);
						} else {
							count[i++] = rnd() % 4;
						}
					}
					check_expansion(count, left != 0, rt, ot);
				}
				// totals of k * tile and k * tile +- 1: ones, and the last row makes up the difference
				for (u64 k = 1; k <= 3; ++k)
					for (int d = -1; d <= 1; ++d) {
						const u64 total = k * ot + d;
						if (total == 0)
							continue;
						std::vector<u64> count(total / 2 + 1, 1);
						count.back() = total - total / 2;
						check_expansion(count, left != 0, rt, ot);
						std::vector<u64> one(3 * rt + 1, 0);   // one row holds them all, rows without a match in front and behind
						one[rt + rt / 2] = total;
						check_expansion(one, left != 0, rt, ot);
					}
				// first and last row without a match, and nothing but such rows
				check_expansion({0, 3, 0, 0, 2, 0}, left != 0, rt, ot);
				check_expansion(std::vector<u64>(3 * rt + 1, 0), left != 0, rt, ot);
			}
}

// totals above 2^32, by arithmetic only: the library's tiles, a few rows of about 2^31 matches among small ones; of every sampled
// output tile the first and the last pair against a search of the rows' prefix sums
static void check_large()
{
	for (int left = 0; left < 2; ++left) {
		const u64 n = 3 * JOIN_ROW_TILE + 17;
		std::vector<u64> count(n), prefix(n + 1, 0);
		for (u64 i = 0; i < n; ++i)
			count[i] = rnd() % 3;
		for (u64 i : {(u64)5, (u64)JOIN_ROW_TILE - 1, (u64)JOIN_ROW_TILE, (u64)2 * JOIN_ROW_TILE + 100, n - 1})
			count[i] = ((u64)1 << 31) + rnd() % 1000;
		for (u64 i = 0; i < n; ++i)
			prefix[i + 1] = prefix[i] + join_row_pairs(count[i], left != 0);
		const std::vector<u64> excl = tile_scan(count, left != 0, JOIN_ROW_TILE);
		const u64 n_pairs = excl.back();
		CHECK(n_pairs == prefix[n] && n_pairs > ((u64)1 << 33));
		const u64 tiles = join_tiles(n_pairs, JOIN_EXPAND_TILE);
		for (int it = 0; it < 600; ++it) {
			const u64 o = it == 0 ? 0 : it == 1 ? tiles - 1 : it < 300 ? rnd() % tiles : (prefix[1 + rnd() % n] / JOIN_EXPAND_TILE) % tiles;
			const u64 p0 = o * JOIN_EXPAND_TILE, p1 = std::min(p0 + JOIN_EXPAND_TILE, n_pairs);
			u32 visited = 0;
			expand_tile(count, left != 0, JOIN_ROW_TILE, JOIN_EXPAND_TILE, excl, o, [&](u64 q) { return q == p0 || q == p1 - 1; }, [&](u64 q, u64 row, u64 t) {
				++visited;
				const u64 want = (u64)(std::upper_bound(prefix.begin(), prefix.end(), q) - prefix.begin()) - 1;
				CHECK(row == want && t == q - prefix[want]);
			});
			CHECK(visited == (p1 - p0 > 1 ? 2u : 1u));
		}
	}
}

int main()
{
	check_routes();
	check_model();
	check_large();
	if (failures) {
		std::printf("join_shape_check: %d failures\n", failures);
		return 1;
	}
	std::printf("join_shape_check OK\n");
	return 0;
}
