// locate_shape_check.cpp -- the arithmetic of rsx_sort_locate*'s search route (radix_sorting_amd/csrc/rsx_locate_shape.hpp) on the CPU:
// the edges and cum of duplicate-heavy values, the start table and the per-key search against std::upper_bound, the finish against
// brute-force less / equal, the LDS layout and the grid.  No GPU and no library: the header alone.  Built by `make cpp`, run by
// tests/test_locate_shape_cpu.py.  Prints "locate_shape_check OK" and returns 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radix_sorting_amd/csrc/rsx_locate_shape.hpp"

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

template <typename KT> struct Prepared {
	std::vector<KT> E;
	std::vector<u64> cum;
	u32 start[LOCATE_START_ENTRIES];
	u32 shift, steps;
};

// what the prepare kernel does, one position after the other: `values` in any order, repeats allowed
template <typename KT> static Prepared<KT> prepare(std::vector<KT> values)
{
	std::sort(values.begin(), values.end());
	Prepared<KT> p;
	for (u64 i = 0; i < values.size(); ++i)
		if (locate_is_head<KT>(i, values[i], i ? values[i - 1] : values[i])) {
			p.E.push_back(values[i]);
			p.cum.push_back(i);
		}
	p.cum.push_back(values.size());
	const u32 D = (u32)p.E.size();
	p.shift = locate_shift<KT>(p.E[0], p.E[D - 1]);
	for (u32 d = 0; d < LOCATE_START_ENTRIES; ++d)
		p.start[d] = locate_start_entry<KT>(p.E.data(), D, p.shift, d);
	p.steps = locate_steps(locate_max_span(p.start));
	return p;
}

// every key within one of any edge, 0 and all-ones: the search against std::upper_bound, eq against a lookup; then the keys
// counted as the kernel counts them and the finish against brute force; cum against brute force
template <typename KT> static void check_case(const char *name, const std::vector<KT> &values, int want_steps = -1)
{
	const Prepared<KT> p = prepare(values);
	const u32 D = (u32)p.E.size();
	CHECK(D >= 1 && D <= LOCATE_MAX_VALUES);
	CHECK(p.steps <= 12);
	if (want_steps >= 0)
		CHECK(p.steps == (u32)want_steps);
	CHECK(p.start[0] == 0 && p.start[256] == D - 1);
	for (u32 d = 0; d < 256; ++d)
		CHECK(p.start[d] <= p.start[d + 1]);
	std::vector<KT> keys = {(KT)0, (KT)~(KT)0};
	for (KT e : p.E) {
		keys.push_back(e);
		keys.push_back((KT)(e - 1));
		keys.push_back((KT)(e + 1));
	}
	std::vector<u64> cnt(locate_counters(D), 0);
	size_t bad = 0;
	for (KT k : keys) {
		u32 eq = 7;
		const u32 b = locate_search<KT, u32>(p.E.data(), D, p.start, p.shift, p.steps, k, &eq);
		const u32 want_b = (u32)(std::upper_bound(p.E.begin(), p.E.end(), k) - p.E.begin());
		const u32 want_eq = std::binary_search(p.E.begin(), p.E.end(), k) ? 1u : 0u;
		if (b != want_b || eq != want_eq)
			++bad;
		else
			cnt[locate_counter(b, eq)] += 1;
		// the bins: values at or below the key, values strictly below it
		u64 at_or_below = 0, strictly = 0;
		if (values.size() <= 6000 && keys.size() <= 1000) {
			for (KT v : values) {
				at_or_below += v <= k;
				strictly += v < k;
			}
			CHECK(p.cum[locate_bin_entry(want_b, want_eq, false)] == at_or_below);
			CHECK(p.cum[locate_bin_entry(want_b, want_eq, true)] == strictly);
		}
	}
	if (bad)
		std::printf("%s: %zu of %zu keys searched wrongly\n", name, bad, keys.size());
	CHECK(bad == 0);
	// cum against a count of its own definition
	{
		std::vector<KT> sorted = values;
		std::sort(sorted.begin(), sorted.end());
		CHECK(p.cum[0] == 0 && p.cum[D] == values.size());
		for (u32 b = 1; b <= D; ++b)
			CHECK(p.cum[b] == (u64)(std::upper_bound(sorted.begin(), sorted.end(), p.E[b - 1]) - sorted.begin()));
	}
	// the finish: incl over the bin totals, less / equal of every edge against the sorted keys
	std::vector<u64> incl(D + 1);
	u64 run = 0;
	for (u32 b = 0; b <= D; ++b)
		incl[b] = run += locate_total(cnt.data(), b);
	CHECK(run == keys.size());
	std::sort(keys.begin(), keys.end());
	for (u32 d = 0; d < D; ++d) {
		const u64 lo = (u64)(std::lower_bound(keys.begin(), keys.end(), p.E[d]) - keys.begin());
		const u64 hi = (u64)(std::upper_bound(keys.begin(), keys.end(), p.E[d]) - keys.begin());
		CHECK(locate_less(incl.data(), d) == lo);
		CHECK(locate_equal(cnt.data(), d) == hi - lo);
	}
}

template <typename KT> static std::vector<KT> distinct_random(u32 D, KT mask, KT base)
{
	std::vector<KT> v;
	while (v.size() < D) {
		v.push_back((KT)(((KT)rnd() & mask) | base));
		if (v.size() == D) {
			std::sort(v.begin(), v.end());
			v.erase(std::unique(v.begin(), v.end()), v.end());
		}
	}
	for (size_t i = v.size(); i > 1; --i)   // the caller's order is any order
		std::swap(v[i - 1], v[rnd() % i]);
	return v;
}

template <typename KT> static void cases_for_width()
{
	const KT ones = (KT)~(KT)0;
	const u32 W = 8 * sizeof(KT);
	for (u32 D : {1u, 2u, 255u, 256u, 257u, 4096u})
		check_case<KT>("random", distinct_random<KT>(D, ones, 0));
	{   // every edge but the last inside one digit: the longest search there is
		std::vector<KT> v;
		for (u32 i = 0; i < 4095; ++i)
			v.push_back((KT)(1000 + i));
		v.push_back((KT)((KT)1 << (W - 1)));
		check_case<KT>("one digit", v, 12);
		v.clear();
		for (u32 i = 0; i < 100; ++i)
			v.push_back((KT)(5 + 2 * i));
		v.push_back((KT)((KT)3 << (W - 2)));
		check_case<KT>("one digit, 100", v, 7);
	}
	{   // exactly two digits
		std::vector<KT> v;
		for (u32 i = 0; i < 300; ++i) {
			v.push_back((KT)(((KT)0x40 << (W - 8)) + 3 * i));
			v.push_back((KT)(((KT)0xC1 << (W - 8)) + 5 * i));
		}
		check_case<KT>("two digits", v);
	}
	// shared prefixes: none, all but the last bit
	check_case<KT>("prefix 0", distinct_random<KT>(500, ones, 0));
	check_case<KT>("prefix W - 1", std::vector<KT>{(KT)0x12345676, (KT)0x12345677});
	check_case<KT>("prefix 24, 200", distinct_random<KT>(200, (KT)0xFF, (KT)(ones << 8)));
	// the ends of the key space
	check_case<KT>("zero and ones", std::vector<KT>{0, ones});
	check_case<KT>("zero", std::vector<KT>{0});
	check_case<KT>("ones", std::vector<KT>{ones});
	check_case<KT>("ends and middle", std::vector<KT>{0, 1, (KT)(ones - 1), ones, (KT)(ones / 2), (KT)(ones / 2 + 1)});
	{   // duplicate-heavy values
		std::vector<KT> v;
		for (u32 i = 0; i < 5000; ++i)
			v.push_back((KT)((rnd() % 37) * 1000003u));
		check_case<KT>("duplicates", v);
		std::vector<KT> same(777, (KT)42);
		check_case<KT>("all the same", same, 0);
	}
}

int main()
{
	cases_for_width<uint32_t>();
	cases_for_width<u64>();
	// u32 with a 31-bit prefix, u64 with 31-, 56- and 63-bit prefixes
	check_case<uint32_t>("u32 prefix 31", std::vector<uint32_t>{0xDEADBEEEu, 0xDEADBEEFu});
	for (u32 prefix : {31u, 56u, 63u}) {
		const u64 low = prefix == 63 ? 1ull : (1ull << (64 - prefix)) - 1;
		const u64 base = 0xA5C3E1F00F1E3C5Aull & ~low;
		const u32 D = (u32)std::min<u64>(low + 1, 300);
		std::vector<u64> v = distinct_random<u64>(D, low, base);
		v.push_back(base);          // both ends of the range, so that exactly `prefix` bits are shared
		v.push_back(base | low);
		const Prepared<u64> p = prepare(v);
		CHECK(p.shift == (64 - prefix > 8 ? 64 - prefix - 8 : 0));
		check_case<u64>("u64 prefix", v);
	}
	// steps
	CHECK(locate_steps(0) == 0 && locate_steps(1) == 1 && locate_steps(2) == 2 && locate_steps(3) == 2 && locate_steps(4) == 3);
	CHECK(locate_steps(4095) == 12 && locate_steps(255) == 8 && locate_steps(256) == 9);
	// the LDS: everything fits, sets within 1 .. 32, parts aligned and apart
	for (u32 D : {1u, 2u, 255u, 256u, 1000u, 4095u, 4096u})
		for (u32 kb : {4u, 8u})
			for (u32 ib : {4u, 8u})
				for (int bin = 0; bin < 2; ++bin)
					for (u32 forced : {0u, 1u, 3u, 32u}) {
						const LocateLds l = locate_lds(D, kb, ib, bin != 0, forced);
						CHECK(l.sets >= 1 && l.sets <= LOCATE_MAX_SETS && l.bytes <= LOCATE_LDS_BYTES);
						CHECK(l.cum_off >= D * kb && l.start_off >= l.cum_off + (bin ? (D + 1) * ib : 0));
						CHECK(l.cnt_off >= l.start_off + LOCATE_START_ENTRIES * 4 && l.bytes == l.cnt_off + l.sets * locate_counters(D) * 4);
						CHECK(l.cum_off % 8 == 0 && l.start_off % 8 == 0 && l.cnt_off % 8 == 0);
						if (forced)
							CHECK(l.sets <= forced);
						if (!forced && l.sets < LOCATE_MAX_SETS)
							CHECK(l.bytes + locate_counters(D) * 4 > LOCATE_LDS_BYTES);
					}
	CHECK(locate_lds(4096, 4, 4, true, 0).sets == 3 && locate_lds(4096, 8, 8, true, 0).sets == 2 && locate_lds(1, 4, 4, true, 0).sets == 32);
	// the grid: every whole tile in exactly one share, at most LOCATE_MAX_WGS shares of at least LOCATE_SHARE_TILES tiles
	for (u64 body : {0ull, 1ull, 4095ull, 4096ull, 4097ull, 16383ull, 16384ull, 16385ull, 49157ull, (1ull << 22) + 5, (1ull << 28), (1ull << 28) + 4097,
	                 (1ull << 40) + 3}) {
		const LocateGrid g = locate_grid(body);
		CHECK(g.tiles == body / LOCATE_TILE && g.wgs >= 1 && g.wgs <= LOCATE_MAX_WGS && g.share_tiles >= LOCATE_SHARE_TILES);
		CHECK((u64)g.wgs * g.share_tiles >= g.tiles);
		CHECK(g.tiles == 0 || (u64)(g.wgs - 1) * g.share_tiles < g.tiles);
	}
	CHECK((locate_flush_tiles() + 3) * LOCATE_TILE < (1ull << 32));   // (two tiles per round, and workgroup 0's loose keys)
	if (failures) {
		std::printf("locate_shape_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("locate_shape_check OK\n");
	return 0;
}
