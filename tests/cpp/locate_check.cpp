// locate_check.cpp -- radix_sort_locate (include/radix_sort.hpp) on uint32_t, float, int64_t and uint8_t keys, ascending and
// descending, with uint32_t and uint64_t indices, on host arrays (the host-pointer form of rsx_sort_locate).
// Built by `make cpp`, run by tests/test_gpu_locate_cpp.py (needs a GPU).  Prints "locate_check: ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "radix_sort.hpp"

static int failures = 0;
#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			if (failures < 20)                                              \
				std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			++failures;                                                     \
		}                                                                   \
	} while (0)

// less / equal from std::lower_bound / std::upper_bound over a std::stable_sort by `before`, the bins the same way round
template <typename T, typename IdxType, typename Before>
static void run(const char *name, const std::vector<T> &src, const std::vector<T> &vals, rsx_order order, Before before)
{
	const size_t n = src.size(), m = vals.size();
	const std::vector<T> src_was = src, vals_was = vals;
	std::vector<T> sorted = src, svals = vals;
	std::stable_sort(sorted.begin(), sorted.end(), before);
	std::stable_sort(svals.begin(), svals.end(), before);
	for (uint32_t flags : {0u, (uint32_t)RSX_LOCATE_BINS_BELOW}) {
		std::vector<IdxType> less(m + 1, IdxType(0xA5)), equal(m + 1, IdxType(0xA5)), bin(n + 1, IdxType(0xA5));
		radix_sort_locate<IdxType>(src.data(), n, vals.data(), m, less.data(), equal.data(), bin.data(), order, flags);
		size_t bad = 0;
		for (size_t j = 0; j < m; ++j) {
			const size_t lo = (size_t)(std::lower_bound(sorted.begin(), sorted.end(), vals[j], before) - sorted.begin());
			const size_t hi = (size_t)(std::upper_bound(sorted.begin(), sorted.end(), vals[j], before) - sorted.begin());
			bad += (size_t)less[j] != lo || (size_t)equal[j] != hi - lo;
		}
		for (size_t i = 0; i < n; ++i) {
			const size_t want = flags ? (size_t)(std::lower_bound(svals.begin(), svals.end(), src[i], before) - svals.begin())
			                          : (size_t)(std::upper_bound(svals.begin(), svals.end(), src[i], before) - svals.begin());
			bad += (size_t)bin[i] != want;
		}
		if (bad)
			std::printf("%s: order %d flags %u: %zu wrong\n", name, (int)order, flags, bad);
		CHECK(bad == 0);
		CHECK(less[m] == IdxType(0xA5) && equal[m] == IdxType(0xA5) && bin[n] == IdxType(0xA5));   // nothing past the last entry
		// less alone: the defaults of the other two
		std::vector<IdxType> only(m + 1, IdxType(0xA5));
		radix_sort_locate<IdxType>(src.data(), n, vals.data(), m, only.data());
		if (order == RSX_ASCENDING)
			CHECK(std::memcmp(only.data(), less.data(), (m + 1) * sizeof(IdxType)) == 0);
	}
	CHECK(std::memcmp(src_was.data(), src.data(), n * sizeof(T)) == 0);
	CHECK(std::memcmp(vals_was.data(), vals.data(), m * sizeof(T)) == 0);
}

template <typename T, typename Less> static void both_orders(const char *name, const std::vector<T> &src, const std::vector<T> &vals, Less less)
{
	auto greater = [&](const T &a, const T &b) { return less(b, a); };
	run<T, uint32_t>(name, src, vals, RSX_ASCENDING, less);
	run<T, uint64_t>(name, src, vals, RSX_DESCENDING, greater);
	run<T, uint64_t>(name, src, vals, RSX_ASCENDING, less);
	run<T, uint32_t>(name, src, vals, RSX_DESCENDING, greater);
}

int main()
{
	std::vector<uint32_t> u;
	std::vector<float> f;
	std::vector<int64_t> s;
	std::vector<uint8_t> b;
	uint64_t x = 88172645463325252ull;
	for (int i = 0; i < 100003; ++i) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		u.push_back((uint32_t)(x >> 11));
		f.push_back((float)((int)(x % 2001) - 1000) / 8.0f);             // many ties, both signs
		s.push_back((int64_t)(x % 200001) - 100000);
		b.push_back((uint8_t)(x >> 33));
	}
	f[5] = INFINITY, f[6] = -INFINITY, f[7] = -0.0f, f[8] = 0.0f;
	// values: some of the keys, some between them; few (the search), many distinct (the sort), for bytes the table
	auto pick = [&](auto &src, size_t m, auto between) {
		typename std::remove_reference<decltype(src)>::type v;
		for (size_t j = 0; j < m; ++j) {
			x ^= x << 13, x ^= x >> 7, x ^= x << 17;
			v.push_back((j & 1) ? src[x % src.size()] : between(x));
		}
		return v;
	};
	// -0.0f orders before +0.0f by the key derivation; otherwise the usual order
	auto fless = [](float a, float c) { return a < c || (a == c && std::signbit(a) && !std::signbit(c)); };
	for (size_t m : {(size_t)1, (size_t)255, (size_t)6000}) {
		both_orders<uint32_t>("u32", u, pick(u, m, [](uint64_t r) { return (uint32_t)r; }), [](uint32_t a, uint32_t c) { return a < c; });
		auto fv = pick(f, m, [](uint64_t r) { return (float)((int)(r % 4003) - 2001) / 16.0f; });
		if (m > 4) {
			fv[0] = -0.0f, fv[1] = 0.0f, fv[2] = INFINITY, fv[3] = -INFINITY;
		}
		both_orders<float>("float", f, fv, fless);
		both_orders<int64_t>("i64", s, pick(s, m, [](uint64_t r) { return (int64_t)(r % 300001) - 150000; }), [](int64_t a, int64_t c) { return a < c; });
		both_orders<uint8_t>("u8", b, pick(b, m, [](uint64_t r) { return (uint8_t)r; }), [](uint8_t a, uint8_t c) { return a < c; });
	}
	{   // no values: nothing written; no keys: zeros; all outputs null throws
		uint32_t a[3] = {3, 1, 2}, v[2] = {2, 9}, less[2] = {0xA5, 0xA5}, equal[2] = {0xA5, 0xA5};
		radix_sort_locate<uint32_t>(a, 3, v, 0, less, equal);
		CHECK(less[0] == 0xA5 && equal[0] == 0xA5);
		radix_sort_locate<uint32_t>(a, 0, v, 2, less, equal);
		CHECK(less[0] == 0 && less[1] == 0 && equal[0] == 0 && equal[1] == 0);
		bool thrown = false;
		try {
			radix_sort_locate<uint32_t>(a, 3, v, 2, (uint32_t *)nullptr);
		} catch (const std::exception &) {
			thrown = true;
		}
		CHECK(thrown);
	}
	if (failures) {
		std::printf("locate_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("locate_check: ok\n");
	return 0;
}
