// reduce_check.cpp -- radix_sort_reduce (include/radix_sort.hpp) against answers derived from std::stable_sort.
// Built by `make cpp`, run by tests/test_gpu_reduce_cpp.py (needs a GPU).  Prints "reduce_check: ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <stdexcept>
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

template <typename T> static bool same_bits(const T &a, const T &b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// groups are runs of bit-equal keys in a stable sort of the indices by kf(key); values: small integers, so that every sum is
// exact whatever its order (floats included); min and max by the value's own derived key
template <typename T, typename V, typename IdxType, typename KeyFunc> static void run(const std::vector<T> &keys, const std::vector<V> &vals, KeyFunc kf)
{
	typedef rsx_detail::reduce_sum_t<V> S;
	const size_t n = keys.size();
	std::vector<size_t> perm(n);
	std::iota(perm.begin(), perm.end(), (size_t)0);
	std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return kf(keys[a]) < kf(keys[b]); });
	std::vector<T> wkeys;
	std::vector<IdxType> wcounts;
	std::vector<S> wsum;
	std::vector<V> wmin, wmax;
	for (size_t i = 0; i < n; ++i) {
		const V v = vals[perm[i]];
		if (i == 0 || !same_bits(keys[perm[i]], keys[perm[i - 1]])) {
			wkeys.push_back(keys[perm[i]]);
			wcounts.push_back(0);
			wsum.push_back((S)0);
			wmin.push_back(v);
			wmax.push_back(v);
		}
		++wcounts.back();
		wsum.back() = (S)(wsum.back() + (S)v);
		if (basic_kdfs::kdf<V>(v) < basic_kdfs::kdf<V>(wmin.back()))
			wmin.back() = v;
		if (basic_kdfs::kdf<V>(v) > basic_kdfs::kdf<V>(wmax.back()))
			wmax.back() = v;
	}
	const std::vector<T> kbefore = keys;
	const std::vector<V> vbefore = vals;
	std::vector<T> okeys(n);
	std::vector<IdxType> counts(n, (IdxType)0xA5);
	std::vector<S> sum(n);
	std::vector<V> mn(n), mx(n);
	const size_t g = radix_sort_reduce<T, V, IdxType>(keys.data(), vals.data(), n, okeys.data(), counts.data(), sum.data(), mn.data(), mx.data(), kf);
	CHECK(g == wkeys.size());
	CHECK(std::memcmp(kbefore.data(), keys.data(), n * sizeof(T)) == 0 && std::memcmp(vbefore.data(), vals.data(), n * sizeof(V)) == 0);
	for (size_t j = 0; j < g && j < wkeys.size(); ++j) {
		CHECK(same_bits(okeys[j], wkeys[j]));
		CHECK(counts[j] == wcounts[j]);
		CHECK(same_bits(sum[j], wsum[j]));
		CHECK(same_bits(mn[j], wmin[j]));
		CHECK(same_bits(mx[j], wmax[j]));
	}
	// sums alone
	std::vector<S> sum2(n);
	CHECK((radix_sort_reduce<T, V, IdxType>(keys.data(), vals.data(), n, nullptr, nullptr, sum2.data(), nullptr, nullptr, kf)) == g);
	for (size_t j = 0; j < g && j < wkeys.size(); ++j)
		CHECK(same_bits(sum2[j], wsum[j]));
}

static uint64_t mix(uint64_t &s)
{
	uint64_t z = (s += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

template <typename T> static std::vector<T> fill(size_t n, uint64_t mask, uint64_t seed)
{
	std::vector<T> v(n);
	uint64_t s = seed;
	for (size_t i = 0; i < n; ++i) {
		const uint64_t z = mix(s) & mask;
		std::memcpy(&v[i], &z, sizeof(T));
	}
	return v;
}

// integers of magnitude below 2^20, both signs where V has one
template <typename V> static std::vector<V> values(size_t n, uint64_t seed)
{
	std::vector<V> v(n);
	uint64_t s = seed;
	for (size_t i = 0; i < n; ++i) {
		const int64_t x = (int64_t)(mix(s) & 0xFFFFF) - (std::is_signed<V>::value ? 0x80000 : 0);
		v[i] = (V)x;
	}
	return v;
}

int main()
{
	{   // a handful by hand
		const std::vector<uint16_t> keys = {255, 45, 45, 45, 1, 2, 3, 255, 0, 65535};
		const std::vector<int32_t> vals = {1, -2, 3, -4, 5, 6, 7, 8, 9, 10};
		std::vector<uint16_t> ok(keys.size());
		std::vector<uint32_t> cnt(keys.size());
		std::vector<int64_t> sum(keys.size());
		std::vector<int32_t> mn(keys.size()), mx(keys.size());
		CHECK(radix_sort_reduce(keys.data(), vals.data(), keys.size(), ok.data(), cnt.data(), sum.data(), mn.data(), mx.data()) == 7);
		CHECK(ok[4] == 45 && cnt[4] == 3 && sum[4] == -3 && mn[4] == -4 && mx[4] == 3);
		CHECK(ok[5] == 255 && cnt[5] == 2 && sum[5] == 9 && mn[5] == 1 && mx[5] == 8);
	}
	run<uint32_t, uint32_t, uint32_t>(fill<uint32_t>(100003, 0x00F0F00F, 1), values<uint32_t>(100003, 11), basic_kdfs::kdf<uint32_t>);   // cells in LDS
	run<uint32_t, float, uint64_t>(fill<uint32_t>(100003, 0x00F0F00F, 2), values<float>(100003, 12), rsx_kdf::descending<uint32_t>{});
	run<uint8_t, double, uint32_t>(fill<uint8_t>(70001, 0xFF, 3), values<double>(70001, 13), basic_kdfs::kdf<uint8_t>);
	run<uint32_t, int64_t, uint32_t>(fill<uint32_t>(50001, 0xFFFFFFFF, 4), values<int64_t>(50001, 14), basic_kdfs::kdf<uint32_t>);        // the sort route
	run<int64_t, int32_t, uint32_t>(fill<int64_t>(60001, 0x80000000FFFFFFFFull, 5), values<int32_t>(60001, 15), basic_kdfs::kdf<int64_t>);
	run<uint32_t, uint64_t, uint32_t>(fill<uint32_t>(90001, 0x000FFFFF, 6), values<uint64_t>(90001, 16), basic_kdfs::kdf<uint32_t>);
	{
		std::vector<float> f = fill<float>(80001, 0xC0700000, 7);   // a few floats of both signs, both zeros among them
		f[5] = -0.0f;
		f[6] = 0.0f;
		f[7] = INFINITY;
		f[8] = -INFINITY;
		run<float, float, uint32_t>(f, values<float>(80001, 17), basic_kdfs::kdf<float>);
		run<float, int32_t, uint32_t>(f, values<int32_t>(80001, 18), rsx_kdf::descending<float>{});
	}
	{   // n < 2
		uint32_t key = 7, okey = 0, cnt = 9;
		float val = -2.5f, mn = 0, mx = 0;
		double sum = 0;
		CHECK(radix_sort_reduce(&key, &val, 1, &okey, &cnt, &sum, &mn, &mx) == 1 && okey == 7 && cnt == 1 && sum == -2.5 && mn == -2.5f && mx == -2.5f);
		cnt = 9;
		CHECK(radix_sort_reduce(&key, &val, 0, &okey, &cnt) == 0 && cnt == 9);
	}
	{   // a KeyFunc that is not the basic one
		const std::vector<uint32_t> keys = {3, 1, 2}, vals = {1, 2, 3};
		std::vector<uint64_t> sum(3);
		bool threw = false;
		try {
			radix_sort_reduce(keys.data(), vals.data(), keys.size(), (uint32_t *)nullptr, (uint32_t *)nullptr, sum.data(), (uint32_t *)nullptr,
			                  (uint32_t *)nullptr, +[](const uint32_t &x) -> uint32_t { return ~x; });
		} catch (const std::invalid_argument &) {
			threw = true;
		}
		CHECK(threw);
	}
	if (failures) {
		std::printf("reduce_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("reduce_check: ok\n");
	return 0;
}
