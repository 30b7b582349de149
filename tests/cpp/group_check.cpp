// group_check.cpp -- radix_sort_group (include/radix_sort.hpp) against answers derived from std::stable_sort.
// Built by `make cpp`, run by tests/test_gpu_group_cpp.py (needs a GPU).  Prints "group_check: ok" and returns 0.
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
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
			++failures;                                                     \
		}                                                                   \
	} while (0)

template <typename T> static bool same_bits(const T &a, const T &b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// the four arrays from a stable sort of the indices by kf(element): groups are runs of bit-equal elements
template <typename T, typename IdxType, typename KeyFunc> struct Want {
	std::vector<IdxType> inverse, counts, first;
	std::vector<T> keys;
	Want(const std::vector<T> &src, KeyFunc kf) : inverse(src.size())
	{
		std::vector<size_t> perm(src.size());
		std::iota(perm.begin(), perm.end(), (size_t)0);
		std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return kf(src[a]) < kf(src[b]); });
		for (size_t i = 0; i < perm.size(); ++i) {
			if (i == 0 || !same_bits(src[perm[i]], src[perm[i - 1]])) {
				keys.push_back(src[perm[i]]);
				counts.push_back(0);
				first.push_back((IdxType)perm[i]);
			}
			inverse[perm[i]] = (IdxType)(keys.size() - 1);
			++counts.back();
		}
	}
};

template <typename T, typename IdxType, typename KeyFunc> static void run(const std::vector<T> &src, KeyFunc kf, bool all)
{
	const Want<T, IdxType, KeyFunc> want(src, kf);
	const size_t n = src.size();
	const std::vector<T> before = src;
	std::vector<IdxType> inverse(n, (IdxType)0xA5), counts(n, (IdxType)0xA5), first(n, (IdxType)0xA5);
	std::vector<T> keys(n);
	size_t g;
	if (all)
		g = radix_sort_group<T, IdxType>(src.data(), inverse.data(), n, keys.data(), counts.data(), first.data(), kf);
	else
		g = radix_sort_group<T, IdxType>(src.data(), inverse.data(), n, keys.data(), nullptr, nullptr, kf);
	CHECK(g == want.keys.size());
	CHECK(std::memcmp(before.data(), src.data(), n * sizeof(T)) == 0);
	CHECK(inverse == want.inverse);
	for (size_t j = 0; j < g && j < want.keys.size(); ++j) {
		CHECK(same_bits(keys[j], want.keys[j]));
		if (all) {
			CHECK(counts[j] == want.counts[j]);
			CHECK(first[j] == want.first[j]);
		}
	}
}

template <typename T> static std::vector<T> fill(size_t n, uint64_t mask, uint64_t seed)
{
	std::vector<T> v(n);
	uint64_t s = seed;
	for (size_t i = 0; i < n; ++i) {
		uint64_t z = (s += 0x9E3779B97F4A7C15ull);
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		z = (z ^ (z >> 31)) & mask;
		std::memcpy(&v[i], &z, sizeof(T));
	}
	return v;
}

int main()
{
	{   // bitmap_sort_16.c's array, one step further
		const std::vector<uint16_t> src = {255, 45, 45, 45, 1, 2, 3, 255, 0, 65535};
		std::vector<uint32_t> inverse(src.size());
		CHECK(radix_sort_group(src.data(), inverse.data(), src.size()) == 7);
		CHECK((inverse == std::vector<uint32_t>{5, 4, 4, 4, 1, 2, 3, 5, 0, 6}));
	}
	for (int all = 0; all < 2; ++all) {
		run<uint32_t, uint32_t>(fill<uint32_t>(100003, 0x00F0FF0F, 1), basic_kdfs::kdf<uint32_t>, all);    // few varying bits
		run<uint32_t, uint64_t>(fill<uint32_t>(50001, 0xFFFFFFFF, 2), basic_kdfs::kdf<uint32_t>, all);     // all distinct, nearly
		run<uint32_t, uint32_t>(fill<uint32_t>(70001, 0x00FF0000, 3), basic_kdfs::kdf<uint32_t>, all);     // one column
		run<int64_t, uint32_t>(fill<int64_t>(60001, 0x800000000003FFFFull, 4), basic_kdfs::kdf<int64_t>, all);
		run<int64_t, uint64_t>(fill<int64_t>(60001, 0x800000000003FFFFull, 5), rsx_kdf::descending<int64_t>{}, all);
		run<uint32_t, uint32_t>(fill<uint32_t>(100003, 0x00F0FF0F, 6), rsx_kdf::descending<uint32_t>{}, all);
		std::vector<float> f = fill<float>(80001, 0xC0700000, 7);   // a few floats of both signs, both zeros among them
		f[5] = -0.0f;
		f[6] = 0.0f;
		f[7] = INFINITY;
		f[8] = -INFINITY;
		run<float, uint32_t>(f, basic_kdfs::kdf<float>, all);
		run<float, uint32_t>(f, rsx_kdf::descending<float>{}, all);
	}
	{   // n < 2
		uint32_t one = 7, key = 0;
		uint32_t inv = 9, cnt = 9, fst = 9;
		CHECK(radix_sort_group(&one, &inv, 1, &key, &cnt, &fst) == 1 && inv == 0 && key == 7 && cnt == 1 && fst == 0);
		inv = 9;
		CHECK(radix_sort_group(&one, &inv, 0) == 0 && inv == 9);
	}
	{   // a KeyFunc that is not the basic one
		const std::vector<uint32_t> src = {3, 1, 2};
		std::vector<uint32_t> inverse(3);
		bool threw = false;
		try {
			radix_sort_group(src.data(), inverse.data(), src.size(), (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
			                 +[](const uint32_t &x) -> uint32_t { return ~x; });
		} catch (const std::invalid_argument &) {
			threw = true;
		}
		CHECK(threw);
	}
	if (failures) {
		std::printf("group_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("group_check: ok\n");
	return 0;
}
