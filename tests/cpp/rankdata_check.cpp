// rankdata_check.cpp -- radix_sort_rankdata (include/radix_sort.hpp) against answers derived from std::stable_sort.
// Built by `make cpp`, run by tests/test_gpu_rankdata_cpp.py (needs a GPU).  Prints "rankdata_check: ok" and returns 0.
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

// the three arrays from a stable sort of the indices by kf(element): runs of bit-equal elements share less and equal
template <typename T, typename IdxType, typename KeyFunc> struct Want {
	std::vector<IdxType> place, less, equal;
	Want(const std::vector<T> &src, KeyFunc kf) : place(src.size()), less(src.size()), equal(src.size())
	{
		std::vector<size_t> perm(src.size());
		std::iota(perm.begin(), perm.end(), (size_t)0);
		std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return kf(src[a]) < kf(src[b]); });
		for (size_t s = 0; s < perm.size();) {
			size_t e = s + 1;
			while (e < perm.size() && same_bits(src[perm[e]], src[perm[s]]))
				++e;
			for (size_t j = s; j < e; ++j) {
				place[perm[j]] = (IdxType)j;
				less[perm[j]] = (IdxType)s;
				equal[perm[j]] = (IdxType)(e - s);
			}
			s = e;
		}
	}
};

// what: bit 0 place, bit 1 less, bit 2 equal
template <typename T, typename IdxType, typename KeyFunc> static void run(const std::vector<T> &src, KeyFunc kf, int what)
{
	const Want<T, IdxType, KeyFunc> want(src, kf);
	const size_t n = src.size();
	const std::vector<T> before = src;
	const IdxType fill = (IdxType)0xA5A5A5A5u;
	std::vector<IdxType> place(n, fill), less(n, fill), equal(n, fill);
	radix_sort_rankdata<T, IdxType>(src.data(), n, what & 1 ? place.data() : nullptr, what & 2 ? less.data() : nullptr,
	                                what & 4 ? equal.data() : nullptr, kf);
	CHECK(std::memcmp(before.data(), src.data(), n * sizeof(T)) == 0);
	CHECK(place == (what & 1 ? want.place : std::vector<IdxType>(n, fill)));
	CHECK(less == (what & 2 ? want.less : std::vector<IdxType>(n, fill)));
	CHECK(equal == (what & 4 ? want.equal : std::vector<IdxType>(n, fill)));
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
	{   // a small array by hand
		const std::vector<uint16_t> src = {255, 45, 45, 45, 1, 2, 3, 255, 0, 65535};
		std::vector<uint32_t> place(src.size()), less(src.size()), equal(src.size());
		radix_sort_rankdata(src.data(), src.size(), place.data(), less.data(), equal.data());
		CHECK((place == std::vector<uint32_t>{7, 4, 5, 6, 1, 2, 3, 8, 0, 9}));
		CHECK((less == std::vector<uint32_t>{7, 4, 4, 4, 1, 2, 3, 7, 0, 9}));
		CHECK((equal == std::vector<uint32_t>{2, 3, 3, 3, 1, 1, 1, 2, 1, 1}));
	}
	for (int what : {1, 6, 7}) {
		run<uint32_t, uint32_t>(fill<uint32_t>(100003, 0x00F0FF0F, 1), basic_kdfs::kdf<uint32_t>, what);   // few varying bits
		run<uint32_t, uint64_t>(fill<uint32_t>(50001, 0xFFFFFFFF, 2), basic_kdfs::kdf<uint32_t>, what);    // all distinct, nearly
		run<uint32_t, uint32_t>(fill<uint32_t>(70001, 0x00FF0000, 3), basic_kdfs::kdf<uint32_t>, what);    // one column
		run<uint32_t, uint64_t>(fill<uint32_t>(70001, 0x00FF0000, 3), rsx_kdf::descending<uint32_t>{}, what);
		run<int64_t, uint32_t>(fill<int64_t>(60001, 0x800000000003FFFFull, 4), basic_kdfs::kdf<int64_t>, what);
		run<int64_t, uint64_t>(fill<int64_t>(60001, 0x800000000003FFFFull, 5), rsx_kdf::descending<int64_t>{}, what);
		run<uint32_t, uint32_t>(fill<uint32_t>(100003, 0x00F0FF0F, 6), rsx_kdf::descending<uint32_t>{}, what);
		std::vector<float> f = fill<float>(80001, 0xC0700000, 7);   // a few floats of both signs, both zeros among them
		f[5] = -0.0f;
		f[6] = 0.0f;
		f[7] = INFINITY;
		f[8] = -INFINITY;
		run<float, uint32_t>(f, basic_kdfs::kdf<float>, what);
		run<float, uint32_t>(f, rsx_kdf::descending<float>{}, what);
	}
	{   // n < 2
		uint32_t one = 7;
		uint32_t place = 9, less = 9, equal = 9;
		radix_sort_rankdata(&one, 1, &place, &less, &equal);
		CHECK(place == 0 && less == 0 && equal == 1);
		place = 9;
		radix_sort_rankdata(&one, 0, &place);
		CHECK(place == 9);
	}
	{   // no output at all
		const std::vector<uint32_t> src = {3, 1, 2};
		bool threw = false;
		try {
			radix_sort_rankdata(src.data(), src.size(), (uint32_t *)nullptr);
		} catch (const std::exception &) {
			threw = true;
		}
		CHECK(threw);
	}
	{   // a KeyFunc that is not the basic one
		const std::vector<uint32_t> src = {3, 1, 2};
		std::vector<uint32_t> place(3);
		bool threw = false;
		try {
			radix_sort_rankdata(src.data(), src.size(), place.data(), (uint32_t *)nullptr, (uint32_t *)nullptr,
			                    +[](const uint32_t &x) -> uint32_t { return ~x; });
		} catch (const std::invalid_argument &) {
			threw = true;
		}
		CHECK(threw);
	}
	if (failures) {
		std::printf("rankdata_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("rankdata_check: ok\n");
	return 0;
}
