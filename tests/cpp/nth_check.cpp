// nth_check.cpp -- radix_sort_nth (include/radix_sort.hpp) on float and uint64_t keys with uint32_t and uint64_t indices.
// Built by `make cpp`, run by tests/test_gpu_nth.py (needs a GPU).  Prints "nth_check: ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
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

// a stable argsort by `less`, the expected answer
template <typename T, typename Less> static std::vector<size_t> stable_order(const std::vector<T> &a, Less less)
{
	std::vector<size_t> idx(a.size());
	std::iota(idx.begin(), idx.end(), (size_t)0);
	std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return less(a[x], a[y]); });
	return idx;
}

template <typename T, typename IdxType, typename Less>
static void run(const std::vector<T> &src, const std::vector<uint64_t> &ranks, rsx_order order, Less less)
{
	const size_t m = ranks.size();
	const std::vector<T> before = src;
	std::vector<T> out(m + 1, T(77));
	std::vector<IdxType> idx(m + 1, IdxType(0xA5));
	radix_sort_nth<T, IdxType>(src.data(), src.size(), ranks.data(), m, out.data(), idx.data(), order);
	const std::vector<size_t> want = stable_order(src, less);
	for (size_t j = 0; j < m; ++j) {
		CHECK((size_t)idx[j] == want[ranks[j]]);
		CHECK(std::memcmp(&out[j], &src[want[ranks[j]]], sizeof(T)) == 0);
	}
	CHECK(out[m] == T(77) && idx[m] == IdxType(0xA5));                 // nothing past element m - 1
	CHECK(std::memcmp(before.data(), src.data(), src.size() * sizeof(T)) == 0);
	std::vector<T> only(m);                                              // keys alone, in the same order
	radix_sort_nth<T, uint32_t>(src.data(), src.size(), ranks.data(), m, only.data(), nullptr, order);
	CHECK(std::memcmp(only.data(), out.data(), m * sizeof(T)) == 0);
}

int main()
{
	std::vector<float> f;
	std::vector<uint64_t> u;
	uint64_t x = 88172645463325252ull;
	for (int i = 0; i < 300001; ++i) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		f.push_back((float)((int)(x % 2001) - 1000) / 8.0f);             // many ties, both signs
		u.push_back(x & 0xFFFFFF00000000FFull);
	}
	f[5] = INFINITY, f[6] = -INFINITY, f[7] = -0.0f, f[8] = 0.0f;
	// -0.0f orders before +0.0f by the key derivation; otherwise the usual order
	auto fless = [](float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); };
	auto fgreater = [&](float a, float b) { return fless(b, a); };
	const uint64_t n = f.size();
	std::vector<std::vector<uint64_t>> lists = {{n / 2}, {0, n - 1}, {n - 1, n / 4, n / 2, n / 4, 0}, {}, {}};
	for (uint64_t i = 1; i < 10; ++i)
		lists[3].push_back(i * n / 10);                                  // deciles
	for (uint64_t i = 0; i < 100; ++i)
		lists[4].push_back(i * n / 100);                                 // more distinct ranks than a selection carries
	for (const auto &ranks : lists) {
		run<float, uint32_t>(f, ranks, RSX_ASCENDING, fless);
		run<float, uint64_t>(f, ranks, RSX_DESCENDING, fgreater);
		run<uint64_t, uint32_t>(u, ranks, RSX_DESCENDING, [](uint64_t a, uint64_t b) { return a > b; });
		run<uint64_t, uint64_t>(u, ranks, RSX_ASCENDING, [](uint64_t a, uint64_t b) { return a < b; });
	}
	{   // m == 0: nothing written; a rank >= n throws
		uint32_t a[3] = {3, 1, 2}, out = 0xA5;
		radix_sort_nth(a, 3, nullptr, 0, &out);
		CHECK(out == 0xA5);
		const uint64_t bad[1] = {3};
		bool thrown = false;
		try {
			radix_sort_nth(a, 3, bad, 1, &out);
		} catch (const std::exception &) {
			thrown = true;
		}
		CHECK(thrown && out == 0xA5);
	}
	if (failures) {
		std::printf("nth_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("nth_check: ok\n");
	return 0;
}
