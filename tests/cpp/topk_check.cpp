// topk_check.cpp -- radix_sort_topk (include/radix_sort.hpp) on float and uint64_t keys with uint32_t and uint64_t indices.
// Built by `make cpp`, run by tests/test_gpu_topk.py (needs a GPU).  Prints "topk_check: ok" and returns 0.
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

// the first k of a stable argsort by `less`, the expected answer
template <typename T, typename Less> static std::vector<size_t> stable_first(const std::vector<T> &a, size_t k, Less less)
{
	std::vector<size_t> idx(a.size());
	std::iota(idx.begin(), idx.end(), (size_t)0);
	std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return less(a[x], a[y]); });
	idx.resize(k);
	return idx;
}

template <typename T, typename IdxType, typename Less> static void run(const std::vector<T> &src, size_t k, rsx_order order, Less less)
{
	const std::vector<T> before = src;
	std::vector<T> out(k + 1, T(77));
	std::vector<IdxType> idx(k + 1, IdxType(0xA5));
	CHECK((radix_sort_topk<T, IdxType>(src.data(), src.size(), k, out.data(), idx.data(), order)) == k);
	const std::vector<size_t> want = stable_first(src, k, less);
	for (size_t j = 0; j < k; ++j) {
		CHECK((size_t)idx[j] == want[j]);
		CHECK(std::memcmp(&out[j], &src[want[j]], sizeof(T)) == 0);
	}
	CHECK(out[k] == T(77) && idx[k] == IdxType(0xA5));               // nothing past element k - 1
	CHECK(std::memcmp(before.data(), src.data(), src.size() * sizeof(T)) == 0);
	std::vector<T> only(k);                                              // keys alone, in the same order
	CHECK((radix_sort_topk<T, uint32_t>(src.data(), src.size(), k, only.data(), nullptr, order)) == k);
	CHECK(std::memcmp(only.data(), out.data(), k * sizeof(T)) == 0);
}

int main()
{
	std::vector<float> f;
	std::vector<uint64_t> u;
	uint64_t x = 88172645463325252ull;
	for (int i = 0; i < 70001; ++i) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		f.push_back((float)((int)(x % 2001) - 1000) / 8.0f);             // many ties, both signs
		u.push_back(x & 0xFFFFFF00000000FFull);
	}
	f[5] = INFINITY, f[6] = -INFINITY, f[7] = -0.0f, f[8] = 0.0f;
	// -0.0f orders before +0.0f by the key derivation; otherwise the usual order
	auto fless = [](float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); };
	auto fgreater = [&](float a, float b) { return fless(b, a); };
	for (size_t k : {(size_t)1, (size_t)10, (size_t)1000, (size_t)35000, f.size()}) {
		run<float, uint32_t>(f, k, RSX_ASCENDING, fless);
		run<float, uint64_t>(f, k, RSX_DESCENDING, fgreater);
		run<uint64_t, uint32_t>(u, k, RSX_DESCENDING, [](uint64_t a, uint64_t b) { return a > b; });
		run<uint64_t, uint64_t>(u, k, RSX_ASCENDING, [](uint64_t a, uint64_t b) { return a < b; });
	}
	{   // k == 0: nothing written; k > n throws
		uint32_t a[3] = {3, 1, 2}, out = 0xA5;
		CHECK((radix_sort_topk(a, 3, 0, &out)) == 0 && out == 0xA5);
		bool thrown = false;
		try {
			radix_sort_topk(a, 3, 4, &out);
		} catch (const std::exception &) {
			thrown = true;
		}
		CHECK(thrown);
	}
	if (failures) {
		std::printf("topk_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("topk_check: ok\n");
	return 0;
}
