// lex_check.cpp -- radix_sort_lex (include/radix_sort.hpp): the variadic form on columns of several types and the rsx_lex_col
// form with per-column orders, against std::stable_sort on tuples of derived keys.
// Built by `make cpp`, run by tests/test_gpu_lex.py (needs a GPU).  Prints "lex_check: ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <tuple>
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

// the stable argsort of 0 .. n-1 by tuples of derived keys, the expected answer
template <typename Tuple> static std::vector<size_t> stable_order(const std::vector<Tuple> &keys)
{
	std::vector<size_t> idx(keys.size());
	std::iota(idx.begin(), idx.end(), (size_t)0);
	std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return keys[x] < keys[y]; });
	return idx;
}

template <typename IdxType> static void compare(const std::vector<IdxType> &got, const std::vector<size_t> &want, size_t n)
{
	size_t bad = 0;
	for (size_t j = 0; j < n; ++j)
		bad += (size_t)got[j] != want[j];
	CHECK(bad == 0);
	CHECK(got[n] == IdxType(0xA5));   // nothing past entry n - 1
}

int main()
{
	const size_t n = 70001;
	std::vector<float> f(n);
	std::vector<int32_t> i32(n);
	std::vector<uint8_t> a8(n), b8(n);
	std::vector<uint16_t> c16(n);
	std::vector<uint64_t> u64(n);
	uint64_t x = 88172645463325252ull;
	for (size_t i = 0; i < n; ++i) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		f[i] = (float)((int)(x % 41) - 20) / 4.0f;   // many ties, both signs
		i32[i] = (int32_t)((x >> 16) % 7) - 3;
		a8[i] = (uint8_t)((x >> 24) & 3);
		b8[i] = (uint8_t)((x >> 32) & 0x83);
		c16[i] = (uint16_t)((x >> 40) & 0x8007);
		u64[i] = x & 0xFF000000000000FFull;
	}
	f[5] = -0.0f, f[6] = 0.0f, f[7] = INFINITY, f[8] = -INFINITY;
	const std::vector<float> f_before = f;
	const std::vector<uint64_t> u_before = u64;

	{   // (float, int32): variadic form, uint32_t indices
		std::vector<std::tuple<uint32_t, uint32_t>> keys(n);
		for (size_t i = 0; i < n; ++i)
			keys[i] = {basic_kdfs::kdf(f[i]), basic_kdfs::kdf(i32[i])};
		std::vector<uint32_t> idx(n + 1, 0xA5);
		CHECK(radix_sort_lex<uint32_t>(idx.data(), n, f.data(), i32.data()) == idx.data());
		compare(idx, stable_order(keys), n);
	}
	{   // (u8, u16, u8, u64): variadic form, uint64_t indices
		std::vector<std::tuple<uint8_t, uint16_t, uint8_t, uint64_t>> keys(n);
		for (size_t i = 0; i < n; ++i)
			keys[i] = {a8[i], c16[i], b8[i], u64[i]};
		std::vector<uint64_t> idx(n + 1, 0xA5);
		radix_sort_lex<uint64_t>(idx.data(), n, a8.data(), c16.data(), b8.data(), u64.data());
		compare(idx, stable_order(keys), n);
	}
	{   // one column: radix_sort_rank's order
		std::vector<std::tuple<uint32_t>> keys(n);
		for (size_t i = 0; i < n; ++i)
			keys[i] = {basic_kdfs::kdf(f[i])};
		std::vector<uint32_t> idx(n + 1, 0xA5);
		radix_sort_lex<uint32_t>(idx.data(), n, f.data());
		compare(idx, stable_order(keys), n);
	}
	{   // per-column orders: (float descending, u8 ascending, int32 descending), the same column twice
		const rsx_lex_col cols[4] = {{f.data(), RSX_F32, RSX_DESCENDING},
		                             {a8.data(), RSX_U8, RSX_ASCENDING},
		                             {i32.data(), RSX_I32, RSX_DESCENDING},
		                             {a8.data(), RSX_U8, RSX_DESCENDING}};
		std::vector<std::tuple<uint32_t, uint8_t, uint32_t, uint8_t>> keys(n);
		for (size_t i = 0; i < n; ++i)
			keys[i] = {~basic_kdfs::kdf(f[i]), a8[i], ~basic_kdfs::kdf(i32[i]), (uint8_t)~a8[i]};
		std::vector<uint32_t> idx(n + 1, 0xA5);
		radix_sort_lex<uint32_t>(idx.data(), n, cols, 4);
		compare(idx, stable_order(keys), n);
	}
	CHECK(std::memcmp(f.data(), f_before.data(), n * sizeof(float)) == 0);
	CHECK(std::memcmp(u64.data(), u_before.data(), n * sizeof(uint64_t)) == 0);
	{   // n == 0 writes nothing, n == 1 writes 0; no columns throws
		uint32_t out[2] = {0xA5, 0xA5};
		radix_sort_lex<uint32_t>(out, 0, f.data(), a8.data());
		CHECK(out[0] == 0xA5);
		radix_sort_lex<uint32_t>(out, 1, f.data(), a8.data());
		CHECK(out[0] == 0 && out[1] == 0xA5);
		bool thrown = false;
		try {
			radix_sort_lex<uint32_t>(out, 1, (const rsx_lex_col *)nullptr, 0);
		} catch (const std::exception &) {
			thrown = true;
		}
		CHECK(thrown);
	}
	if (failures) {
		std::printf("lex_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("lex_check: ok\n");
	return 0;
}
