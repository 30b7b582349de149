// segments_check.cpp -- radix_sort_segments (include/radix_sort.hpp) on uint32_t, float, int64_t and uint8_t keys, ascending and
// descending, with uint32_t and uint64_t offsets and indices, global and local, on host arrays (the host-pointer form of
// rsx_sort_segments), against std::stable_sort of every segment's positions.
// Built by `make cpp`, run by tests/test_gpu_segments_cpp.py (needs a GPU).  Prints "segments_check: ok" and returns 0.
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
			if (failures < 20)                                              \
				std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			++failures;                                                     \
		}                                                                   \
	} while (0)

template <typename T, typename IdxType, typename Before>
static void run(const char *name, const std::vector<T> &src, const std::vector<size_t> &cuts, rsx_order order, Before before)
{
	const size_t n = src.size(), m = cuts.size() - 1;
	const std::vector<T> src_was = src;
	std::vector<IdxType> off(cuts.begin(), cuts.end());
	const std::vector<IdxType> off_was = off;
	std::vector<size_t> want(n);
	std::iota(want.begin(), want.end(), (size_t)0);
	for (size_t s = 0; s < m; ++s)
		std::stable_sort(want.begin() + cuts[s], want.begin() + cuts[s + 1], [&](size_t a, size_t c) { return before(src[a], src[c]); });
	for (bool local : {false, true}) {
		std::vector<T> keys(n + 1);
		std::memset(keys.data(), 0xA5, (n + 1) * sizeof(T));
		std::vector<IdxType> idx(n + 1, IdxType(0xA5));
		radix_sort_segments<IdxType>(src.data(), n, off.data(), m, keys.data(), idx.data(), order, local);
		size_t bad = 0;
		for (size_t s = 0; s < m; ++s)
			for (size_t j = cuts[s]; j < cuts[s + 1]; ++j)
				bad += (size_t)idx[j] != want[j] - (local ? cuts[s] : 0) || std::memcmp(&keys[j], &src[want[j]], sizeof(T)) != 0;
		if (bad)
			std::printf("%s: order %d local %d m %zu: %zu wrong\n", name, (int)order, (int)local, m, bad);
		CHECK(bad == 0);
		const unsigned char *past = (const unsigned char *)&keys[n];
		CHECK(past[0] == 0xA5 && idx[n] == IdxType(0xA5));   // nothing past the last entry
		std::vector<T> only(n);
		radix_sort_segments<IdxType>(src.data(), n, off.data(), m, only.data(), (IdxType *)nullptr, order);
		CHECK(std::memcmp(only.data(), keys.data(), n * sizeof(T)) == 0);
	}
	CHECK(std::memcmp(src_was.data(), src.data(), n * sizeof(T)) == 0);
	CHECK(off == off_was);
}

template <typename T, typename Less> static void both_orders(const char *name, const std::vector<T> &src, const std::vector<size_t> &cuts, Less less)
{
	auto greater = [&](const T &a, const T &b) { return less(b, a); };
	run<T, uint32_t>(name, src, cuts, RSX_ASCENDING, less);
	run<T, uint64_t>(name, src, cuts, RSX_DESCENDING, greater);
}

int main()
{
	std::vector<uint32_t> u;
	std::vector<float> f;
	std::vector<int64_t> s;
	std::vector<uint8_t> b;
	uint64_t x = 88172645463325252ull;
	const size_t n = 60007;
	for (size_t i = 0; i < n; ++i) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		u.push_back((uint32_t)(x >> 11));
		f.push_back((float)((int)(x % 2001) - 1000) / 8.0f);             // many ties, both signs
		s.push_back((int64_t)(x % 200001) - 100000);
		b.push_back((uint8_t)(x >> 33));
	}
	f[5] = INFINITY, f[6] = -INFINITY, f[7] = -0.0f, f[8] = 0.0f;
	// segments of every class: empty, one key, a dozen, a few hundred, a few thousand, and one of 20000 keys (longer than the LDS
	// route takes for 8-byte keys with indices)
	std::vector<size_t> cuts = {0};
	const size_t lens[] = {0, 1, 12, 0, 300, 64, 65, 2500, 1, 20000, 257, 2048, 2049, 9000, 0};
	for (size_t l : lens)
		cuts.push_back(cuts.back() + l);
	while (cuts.back() < n) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		cuts.push_back(std::min(n, cuts.back() + (size_t)(x % 40)));
	}
	// -0.0f orders before +0.0f by the key derivation; otherwise the usual order
	auto fless = [](float a, float c) { return a < c || (a == c && std::signbit(a) && !std::signbit(c)); };
	both_orders<uint32_t>("u32", u, cuts, [](uint32_t a, uint32_t c) { return a < c; });
	both_orders<float>("float", f, cuts, fless);
	both_orders<int64_t>("i64", s, cuts, [](int64_t a, int64_t c) { return a < c; });
	both_orders<uint8_t>("u8", b, cuts, [](uint8_t a, uint8_t c) { return a < c; });
	{   // uniform rows without offsets; nothing to do; what is refused
		uint32_t a[6] = {3, 1, 2, 9, 8, 7}, keys[6] = {0}, idx[6] = {0};
		radix_sort_segments<uint32_t>(a, 6, (const uint32_t *)nullptr, 2, keys, idx, RSX_ASCENDING, true);
		CHECK(keys[0] == 1 && keys[1] == 2 && keys[2] == 3 && keys[3] == 7 && keys[4] == 8 && keys[5] == 9);
		CHECK(idx[0] == 1 && idx[1] == 2 && idx[2] == 0 && idx[3] == 2 && idx[4] == 1 && idx[5] == 0);
		keys[0] = 0xA5;
		radix_sort_segments<uint32_t>(a, 0, (const uint32_t *)nullptr, 2, keys, idx);
		radix_sort_segments<uint32_t>(a, 6, (const uint32_t *)nullptr, 0, keys, idx);
		CHECK(keys[0] == 0xA5);
		const uint32_t bad_off[3] = {0, 4, 5};
		for (int which = 0; which < 4; ++which) {
			bool thrown = false;
			try {
				if (which == 0)
					radix_sort_segments<uint32_t>(a, 6, (const uint32_t *)nullptr, 2, (uint32_t *)nullptr);   // both outputs null
				else if (which == 1)
					radix_sort_segments<uint32_t>(a, 6, (const uint32_t *)nullptr, 2, a);                    // out_keys == src
				else if (which == 2)
					radix_sort_segments<uint32_t>(a, 6, (const uint32_t *)nullptr, 4, keys);                 // 6 keys in 4 rows
				else
					radix_sort_segments<uint32_t>(a, 6, bad_off, 2, keys);                                   // offsets[m] != n
			} catch (const std::exception &) {
				thrown = true;
			}
			CHECK(thrown);
		}
		CHECK(keys[0] == 0xA5);
	}
	if (failures) {
		std::printf("segments_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("segments_check: ok\n");
	return 0;
}
