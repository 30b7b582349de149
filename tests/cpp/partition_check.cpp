// partition_check.cpp -- radix_sort_partition (include/radix_sort.hpp) on uint32_t, float, int64_t and uint8_t keys, ascending and
// descending, with uint32_t and uint64_t indices, on host arrays (the host-pointer form of rsx_sort_partition).
// Built by `make cpp`, run by tests/test_gpu_partition_cpp.py (needs a GPU).  Prints "partition_check: ok" and returns 0.
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

// the bins from std::upper_bound / std::lower_bound over the sorted edges, the order from std::stable_sort of the positions by bin
template <typename T, typename IdxType, typename Before>
static void run(const char *name, const std::vector<T> &src, const std::vector<T> &edges, rsx_order order, Before before)
{
	const size_t n = src.size(), m = edges.size();
	const std::vector<T> src_was = src, edges_was = edges;
	std::vector<T> sedges = edges;
	std::stable_sort(sedges.begin(), sedges.end(), before);
	for (uint32_t flags : {0u, (uint32_t)RSX_PARTITION_BELOW}) {
		std::vector<size_t> bin(n), want_idx(n), want_off(m + 2, 0);
		for (size_t i = 0; i < n; ++i) {
			bin[i] = flags ? (size_t)(std::lower_bound(sedges.begin(), sedges.end(), src[i], before) - sedges.begin())
			               : (size_t)(std::upper_bound(sedges.begin(), sedges.end(), src[i], before) - sedges.begin());
			want_off[bin[i] + 1] += 1;
		}
		for (size_t j = 1; j < m + 2; ++j)   // offsets[j] = the elements with a bin below j
			want_off[j] += want_off[j - 1];
		std::iota(want_idx.begin(), want_idx.end(), (size_t)0);
		std::stable_sort(want_idx.begin(), want_idx.end(), [&](size_t a, size_t c) { return bin[a] < bin[c]; });
		std::vector<T> keys(n + 1);
		std::memset(keys.data(), 0xA5, (n + 1) * sizeof(T));
		std::vector<IdxType> idx(n + 1, IdxType(0xA5)), off(m + 3, IdxType(0xA5));
		radix_sort_partition<IdxType>(src.data(), n, edges.data(), m, keys.data(), idx.data(), off.data(), order, flags);
		size_t bad = 0;
		for (size_t i = 0; i < n; ++i)
			bad += (size_t)idx[i] != want_idx[i] || std::memcmp(&keys[i], &src[want_idx[i]], sizeof(T)) != 0;
		for (size_t j = 0; j < m + 2; ++j)
			bad += (size_t)off[j] != want_off[j];
		if (bad)
			std::printf("%s: order %d flags %u m %zu: %zu wrong\n", name, (int)order, flags, m, bad);
		CHECK(bad == 0);
		const unsigned char *past = (const unsigned char *)&keys[n];
		CHECK(past[0] == 0xA5 && idx[n] == IdxType(0xA5) && off[m + 2] == IdxType(0xA5));   // nothing past the last entry
		// keys alone: the defaults of the other two
		std::vector<T> only(n);
		radix_sort_partition<IdxType>(src.data(), n, edges.data(), m, only.data());
		if (order == RSX_ASCENDING && !flags)
			CHECK(std::memcmp(only.data(), keys.data(), n * sizeof(T)) == 0);
	}
	CHECK(std::memcmp(src_was.data(), src.data(), n * sizeof(T)) == 0);
	CHECK(std::memcmp(edges_was.data(), edges.data(), m * sizeof(T)) == 0);
}

template <typename T, typename Less> static void both_orders(const char *name, const std::vector<T> &src, const std::vector<T> &edges, Less less)
{
	auto greater = [&](const T &a, const T &b) { return less(b, a); };
	run<T, uint32_t>(name, src, edges, RSX_ASCENDING, less);
	run<T, uint64_t>(name, src, edges, RSX_DESCENDING, greater);
}

int main()
{
	std::vector<uint32_t> u;
	std::vector<float> f;
	std::vector<int64_t> s;
	std::vector<uint8_t> b;
	uint64_t x = 88172645463325252ull;
	for (int i = 0; i < 50003; ++i) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		u.push_back((uint32_t)(x >> 11));
		f.push_back((float)((int)(x % 2001) - 1000) / 8.0f);             // many ties, both signs
		s.push_back((int64_t)(x % 200001) - 100000);
		b.push_back((uint8_t)(x >> 33));
	}
	f[5] = INFINITY, f[6] = -INFINITY, f[7] = -0.0f, f[8] = 0.0f;
	// edges: some of the keys, some between them; one (std::stable_partition), few (the scatter), many distinct (the sort)
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
	for (size_t m : {(size_t)1, (size_t)3, (size_t)200, (size_t)700}) {
		both_orders<uint32_t>("u32", u, pick(u, m, [](uint64_t r) { return (uint32_t)r; }), [](uint32_t a, uint32_t c) { return a < c; });
		auto fv = pick(f, m, [](uint64_t r) { return (float)((int)(r % 4003) - 2001) / 16.0f; });
		if (m > 4) {
			fv[0] = -0.0f, fv[1] = 0.0f, fv[2] = INFINITY, fv[3] = -INFINITY;
		}
		both_orders<float>("float", f, fv, fless);
		both_orders<int64_t>("i64", s, pick(s, m, [](uint64_t r) { return (int64_t)(r % 300001) - 150000; }), [](int64_t a, int64_t c) { return a < c; });
		both_orders<uint8_t>("u8", b, pick(b, m, [](uint64_t r) { return (uint8_t)r; }), [](uint8_t a, uint8_t c) { return a < c; });
	}
	{   // no edges: one part; no keys: zero offsets; both outputs null and out_keys == src throw
		uint32_t a[3] = {3, 1, 2}, v[2] = {2, 9}, keys[3] = {0xA5, 0xA5, 0xA5}, idx[3] = {0xA5, 0xA5, 0xA5}, off[4] = {0xA5, 0xA5, 0xA5, 0xA5};
		radix_sort_partition<uint32_t>(a, 3, v, 0, keys, idx, off);
		CHECK(keys[0] == 3 && keys[1] == 1 && keys[2] == 2 && idx[0] == 0 && idx[1] == 1 && idx[2] == 2 && off[0] == 0 && off[1] == 3 && off[2] == 0xA5);
		radix_sort_partition<uint32_t>(a, 0, v, 2, keys, idx, off);
		CHECK(off[0] == 0 && off[1] == 0 && off[2] == 0 && off[3] == 0 && keys[0] == 3 && idx[0] == 0);
		for (int which = 0; which < 2; ++which) {
			bool thrown = false;
			try {
				radix_sort_partition<uint32_t>(a, 3, v, 2, which ? a : (uint32_t *)nullptr);
			} catch (const std::exception &) {
				thrown = true;
			}
			CHECK(thrown);
		}
	}
	if (failures) {
		std::printf("partition_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("partition_check: ok\n");
	return 0;
}
