// join_check.cpp -- radix_sort_join and radix_sort_join_pairs (include/radix_sort.hpp) on uint32_t, float, int64_t and uint8_t keys,
// ascending and descending, inner and left, with uint32_t and uint64_t indices, on host arrays (the host-pointer forms of
// rsx_sort_join and rsx_join_pairs), against a restatement by std::stable_sort of the right row numbers and std::equal_range.
// Built by `make cpp`, run by tests/test_gpu_join_cpp.py (needs a GPU).  Prints "join_check: ok" and returns 0.
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
static void run(const char *name, const std::vector<T> &left, const std::vector<T> &right, rsx_order order, Before before)
{
	const size_t n = left.size(), m = right.size();
	const std::vector<T> left_was = left, right_was = right;
	// the stable order of the right rows, and the right keys in that order
	std::vector<size_t> perm(m);
	std::iota(perm.begin(), perm.end(), (size_t)0);
	std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return before(right[a], right[b]); });
	std::vector<T> sorted(m);
	for (size_t j = 0; j < m; ++j)
		sorted[j] = right[perm[j]];
	for (uint32_t flags : {0u, (uint32_t)RSX_JOIN_LEFT}) {
		std::vector<IdxType> want_l, want_r;
		std::vector<size_t> lo(n), cnt(n);
		for (size_t i = 0; i < n; ++i) {
			const auto range = std::equal_range(sorted.begin(), sorted.end(), left[i], before);
			lo[i] = (size_t)(range.first - sorted.begin());
			cnt[i] = (size_t)(range.second - range.first);
			for (size_t t = 0; t < cnt[i]; ++t) {
				want_l.push_back((IdxType)i);
				want_r.push_back((IdxType)perm[lo[i] + t]);
			}
			if (!cnt[i] && flags) {
				want_l.push_back((IdxType)i);
				want_r.push_back((IdxType)~(IdxType)0);
			}
		}
		std::vector<IdxType> start(n + 1, IdxType(0xA5)), count(n + 1, IdxType(0xA5)), rp(m + 1, IdxType(0xA5));
		const uint64_t pairs = radix_sort_join<IdxType>(left.data(), n, right.data(), m, start.data(), count.data(), rp.data(), order, flags);
		size_t bad = 0;
		for (size_t i = 0; i < n; ++i)
			bad += (size_t)count[i] != cnt[i] || (cnt[i] && (size_t)start[i] != lo[i]);
		for (size_t j = 0; j < m; ++j)
			bad += (size_t)rp[j] != perm[j];
		if (bad)
			std::printf("%s: order %d flags %u: %zu ranges wrong\n", name, (int)order, flags, bad);
		CHECK(bad == 0);
		CHECK(pairs == want_l.size());
		CHECK(start[n] == IdxType(0xA5) && count[n] == IdxType(0xA5) && rp[m] == IdxType(0xA5));   // nothing past the last entry
		// the number of pairs alone
		CHECK(radix_sort_join<IdxType>(left.data(), n, right.data(), m, (IdxType *)nullptr, (IdxType *)nullptr, (IdxType *)nullptr, order, flags) == pairs);
		std::vector<IdxType> out_l(pairs + 1, IdxType(0xA5)), out_r(pairs + 1, IdxType(0xA5));
		const uint64_t got = radix_sort_join_pairs<IdxType>(start.data(), count.data(), rp.data(), n, m, out_l.data(), out_r.data(), pairs, flags);
		CHECK(got == pairs);
		if (got == want_l.size()) {
			CHECK(std::memcmp(out_l.data(), want_l.data(), pairs * sizeof(IdxType)) == 0);
			CHECK(std::memcmp(out_r.data(), want_r.data(), pairs * sizeof(IdxType)) == 0);
		}
		CHECK(out_l[pairs] == IdxType(0xA5) && out_r[pairs] == IdxType(0xA5));
		if (pairs) {   // one entry short: an error, nothing written
			std::vector<IdxType> small(pairs, IdxType(0xA5));
			bool thrown = false;
			try {
				radix_sort_join_pairs<IdxType>(start.data(), count.data(), rp.data(), n, m, small.data(), (IdxType *)nullptr, pairs - 1, flags);
			} catch (const std::exception &) {
				thrown = true;
			}
			CHECK(thrown && std::count(small.begin(), small.end(), IdxType(0xA5)) == (std::ptrdiff_t)pairs);
		}
	}
	CHECK(std::memcmp(left_was.data(), left.data(), n * sizeof(T)) == 0);
	CHECK(std::memcmp(right_was.data(), right.data(), m * sizeof(T)) == 0);
}

template <typename T, typename Less> static void both_orders(const char *name, const std::vector<T> &left, const std::vector<T> &right, Less less)
{
	auto greater = [&](const T &a, const T &b) { return less(b, a); };
	run<T, uint32_t>(name, left, right, RSX_ASCENDING, less);
	run<T, uint64_t>(name, left, right, RSX_DESCENDING, greater);
}

int main()
{
	uint64_t x = 88172645463325252ull;
	auto next = [&]() {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;
		return x;
	};
	for (size_t scale : {(size_t)1, (size_t)40}) {
		const size_t n = 700 * scale + 3, m = 500 * scale + 1;
		std::vector<uint32_t> ul, ur, dl, dr;
		std::vector<float> fl, fr;
		std::vector<int64_t> sl, sr;
		std::vector<uint8_t> bl, br;
		for (size_t i = 0; i < n + m; ++i) {
			const uint64_t r = next();
			const bool to_left = i < n;
			(to_left ? ul : ur).push_back((uint32_t)(r % (m / 3 + 1)) * 2654435761u);        // many to many, every bit varies
			(to_left ? dl : dr).push_back(0x00AB0000u | (uint32_t)(r % 3001) << 4);            // dense ids: direct addressing
			(to_left ? fl : fr).push_back((float)((int)(r % 2001) - 1000) / 8.0f);           // many ties, both signs
			(to_left ? sl : sr).push_back((int64_t)(r % 20001) - 10000);
			(to_left ? bl : br).push_back((uint8_t)(r >> 33));
		}
		fl[5] = INFINITY, fl[6] = -INFINITY, fl[7] = -0.0f, fl[8] = 0.0f, fr[1] = 0.0f, fr[2] = 0.0f, fr[3] = INFINITY;
		dl[9] = 0x80AB0010u;   // off the right keys' fixed bits
		// -0.0f orders before +0.0f by the key derivation and matches only itself; otherwise the usual order
		auto fless = [](float a, float c) { return a < c || (a == c && std::signbit(a) && !std::signbit(c)); };
		both_orders<uint32_t>("u32", ul, ur, [](uint32_t a, uint32_t c) { return a < c; });
		both_orders<uint32_t>("u32 dense", dl, dr, [](uint32_t a, uint32_t c) { return a < c; });
		both_orders<float>("float", fl, fr, fless);
		both_orders<int64_t>("i64", sl, sr, [](int64_t a, int64_t c) { return a < c; });
		both_orders<uint8_t>("u8", bl, br, [](uint8_t a, uint8_t c) { return a < c; });
	}
	{   // no right rows: zeros; no left rows: an iota; both outputs null throws
		uint32_t a[3] = {3, 1, 2}, v[2] = {2, 9}, start[3] = {0xA5, 0xA5, 0xA5}, count[3] = {0xA5, 0xA5, 0xA5}, rp[2] = {0xA5, 0xA5};
		CHECK(radix_sort_join<uint32_t>(a, 3, v, 0, start, count, rp) == 0);
		CHECK(count[0] == 0 && count[1] == 0 && count[2] == 0 && rp[0] == 0xA5);
		CHECK(radix_sort_join<uint32_t>(a, 3, v, 0, start, count, rp, RSX_ASCENDING, RSX_JOIN_LEFT) == 3);
		CHECK(radix_sort_join<uint32_t>(a, 0, v, 2, start, count, rp) == 0);
		CHECK(rp[0] == 0 && rp[1] == 1);
		bool thrown = false;
		try {
			radix_sort_join_pairs<uint32_t>(start, count, rp, 3, 2, (uint32_t *)nullptr, (uint32_t *)nullptr, 8);
		} catch (const std::exception &) {
			thrown = true;
		}
		CHECK(thrown);
	}
	if (failures) {
		std::printf("join_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("join_check: ok\n");
	return 0;
}
