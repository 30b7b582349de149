// threads_check.cpp -- four host threads inside the library at once, without an interpreter lock between them: three with a
// stream of their own (two hipStreamNonBlocking, one plain hipStreamCreate) on the device entry points, one on the host-pointer
// templates (radix_sort, radix_sort_rank), which use the default stream's context.  Every result is compared with std::sort /
// std::stable_sort of a copy; each thread makes one refused call and must find its own text in rsx_last_error(); one thread
// arms rsx_capture_histogram and must receive the counts of its own keys.  Needs a GPU; run by tests/test_gpu_cpp.py.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "radix_sort.hpp"
#include "radix_sort_rank.hpp"

static std::atomic<int> failures{0};
#define CHECK(cond)                                                                    \
	do {                                                                               \
		if (!(cond)) {                                                                 \
			printf("FAILED %s:%d (thread %d): %s\n", __FILE__, __LINE__, tid, #cond);  \
			++failures;                                                                \
		}                                                                              \
	} while (0)
#define HIP_OK(call) CHECK((call) == hipSuccess)

static const size_t SIZES[4] = {3000, 70001, 300001, 1000003};
static const int ROUNDS = 8;
static const size_t NMAX = 1000003;

// the double's place in the library's order: basic_kdfs::kdf (sign-magnitude to unsigned); descending = its complement
static uint64_t f64_key(double v)
{
	uint64_t u;
	std::memcpy(&u, &v, 8);
	return (u >> 63) ? ~u : u ^ 0x8000000000000000ull;
}

struct DeviceBufs {
	void *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;   // a, b: 8 bytes per element; c, d: 8 bytes per element (2 n indices)
};

template <typename T> static void up(int tid, void *dst, const std::vector<T> &v, hipStream_t s)
{
	HIP_OK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
}
template <typename T> static void down(int tid, std::vector<T> &v, const void *src, hipStream_t s)
{
	HIP_OK(hipMemcpyAsync(v.data(), src, v.size() * sizeof(T), hipMemcpyDeviceToHost, s));
	HIP_OK(hipStreamSynchronize(s));
}

static void stream_thread(int tid, hipStream_t s, bool with_histogram)
{
	DeviceBufs B;
	HIP_OK(hipMalloc(&B.a, NMAX * 8));
	HIP_OK(hipMalloc(&B.b, NMAX * 8));
	HIP_OK(hipMalloc(&B.c, NMAX * 8));
	HIP_OK(hipMalloc(&B.d, NMAX * 8));
	std::mt19937_64 rng(7000 + tid);
	for (int round = 0; round < ROUNDS; ++round) {
		const size_t n = SIZES[(round + tid) % 4];
		{   // rsx_sort_device, u32 ascending; once with the caller's histogram armed
			std::vector<uint32_t> in(n), got(n);
			for (auto &x : in)
				x = (uint32_t)rng();
			auto want = in;
			std::sort(want.begin(), want.end());
			up(tid, B.a, in, s);
			std::vector<uint64_t> hist(256 * 4, 0xA5A5A5A5A5A5A5A5ull);
			const bool armed = with_histogram && round == 1;
			if (armed)
				CHECK(rsx_capture_histogram(hist.data(), hist.size()) == RSX_OK);
			void *res = nullptr;
			rsx_info info;
			CHECK(rsx_sort_device(B.a, B.b, n, RSX_U32, RSX_ASCENDING, s, &res, &info) == RSX_OK);
			CHECK(res == (info.result_in_aux ? B.b : B.a));
			down(tid, got, res, s);
			CHECK(got == want);
			if (armed) {
				std::vector<uint64_t> counts(256 * 4, 0);
				for (uint32_t x : in)
					for (int j = 0; j < 4; ++j)
						++counts[256 * j + ((x >> (8 * j)) & 0xFF)];
				CHECK(hist == counts);
			}
		}
		{   // rsx_sort_device, f64 descending
			std::vector<double> in(n), got(n);
			for (auto &x : in)
				x = (double)(int64_t)rng() * 1e-3;
			auto want = in;
			std::stable_sort(want.begin(), want.end(), [](double x, double y) { return f64_key(x) > f64_key(y); });
			up(tid, B.a, in, s);
			void *res = nullptr;
			rsx_info info;
			CHECK(rsx_sort_device(B.a, B.b, n, RSX_F64, RSX_DESCENDING, s, &res, &info) == RSX_OK);
			down(tid, got, res, s);
			CHECK(std::memcmp(got.data(), want.data(), n * 8) == 0);
		}
		{   // rsx_sort_pairs_device: i32 keys (few distinct values in a part of them: ties), u32 payload 3 i + 1
			std::vector<int32_t> keys(n), gk(n);
			std::vector<uint32_t> vals(n), gv(n), perm(n);
			for (size_t i = 0; i < n; ++i) {
				keys[i] = (i % 3) ? (int32_t)rng() : (int32_t)(rng() % 64) - 32;
				vals[i] = (uint32_t)(3 * i + 1);
			}
			std::iota(perm.begin(), perm.end(), 0u);
			std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
			up(tid, B.a, keys, s);
			up(tid, B.c, vals, s);
			rsx_info info;
			CHECK(rsx_sort_pairs_device(B.a, B.b, B.c, B.d, n, RSX_I32, 4, RSX_ASCENDING, s, &info) == RSX_OK);
			down(tid, gk, info.result_in_aux ? B.b : B.a, s);
			down(tid, gv, info.result_in_aux ? B.d : B.c, s);
			bool same = true;
			for (size_t i = 0; i < n; ++i)
				same &= gk[i] == keys[perm[i]] && gv[i] == vals[perm[i]];
			CHECK(same);
		}
		{   // rsx_sort_rank_device: u16 keys with ties
			std::vector<uint16_t> keys(n);
			std::vector<uint32_t> want(n), got(n);
			for (auto &x : keys)
				x = (uint16_t)(rng() % 5000);
			std::iota(want.begin(), want.end(), 0u);
			std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
			up(tid, B.a, keys, s);
			void *res = nullptr;
			rsx_info info;
			CHECK(rsx_sort_rank_device(B.a, B.c, n, RSX_U16, 4, RSX_ASCENDING, s, &res, &info) == RSX_OK);
			CHECK(res == (info.result_in_aux ? (void *)((uint32_t *)B.c + n) : B.c));
			down(tid, got, res, s);
			CHECK(got == want);
		}
		{   // rsx_sort_inplace_async, then hipStreamSynchronize
			std::vector<uint32_t> in(n), got(n);
			for (auto &x : in)
				x = (uint32_t)rng() & 0x00FFFFFFu;
			auto want = in;
			std::sort(want.begin(), want.end());
			up(tid, B.a, in, s);
			CHECK(rsx_sort_inplace_async(B.a, B.b, n, RSX_U32, RSX_ASCENDING, s) == RSX_OK);
			HIP_OK(hipStreamSynchronize(s));
			down(tid, got, B.a, s);
			CHECK(got == want);
		}
		if (round == 3) {   // one refused call, another one in every thread: the text is this thread's
			void *res = nullptr;
			rsx_info info;
			const char *mine = tid == 0 ? "rsx_sort_device" : tid == 1 ? "rsx_sort_rank_device" : "rsx_sort_pairs_device";
			int rc;
			if (tid == 0)
				rc = rsx_sort_device(B.a, B.b, n, (rsx_dtype)99, RSX_ASCENDING, s, &res, &info);
			else if (tid == 1)
				rc = rsx_sort_rank_device(B.a, B.c, n, RSX_U32, 3, RSX_ASCENDING, s, &res, &info);
			else
				rc = rsx_sort_pairs_device(B.a, B.b, B.c, B.d, n, RSX_U32, 3, RSX_ASCENDING, s, &info);
			CHECK(rc == RSX_EINVAL);
			std::this_thread::yield();
			CHECK(std::strncmp(rsx_last_error(), mine, std::strlen(mine)) == 0 && rsx_last_error()[std::strlen(mine)] == ':');
		}
	}
	// the text is still this thread's after everything the others did meanwhile
	CHECK(std::strstr(rsx_last_error(), tid == 0 ? "rsx_sort_device:" : tid == 1 ? "rsx_sort_rank_device:" : "rsx_sort_pairs_device:") ==
	      rsx_last_error());
	HIP_OK(hipStreamSynchronize(s));
	HIP_OK(hipFree(B.a));
	HIP_OK(hipFree(B.b));
	HIP_OK(hipFree(B.c));
	HIP_OK(hipFree(B.d));
}

// the host-pointer templates: the default stream's context, host buffers staged on every call
static void host_thread(int tid)
{
	std::mt19937_64 rng(7000 + tid);
	for (int round = 0; round < ROUNDS; ++round) {
		const size_t n = SIZES[(round + tid) % 4];
		{
			std::vector<uint32_t> a(n), b(n);
			for (auto &x : a)
				x = (uint32_t)rng();
			auto want = a;
			std::sort(want.begin(), want.end());
			uint32_t *r = radix_sort(a.data(), b.data(), n);
			CHECK(std::memcmp(r, want.data(), n * 4) == 0);
		}
		{
			std::vector<int16_t> a(n);
			std::vector<uint32_t> ib(2 * n), want(n);
			for (auto &x : a)
				x = (int16_t)rng();
			std::iota(want.begin(), want.end(), 0u);
			std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return a[x] < a[y]; });
			uint32_t *r = radix_sort_rank(a.data(), ib.data(), n);
			CHECK(std::memcmp(r, want.data(), n * 4) == 0);
		}
		if (round == 3) {
			uint32_t two[2] = {2, 1};
			CHECK(rsx_sort_inplace_async(two, two, 2, (rsx_dtype)99, RSX_ASCENDING, nullptr) == RSX_EINVAL);
			CHECK(std::strstr(rsx_last_error(), "rsx_sort_inplace_async:") == rsx_last_error());
			CHECK(two[0] == 2 && two[1] == 1);
		}
	}
	CHECK(std::strstr(rsx_last_error(), "rsx_sort_inplace_async:") == rsx_last_error());
}

int main()
{
	const int tid = -1;
	if (rsx_device_count() <= 0) {
		printf("threads_check: no gfx950 device\n");
		return 2;
	}
	hipStream_t s[3];
	HIP_OK(hipStreamCreateWithFlags(&s[0], hipStreamNonBlocking));
	HIP_OK(hipStreamCreateWithFlags(&s[1], hipStreamNonBlocking));
	HIP_OK(hipStreamCreate(&s[2]));
	if (failures)
		return 1;
	{
		std::vector<std::thread> th;
		for (int t = 0; t < 3; ++t)
			th.emplace_back(stream_thread, t, s[t], t == 1);
		th.emplace_back(host_thread, 3);
		for (auto &x : th)
			x.join();
	}
	CHECK(rsx_last_error()[0] == '\0');      // (the main thread never failed: the workers' texts are theirs)
	for (int t = 0; t < 3; ++t)
		rsx_release_stream(s[t]);
	for (int t = 0; t < 3; ++t)
		HIP_OK(hipStreamDestroy(s[t]));
	rsx_release();
	if (failures) {
		printf("threads_check: %d FAILED\n", failures.load());
		return 1;
	}
	printf("threads_check OK\n");
	return 0;
}
