// unique_check.cpp -- radix_sort_unique (include/radix_sort.hpp) on Listing 7's array and on a float case.
// Built by `make cpp`, run by tests/test_gpu_unique.py (needs a GPU).  Prints "unique_check: ok" and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

int main()
{
	{   // bitmap_sort_16.c: the input array and the output it prints
		std::vector<uint16_t> src = {255, 45, 45, 45, 1, 2, 3, 255, 0, 65535}, aux(src.size(), 0xA5A5);
		const std::vector<uint16_t> want = {0, 1, 2, 3, 45, 255, 65535};
		size_t nu = 0;
		uint16_t *res = radix_sort_unique(src.data(), aux.data(), src.size(), &nu);
		CHECK(res == src.data() || res == aux.data());
		CHECK(nu == want.size());
		for (size_t i = 0; i < want.size() && i < nu; ++i)
			CHECK(res[i] == want[i]);
		for (size_t i = 0; i < nu; ++i)
			std::printf("%u ", (unsigned)res[i]);
		std::printf("\n");
	}
	{   // descending
		std::vector<uint16_t> src = {255, 45, 45, 45, 1, 2, 3, 255, 0, 65535}, aux(src.size(), 0);
		const std::vector<uint16_t> want = {65535, 255, 45, 3, 2, 1, 0};
		size_t nu = 0;
		uint16_t *res = radix_sort_unique(src.data(), aux.data(), src.size(), &nu, rsx_kdf::descending<uint16_t>{});
		CHECK(nu == want.size());
		for (size_t i = 0; i < want.size() && i < nu; ++i)
			CHECK(res[i] == want[i]);
	}
	{   // floats: distinct BIT PATTERNS in KDF order -- -0.0f sorts before +0.0f and both stay
		std::vector<float> src = {1.5f, -0.0f, 0.0f, -2.0f, 1.5f, INFINITY, -2.0f, 0.0f, -INFINITY, 1.5f}, aux(src.size(), 0.f);
		const std::vector<float> want = {-INFINITY, -2.0f, -0.0f, 0.0f, 1.5f, INFINITY};
		size_t nu = 0;
		float *res = radix_sort_unique(src.data(), aux.data(), src.size(), &nu);
		CHECK(nu == want.size());
		for (size_t i = 0; i < want.size() && i < nu; ++i)
			CHECK(std::memcmp(&res[i], &want[i], sizeof(float)) == 0);
	}
	{   // n < 2: src, aux untouched
		uint32_t one = 7, other = 0xA5;
		size_t nu = 99;
		CHECK(radix_sort_unique(&one, &other, 1, &nu) == &one && nu == 1 && other == 0xA5);
		CHECK(radix_sort_unique(&one, &other, 0, &nu) == &one && nu == 0);
	}
	if (failures) {
		std::printf("unique_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("unique_check: ok\n");
	return 0;
}
