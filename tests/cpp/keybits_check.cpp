// keybits_check: the host arithmetic of radix_sorting_amd/csrc/rsx_keybits.hpp on the CPU -- the shape of the bitmap over the packed
// varying bits, the variant of the mark kernel, the grids of the sweeps, the runs of a mask -- against the numbers the drivers of
// rsx_sort_unique*, rsx_sort_group* and rsx_sort_rankdata* each worked out for themselves before there was one place for them
// (and that tests/test_gpu_unique.py asserts as table_bytes).  No GPU and no library: the program includes the header alone; exits
// non-zero at the first mismatch.
#include "../../radix_sorting_amd/csrc/rsx_keybits.hpp"

#include <cstdio>
#include <cstring>

using namespace rsx;
typedef unsigned long long ull;

#define CHECK(cond, ...)                                \
	do {                                                \
		if (!(cond)) {                                  \
			fprintf(stderr, "keybits_check: %s: ", #cond); \
			fprintf(stderr, __VA_ARGS__);               \
			fprintf(stderr, "\n");                      \
			return 1;                                   \
		}                                               \
	} while (0)

static int check_runs(const char *what, ull mask, bool fits, unsigned n, const unsigned (*want)[3])
{
	BitRuns r;
	memset(&r, 0xEE, sizeof r);
	CHECK(bit_runs(mask, &r) == fits, "%s: mask %#llx", what, mask);
	if (!fits)
		return 0;
	CHECK(r.n == n, "%s: mask %#llx has %u runs, expected %u", what, mask, (unsigned)r.n, n);
	ull packed = 0;   // all ones through the runs: the lowest popcount(mask) bits
	for (unsigned i = 0; i < n; ++i) {
		CHECK(r.src[i] == want[i][0] && r.len[i] == want[i][1] && r.dst[i] == want[i][2], "%s: run %u is (src %u, len %u, dst %u)", what, i,
		      (unsigned)r.src[i], (unsigned)r.len[i], (unsigned)r.dst[i]);
		packed |= ((mask >> r.src[i]) & ((r.len[i] == 64 ? 0 : 1ull << r.len[i]) - 1)) << r.dst[i];
	}
	const int bits = __builtin_popcountll(mask);
	CHECK(packed == (bits == 64 ? ~0ull : (1ull << bits) - 1), "%s: the runs pack mask %#llx to %#llx", what, mask, packed);
	return 0;
}

int main()
{
	// (BitRuns is a kernel argument: one count and three times eight bytes, no padding)
	CHECK(sizeof(BitRuns) == 25 && alignof(BitRuns) == 1, "sizeof(BitRuns) = %zu", sizeof(BitRuns));

	// ---- the bitmap: words = max(1024, 2^vbits / 32), chunks of 1024 words, the mark kernel's variant and largest grid ----
	for (unsigned v = 1; v <= 30; ++v) {
		const BitmapShape s = bitmap_shape(v);
		const ull words = (1ull << v) / 32 > 1024 ? (1ull << v) / 32 : 1024;
		CHECK(s.words == words && s.chunks == words / 1024 && s.bytes == words * 4, "%u bits: %llu words, %llu chunks, %zu bytes", v, s.words, s.chunks,
		      s.bytes);
		CHECK(s.chunks >= 1 && s.chunks * 1024 == s.words, "%u bits: the words are no whole chunks", v);
		CHECK(s.lds_bits == (v <= 16 ? 16u : v <= 18 ? 18u : v <= 20 ? 20u : 0u), "%u bits: mark variant %u", v, s.lds_bits);
		CHECK(s.full == (v == 19 || v == 20 ? 256u : 512u), "%u bits: full grid %u", v, s.full);
	}
	static const struct { unsigned v; size_t bytes; } sizes[] = {{1, 4096}, {15, 4096}, {16, 8192}, {19, 65536}, {20, 131072}, {22, 1u << 19}, {24, 1u << 21}};
	for (const auto &c : sizes)
		CHECK(bitmap_shape(c.v).bytes == c.bytes, "%u bits: %zu bytes, expected %zu", c.v, bitmap_shape(c.v).bytes, c.bytes);

	// ---- the sweep grid: clamp(nvec / 16384, 1, full) over nvec = n x key bytes / 16 vectors ----
	static const struct { ull nvec; unsigned grid512, grid256; } grids[] = {
	    {0, 1, 1},           {16383, 1, 1},           {16384, 1, 1},           {2 * 16384 - 1, 1, 1},   {2 * 16384, 2, 2},
	    {256 * 16384, 256, 256}, {256 * 16384 + 16384, 257, 256}, {512 * 16384 - 1, 511, 256}, {512 * 16384, 512, 256}, {512 * 16384 + 1, 512, 256},
	    {513 * 16384, 512, 256}, {1ull << 40, 512, 256},
	};
	for (const auto &g : grids)
		for (size_t kb = 1; kb <= 8; kb *= 2) {
			const ull per = 16 / kb, n = g.nvec * per;   // keys in the vectors, and the most that begin no further one
			CHECK(sweep_grid(n, kb) == g.grid512 && sweep_grid(n + per - 1, kb) == g.grid512, "%llu vectors of %zu-byte keys: grid %u", g.nvec, kb,
			      sweep_grid(n, kb));
			CHECK(sweep_grid(n, kb, 512) == g.grid512 && sweep_grid(n, kb, 256) == g.grid256, "%llu vectors of %zu-byte keys: grid %u of 256", g.nvec, kb,
			      sweep_grid(n, kb, 256));
		}
	CHECK(sweep_grid(1u << 22, 4) == 64 && sweep_grid(1u << 22, 2) == 32 && sweep_grid(1u << 28, 4, 256) == 256, "2^22 keys: grid %u",
	      sweep_grid(1u << 22, 4));

	// ---- bit_runs ----
	static const unsigned three[3][3] = {{0, 4, 0}, {8, 8, 4}, {20, 4, 12}};
	static const unsigned eight[8][3] = {{0, 1, 0}, {2, 1, 1}, {4, 1, 2}, {6, 1, 3}, {8, 1, 4}, {10, 1, 5}, {12, 1, 6}, {14, 50, 7}};
	static const unsigned top[2][3] = {{3, 1, 0}, {60, 4, 1}};
	static const unsigned all[1][3] = {{0, 64, 0}};
	static const unsigned bit63[1][3] = {{63, 1, 0}};
	if (check_runs("three runs", 0x00F0FF0Full, true, 3, three) || check_runs("eight runs", 0xFFFFFFFFFFFFD555ull, true, 8, eight) ||
	    check_runs("nine runs", 0x15555ull, false, 0, nullptr) || check_runs("sixteen runs", 0x55555555ull, false, 0, nullptr) ||
	    check_runs("a run that ends at bit 63", 0xF000000000000008ull, true, 2, top) || check_runs("every bit", ~0ull, true, 1, all) ||
	    check_runs("bit 63 alone", 1ull << 63, true, 1, bit63) || check_runs("no bit", 0, true, 0, nullptr))
		return 1;

	// ---- one kept column: the byte is the packed value, and what bit_runs makes of the byte's mask ----
	for (unsigned c = 0; c < 8; ++c) {
		const BitRuns r = column_runs(c);
		BitRuns m;
		CHECK(r.n == 1 && r.src[0] == 8 * c && r.len[0] == 8 && r.dst[0] == 0, "column %u: (n %u, src %u, len %u, dst %u)", c, (unsigned)r.n,
		      (unsigned)r.src[0], (unsigned)r.len[0], (unsigned)r.dst[0]);
		CHECK(bit_runs(0xFFull << (8 * c), &m) && m.n == 1 && m.src[0] == r.src[0] && m.len[0] == 8 && m.dst[0] == 0, "column %u: bit_runs differs", c);
		for (unsigned i = 1; i < 8; ++i)
			CHECK(r.src[i] == 0 && r.len[i] == 0 && r.dst[i] == 0, "column %u: run %u is not zero", c, i);
	}
	printf("keybits_check OK\n");
	return 0;
}
