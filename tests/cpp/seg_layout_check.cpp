// seg_layout_check: SegLayout and SlotParts (radix_sorting_amd/csrc/rsx_seg_layout.hpp) on the CPU -- the layout of the segmented
// routes' control block against the sizes the routes allocated before there was one function for it, and the placement of
// level-1 slots in two arrays, whose mistakes no GPU test can steer (they depend on where hipMalloc puts the scratch array).
// No GPU and no library: the program includes the header alone; exits non-zero at the first mismatch.
#include "../../radix_sorting_amd/csrc/rsx_seg_layout.hpp"

#include <cstdio>

typedef unsigned long long ull;

#define CHECK(cond, ...)                                  \
	do {                                                  \
		if (!(cond)) {                                    \
			fprintf(stderr, "seg_layout_check: %s: ", #cond); \
			fprintf(stderr, __VA_ARGS__);                 \
			fprintf(stderr, "\n");                        \
			return 1;                                     \
		}                                                 \
	} while (0)

// The tile constants of the kernels, as literals (the header under test knows none of them):
//   Sc2Cfg<u32, NoVal>::TILE = 1024 x 32, Sc2Cfg<u64, NoVal>::TILE = 1024 x 16   (rsx_scatter2.hpp: BLOCK x KPT)
//   Pass16aCfg::TILE = 1024 x 24                                                    (rsx_pass16.hpp)
//   Pass2wCfg<u32>::TILE = 1024 x 12                                                (rsx_pass2w.hpp)
//   seg_extra_rows: 256 for 4-byte keys, 512 for 8-byte keys; seg_tile_rows: the tiles of the atom pass + 514, 8-byte keys at
//   least the status rows                                                           (rsx_route_levels.hpp)
static const ull TILE4 = 32768, TILE8 = 16384, TILE16A = 24576, TILE2W = 12288;

static ull ceil_div(ull a, ull b) { return (a + b - 1) / b; }

// `total`: the bytes seg_bytes<KT>(n) returned before SegLayout, worked out by hand from its formula
//   rows = ceil(n / TILE) + extra;  st = 256 + rows x 1024;  hist = 262144 x (key bytes - 1)
//   total = 256 + hist + (key bytes - 1) x st + 65536 x 16 + tile_rows x 16 + 260 x 4 + 65536 x 4
static int check_layout(size_t kb, ull n, ull total)
{
	const ull tile = kb == 4 ? TILE4 : TILE8, extra = kb == 4 ? 256 : 512;
	const ull rows = ceil_div(n, tile) + extra;
	const ull tile_rows = kb == 4 ? ceil_div(n, TILE16A) + 514 : (rows > ceil_div(n, TILE2W) + 514 ? rows : ceil_div(n, TILE2W) + 514);
	const SegLayout l = seg_layout_for(kb, (size_t)n, (size_t)tile, extra, tile_rows);
	CHECK(seg_rows((size_t)n, (size_t)tile, extra) == rows && l.rows == rows, "%zu-byte keys, n = %llu: rows %llu, expected %llu", kb, n, (ull)l.rows, rows);
	CHECK(l.st_bytes == 256 + rows * 1024, "%zu-byte keys, n = %llu: st_bytes %zu", kb, n, l.st_bytes);
	// the regions in order, none overlapping, each of the size the routes allocated
	const size_t off[8] = {0, l.hist_off, l.status_off, l.segtab_off, l.tiles_off, l.btile_off, l.redo_off, l.total};
	const ull size[7] = {256, 262144ull * (kb - 1), (kb - 1) * (256 + rows * 1024), 65536ull * 16, tile_rows * 16, 260 * 4, 65536ull * 4};
	static const char *const name[7] = {"ctl", "hist", "status", "segtab", "tiles", "btile", "redo"};
	for (int r = 0; r < 7; ++r) {
		CHECK(off[r] < off[r + 1], "%zu-byte keys, n = %llu: region %s at %zu does not lie in front of the next at %zu", kb, n, name[r], off[r], off[r + 1]);
		CHECK(off[r + 1] - off[r] == size[r], "%zu-byte keys, n = %llu: region %s holds %zu bytes, expected %llu", kb, n, name[r], off[r + 1] - off[r], size[r]);
		CHECK(off[r] % 16 == 0, "%zu-byte keys, n = %llu: region %s at %zu is not 16-byte aligned", kb, n, name[r], off[r]);
	}
	CHECK(l.total == total, "%zu-byte keys, n = %llu: total %zu, expected %llu", kb, n, l.total, total);
	// the status region of every pass inside the status part, its words 256 bytes behind its ticket
	for (size_t j = 0; j + 1 < kb; ++j) {
		CHECK(l.status(j) == l.status_off + j * l.st_bytes && l.cursors(j) == l.status(j) + 256, "%zu-byte keys, n = %llu: status(%zu)", kb, n, j);
		CHECK(l.status(j) + l.st_bytes <= l.segtab_off, "%zu-byte keys, n = %llu: status region %zu ends behind the status part", kb, n, j);
	}
	return 0;
}

// One placement: `lo` slots of `cap1` elements in the spare buffer of n elements at `spare`, the others in a scratch array at
// `scratch` sized as blind_enqueue sizes it ((256 - lo) x cap1 + tile elements).  Both addresses are numbers only: nothing is read.
static int check_parts(const char *what, uintptr_t spare, uintptr_t scratch, unsigned lo, unsigned cap1, size_t esz, ull tile, bool fits)
{
	const SlotParts p((const void *)spare, (const void *)scratch, lo, cap1, esz, (size_t)tile);
	CHECK(p.fits32() == fits, "%s: fits32() is %d, span %llu", what, (int)p.fits32(), (ull)p.span);
	if (!fits)
		return 0;
	const uintptr_t scratch_end = scratch + ((ull)(256 - lo) * cap1 + tile) * esz, spare_end = spare + (ull)lo * cap1 * esz;
	CHECK(p.base == (lo && spare < p.hi ? spare : p.hi), "%s: the base is not the lower part", what);
	CHECK(p.hi + (ull)lo * cap1 * esz == scratch, "%s: hi is not lo slots in front of the scratch array", what);
	for (unsigned d = 0; d < 256; ++d) {
		const ull off = d < lo ? p.off_lo : p.off_hi;
		const ull elem = off + (ull)d * cap1;   // (what the pass adds to the base, in 32 bits)
		const uintptr_t a = p.base + (uintptr_t)(elem * esz);
		CHECK(elem + cap1 <= 0xFFFFFFFFull + 1, "%s: slot %u ends at element %llu of the base", what, d, elem + cap1);
		if (d < lo)
			CHECK(a == spare + (ull)d * cap1 * esz && a + (ull)cap1 * esz <= spare_end, "%s: slot %u does not lie in the spare buffer", what, d);
		else
			CHECK(a == scratch + (ull)(d - lo) * cap1 * esz && a + (ull)cap1 * esz <= scratch_end, "%s: slot %u does not lie in scratch", what, d);
	}
	// the last slot plus a tile (where a lost attempt's runs are dumped) ends inside scratch, within 32-bit reach of the base
	const ull last = p.off_hi + 255ull * cap1;
	CHECK(p.base + (uintptr_t)((last + cap1 + tile) * esz) <= scratch_end, "%s: the dump area ends behind the scratch array", what);
	CHECK(last + cap1 + tile <= p.span && p.span <= 0xFFFFFFFFull, "%s: the dump area ends at element %llu, span %llu", what, last + cap1 + tile, (ull)p.span);
	return 0;
}

int main()
{
	// ---- SegLayout: 4- and 8-byte keys at n = 1, TILE - 1, TILE, TILE + 1, 2^22, 2^24 + 99, 2^28, 2^30 - 1 ----
	static const struct { size_t kb; ull n, total; } cases[] = {
	    {4, 1, 2896960},           {4, 32767, 2896976},        {4, 32768, 2896976},        {4, 32769, 2900048},
	    {4, 1ull << 22, 3289824},  {4, (1ull << 24) + 99, 4480736}, {4, 1ull << 28, 28234464}, {4, (1ull << 30) - 1, 104256224},
	    {8, 1, 6834240},           {8, 16383, 6834256},        {8, 16384, 6834256},        {8, 16385, 6841424},
	    {8, 1ull << 22, 8667536},  {8, (1ull << 24) + 99, 14196112}, {8, 1ull << 28, 124617104}, {8, (1ull << 30) - 1, 477987216},
	};
	for (const auto &c : cases)
		if (check_layout(c.kb, c.n, c.total))
			return 1;

	// ---- SlotParts ----
	const uintptr_t A = (uintptr_t)1 << 40;   // (an address with room below it for the virtual slot 0)
	for (size_t esz = 4; esz <= 8; esz += 4) {
		const ull tile = esz == 4 ? TILE4 : TILE8;
		const unsigned cap1 = 1310720;   // slot_cap_for(2^20): the level-1 slots of 2^28 keys
		const unsigned lo = 204;         // n / cap1 of 2^28 keys
		const ull reach = 257ull * cap1 + tile;   // elements behind the virtual slot 0 a pass may touch
		// spare below scratch, spare above scratch, neighbours and a GiB apart
		if (check_parts("spare below scratch", A, A + ((ull)1 << 30), lo, cap1, esz, tile, true) ||
		    check_parts("spare above scratch", A + ((ull)8 << 30), A, lo, cap1, esz, tile, true) ||
		    check_parts("spare ends where scratch begins", A, A + (ull)lo * cap1 * esz, lo, cap1, esz, tile, true))
			return 1;
		// lo = 0: everything in scratch, whatever the spare buffer is; lo = 255: one slot in scratch
		if (check_parts("lo = 0", 0, A, 0, cap1, esz, tile, true) || check_parts("lo = 0, a spare buffer far away", A + ((ull)1 << 44), A, 0, cap1, esz, tile, true) ||
		    check_parts("lo = 255, spare below", A, A + ((ull)3 << 30), 255, cap1, esz, tile, true) ||
		    check_parts("lo = 255, spare above", A + ((ull)3 << 31), A, 255, cap1, esz, tile, true))
			return 1;
		// a span of exactly 2^32 - 1 elements fits, one of 2^32 does not: the parts (2^32 - 1 - reach) and (2^32 - reach) elements apart
		const ull gap_fit = 0xFFFFFFFFull - reach, gap_no = gap_fit + 1;
		const uintptr_t scratch = A + ((ull)1 << 36), hi = scratch - (ull)lo * cap1 * esz;
		if (check_parts("span 2^32 - 1, spare below", hi - gap_fit * esz, scratch, lo, cap1, esz, tile, true) ||
		    check_parts("span 2^32, spare below", hi - gap_no * esz, scratch, lo, cap1, esz, tile, false) ||
		    check_parts("span 2^32 - 1, spare above", hi + gap_fit * esz, scratch, lo, cap1, esz, tile, true) ||
		    check_parts("span 2^32, spare above", hi + gap_no * esz, scratch, lo, cap1, esz, tile, false))
			return 1;
		const SlotParts edge((const void *)(hi - gap_fit * esz), (const void *)scratch, lo, cap1, esz, (size_t)tile);
		CHECK(edge.span == 0xFFFFFFFFull, "the span of the edge case is %llu", (ull)edge.span);
	}
	printf("seg_layout_check OK\n");
	return 0;
}
