// rsx_locate_shape.hpp: the arithmetic of rsx_sort_locate*'s search route (rsx_locate.hpp) -- the digit of the start
// table, its entries, the number of halvings, the per-key search, the layout of the workgroup's LDS, the shares of the grid
// and what the finish reads out of the summed counters.  Nothing of HIP and nothing of Ctx is used here: every function is
// __host__ __device__ under hipcc and plain C++ otherwise; tests/cpp/locate_shape_check.cpp includes this file alone and checks it
// on the CPU against std::upper_bound.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RSX_LOCATE_HD __host__ __device__ inline
#else
#define RSX_LOCATE_HD inline
#endif

namespace rsx {

typedef unsigned long long u64;
typedef unsigned int u32;

// The search kernel: a tile is LOCATE_TILE keys (four per thread), a workgroup owns a contiguous share of whole tiles -- at least
// LOCATE_SHARE_TILES of them, and there are at most LOCATE_MAX_WGS shares (one workgroup per CU: its LDS is LOCATE_LDS_BYTES).
enum : u32 { LOCATE_MAX_VALUES = 4096, LOCATE_THREADS = 1024, LOCATE_TILE = 4096, LOCATE_SHARE_TILES = 4, LOCATE_MAX_WGS = 256,
             LOCATE_LDS_BYTES = 147456, LOCATE_MAX_SETS = 32, LOCATE_START_ENTRIES = 257 };

// ---- the edges ----------------------------------------------------------------------------------------------------------------
// Over the values' derived keys in ascending order: position i is a head where its key differs from the one before it.  Head
// number d is edge E[d], and cum[d] = its position = the values below it; cum[D] = m.  So cum[b] values lie at or below edge b - 1.
template <typename KT> RSX_LOCATE_HD bool locate_is_head(u64 i, KT k, KT prev) { return i == 0 || k != prev; }

// ---- the start table ----------------------------------------------------------------------------------------------------------
// The edges E[0 .. D) ascend strictly.  The leading bits E[0] and E[D-1] share are the same in every edge and in every key
// between them; the digit of a key is the eight bits behind them (fewer differ: the lowest eight bits).
template <typename KT> RSX_LOCATE_HD u32 locate_shift(KT first, KT last)
{
	const KT x = (KT)(first ^ last);
	if (!x)
		return 0;
	const u32 top = 64u - (u32)__builtin_clzll((u64)x);   // bits from the highest differing one down
	return top > 8u ? top - 8u : 0u;
}
template <typename KT> RSX_LOCATE_HD u32 locate_digit(KT k, u32 shift) { return (u32)(k >> shift) & 0xFFu; }

// start[d], d in 0 .. 256: the first of the edges E[0 .. D-1) whose digit is at least d (start[256] = D - 1).  The LAST edge is
// left out: a key that reaches it is answered by the compare against it, so a digit's span holds at most D - 1 <= 4095 edges.
template <typename KT> RSX_LOCATE_HD u32 locate_start_entry(const KT *E, u32 D, u32 shift, u32 d)
{
	u32 lo = 0, hi = D ? D - 1u : 0u;
	while (lo < hi) {
		const u32 mid = (lo + hi) / 2u;
		if (locate_digit<KT>(E[mid], shift) < d)
			lo = mid + 1u;
		else
			hi = mid;
	}
	return lo;
}

// halvings that find a count in 0 .. span: the smallest s with 2^s > span
RSX_LOCATE_HD u32 locate_steps(u32 span)
{
	u32 s = 0;
	while (((u32)1 << s) <= span)
		++s;
	return s;
}
template <typename ST> RSX_LOCATE_HD u32 locate_max_span(const ST *start)
{
	u32 most = 0;
	for (u32 d = 0; d < 256u; ++d) {
		const u32 span = (u32)start[d + 1u] - (u32)start[d];
		most = span > most ? span : most;
	}
	return most;
}

// ---- the search of one key ----------------------------------------------------------------------------------------------------
// b = the number of edges <= k (0 .. D), *eq = 1 where k IS an edge (then E[b - 1] == k).  `steps` halvings for every key,
// whatever its digit, and no branch on the key: the two compares against E[0] and E[D-1] override what the halvings found.
template <typename KT, typename ST> RSX_LOCATE_HD u32 locate_search(const KT *E, u32 D, const ST *start, u32 shift, u32 steps, KT k, u32 *eq)
{
	const bool below = k < E[0], above = k >= E[D - 1u];
	const u32 d = locate_digit<KT>(k, shift);
	const u32 lo = (u32)start[d], span = (u32)start[d + 1u] - lo;
	u32 c = 0;
	for (u32 s = steps; s-- > 0u;) {
		const u32 cand = c + ((u32)1 << s);
		const u32 at = lo + (cand <= span ? cand : span);
		const KT e = E[at ? at - 1u : 0u];
		c = (cand <= span && e <= k) ? cand : c;
	}
	const u32 b = below ? 0u : above ? D : lo + c;
	*eq = (b && E[b ? b - 1u : 0u] == k) ? 1u : 0u;
	return b;
}

// the counter a key adds to, of 2 (D + 1): keys with b edges at or below them, apart from (2b) or on (2b + 1) edge b - 1
RSX_LOCATE_HD u32 locate_counter(u32 b, u32 eq) { return 2u * b + eq; }
RSX_LOCATE_HD u32 locate_counters(u32 D) { return 2u * (D + 1u); }
// the bin of a key: cum[b] = the values at or below edge b - 1 (cum[0] = 0, cum[D] = m); BELOW: those strictly below the key
RSX_LOCATE_HD u32 locate_bin_entry(u32 b, u32 eq, bool below) { return below ? b - eq : b; }

// ---- the finish ---------------------------------------------------------------------------------------------------------------
// cnt[0 .. 2 (D + 1)): the counters summed over every workgroup.  tot[b] = cnt[2b] + cnt[2b + 1] keys have exactly b edges at or
// below them; incl[b] = tot[0] + .. + tot[b].  For a value whose derived key is edge d: the keys below it have at most d edges at
// or below them, the keys equal to it have d + 1 and sit on the edge.
RSX_LOCATE_HD u64 locate_total(const u64 *cnt, u32 b) { return cnt[2u * b] + cnt[2u * b + 1u]; }
RSX_LOCATE_HD u64 locate_less(const u64 *incl, u32 d) { return incl[d]; }
RSX_LOCATE_HD u64 locate_equal(const u64 *cnt, u32 d) { return cnt[2u * (d + 1u) + 1u]; }

// ---- the workgroup's LDS ------------------------------------------------------------------------------------------------------
// [E: D keys][cum: D + 1 indices, where bins are wanted][start: 257 u32][R sets of 2 (D + 1) u32 counters], each part a
// multiple of 8 bytes.  R is as many sets as fit, at most LOCATE_MAX_SETS (`forced`: RSX_LOCATE_COUNTER_SETS, cut to what fits).
struct LocateLds {
	u32 cum_off, start_off, cnt_off, sets, bytes;
};
RSX_LOCATE_HD u32 locate_round8(u32 x) { return (x + 7u) & ~7u; }
RSX_LOCATE_HD LocateLds locate_lds(u32 D, u32 key_bytes, u32 idx_bytes, bool want_bin, u32 forced)
{
	LocateLds l;
	l.cum_off = locate_round8(D * key_bytes);
	l.start_off = l.cum_off + (want_bin ? locate_round8((D + 1u) * idx_bytes) : 0u);
	l.cnt_off = l.start_off + locate_round8(LOCATE_START_ENTRIES * 4u);
	const u32 per = locate_counters(D) * 4u;
	u32 fit = (LOCATE_LDS_BYTES - l.cnt_off) / per;
	fit = fit > LOCATE_MAX_SETS ? (u32)LOCATE_MAX_SETS : fit;
	l.sets = forced && forced < fit ? forced : fit;
	l.bytes = l.cnt_off + l.sets * per;
	return l;
}

// ---- the grid -----------------------------------------------------------------------------------------------------------------
// `body` keys are read as whole tiles; what is left behind the last whole tile (and before the first 16-byte boundary) is
// workgroup 0's.  A share is at least LOCATE_SHARE_TILES tiles, and there are at most LOCATE_MAX_WGS of them.
struct LocateGrid {
	u64 tiles, share_tiles;
	u32 wgs;
};
RSX_LOCATE_HD LocateGrid locate_grid(u64 body)
{
	LocateGrid g;
	g.tiles = body / LOCATE_TILE;
	const u64 even = (g.tiles + LOCATE_MAX_WGS - 1u) / LOCATE_MAX_WGS;
	g.share_tiles = even > LOCATE_SHARE_TILES ? even : (u64)LOCATE_SHARE_TILES;
	const u64 wgs = (g.tiles + g.share_tiles - 1u) / g.share_tiles;
	g.wgs = (u32)(wgs ? wgs : 1u);
	return g;
}
// tiles a workgroup may take between two flushes of its 32-bit counters: fewer than 2^32 keys
RSX_LOCATE_HD u64 locate_flush_tiles() { return (((u64)1 << 32) - 1u) / LOCATE_TILE - 4u; }

}  // namespace rsx
