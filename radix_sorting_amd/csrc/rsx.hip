// rsx.hip -- host side of librsx.so: the extern "C" surface declared in
// include/rsx.h on top of the kernels in rsx_kernels.hpp.
//
// The control flow mirrors rs_sort_main (radix_sort.hpp:31-93): histogram +
// pre-sorted test -> early exit -> column probe -> exclusive scan -> one stable
// scatter pass per kept column, ping-ponging two buffers -> "returned pointer".
// There is deliberately no CPU path here: if HIP cannot give us a gfx950
// device, every entry point fails with RSX_ENODEVICE.
#include "../../include/rsx.h"
#include "rsx_kernels.hpp"
#include "rsx_scatter2.hpp"
#include "rsx_small.hpp"
#include "rsx_hybrid.hpp"
#include "rsx_leaf16.hpp"
#include "rsx_pass16.hpp"
#include "rsx_pass32.hpp"
#include "rsx_leafc.hpp"
#include "rsx_logroute.hpp"
#include "rsx_pass64.hpp"
#include "rsx_unique.hpp"
#include "rsx_group.hpp"
#include "rsx_rankdata.hpp"
#include "rsx_topk.hpp"
#include "rsx_nth.hpp"
#include "rsx_lex.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <functional>
#include <atomic>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

using namespace rsx;

#include "rsx_env.hpp"          // the RSX_* switches
#include "rsx_seg_layout.hpp"   // SegLayout, SlotParts: where the segmented routes' control block and level-1 slots lie
#include "rsx_ctx.hpp"          // the error convention, DevBuf, Ctx, profiling, get_ctx
#include "rsx_route_levels.hpp" // MSB passes and leaves behind a histogram: the control block, the leaves, one and two levels
#include "rsx_route_blind.hpp"  // ... and without one: gates, sizes, blind_enqueue / pairs_blind_enqueue and their blocking sorts

namespace {

// tiles per super-tile: as many as keeps at least ~2048 super-tiles in flight, at most 8
u32 choose_tps(size_t n, size_t tile)
{
	const u64 tiles = (n + tile - 1) / tile;
	u64 tps = tiles / 2048;
	if (tps > 8)
		tps = 8;
	if (tps < 1)
		tps = 1;
	return (u32)tps;
}

// ---- phase 1: histogram + plan (radix_sort.hpp:48-80) --------------------------
template <typename KT>
int launch_hist(Ctx &c, const KT *d_src, size_t n, KdfArgs<KT> ka, u64 *d_hist, u32 *d_unsorted, u32 colmask = ~0u,
                const HistFuse *fuse = nullptr)
{
	typedef HistCfg<KT> C;
	const u64 per_block = (u64)C::BLOCK * C::U * C::VEC;     // elements one workgroup covers per sweep
	u64 blocks = (n + per_block - 1) / per_block;
	if (blocks > 512)                                         // 256 CUs x 2 workgroups of 1024 threads
		blocks = 512;
	if (blocks < 1)
		blocks = 1;
	const u32 cols256 = (u32)sizeof(KT) * 256;
	RSX_TRY(c.hpart.ensure((size_t)blocks * cols256 * sizeof(u32)));
	ProfScope prof(0, (u64)n * sizeof(KT), c.stream);
	// up to 128 workgroups add their counts to the histogram themselves (one launch and its gap less: 7 of the 62 us of
	// a 10^5-key sort); beyond that the rows are summed by a kernel of their own
	const bool direct = blocks <= 128;
	const u32 *gate = c.pass_gate ? &c.pass_gate->mode : nullptr;
	HistFuse nofuse{};
	nofuse.gate = gate;
	if (fuse) {
		// the kernel also zeroes what the caller names (FUSED, rsx_hist.hpp)
		if (ka.fmask == 0 && ka.sflip == 0 && ka.desc == 0)
			hipLaunchKernelGGL((rsx_hist_kernel<KT, C, HIST_PLAIN, true>), dim3((unsigned)blocks), dim3(C::BLOCK), 0, c.stream, d_src,
			                   (u64)n, (u32 *)c.hpart.p, d_unsorted, ka, colmask, direct ? d_hist : (u64 *)nullptr, *fuse);
		else
			hipLaunchKernelGGL((rsx_hist_kernel<KT, C, HIST_GENERIC, true>), dim3((unsigned)blocks), dim3(C::BLOCK), 0, c.stream, d_src,
			                   (u64)n, (u32 *)c.hpart.p, d_unsorted, ka, colmask, direct ? d_hist : (u64 *)nullptr, *fuse);
	} else
	// keys that are their own KDF (unsigned, ascending) take the instantiation without the KDF arithmetic
	if (ka.fmask == 0 && ka.sflip == 0 && ka.desc == 0)
		hipLaunchKernelGGL((rsx_hist_kernel<KT, C, HIST_PLAIN>), dim3((unsigned)blocks), dim3(C::BLOCK), 0, c.stream, d_src, (u64)n,
		                   (u32 *)c.hpart.p, d_unsorted, ka, colmask, direct ? d_hist : (u64 *)nullptr, nofuse);
	else
		hipLaunchKernelGGL((rsx_hist_kernel<KT, C, HIST_GENERIC>), dim3((unsigned)blocks), dim3(C::BLOCK), 0, c.stream, d_src, (u64)n,
		                   (u32 *)c.hpart.p, d_unsorted, ka, colmask, direct ? d_hist : (u64 *)nullptr, nofuse);
	if (!direct)
		hipLaunchKernelGGL(rsx_hist_reduce_kernel, dim3((unsigned)sizeof(KT), HIST_REDUCE_SPLIT), dim3(256), 0, c.stream,
		                   (const u32 *)c.hpart.p, d_hist, (u32)blocks, cols256, gate);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

template <typename KT>
int plan_phase(Ctx &c, const KT *d_src, size_t n, KdfArgs<KT> ka, Plan *out, size_t status_total = 0,
               HybCaps caps = HybCaps{0, 0, 0, 0}, bool fuse_ok = false, bool *self_plan = nullptr)
{
	// self_plan (in: the caller would like pass 0 to derive the plan itself, SCATTER_SELF_PLAN; out: whether it has to):
	// then only the histogram is enqueued here -- no plan kernel, no event
	const size_t hist_bytes = sizeof(KT) * 256 * sizeof(u64);
	if (c.hist.external)
		RSX_TRY(c.hist.ensure(hist_bytes));
	// (fuse_ok: the blocking entry points only.  A captured graph replays the SAME launch, so it cannot alternate between
	// the two sets of flags: the device-scheduled *_async sorts keep the separate zeroing launch, and a set of their own
	// (Ctx::ASYNC_SET) -- a replay between two blocking sorts would otherwise fill the set the second one trusts to be zero.)
	if (fuse_ok && status_total && !out && !c.small.external && c.gen < Ctx::ASYNC_SET && !env().no_fused_hist) {
		// Small arrays: the histogram kernel also zeroes (no launch for that).  The set of flags / histogram this sort uses
		// was zeroed by the previous sort (or at start-up); this sort's histogram kernel zeroes the other set for the next
		// one, and the status words of its own passes (which run after it).  One workgroup then makes the plan.
		RSX_TRY(c.status.ensure(status_total));
		c.gen ^= 1u;
		HistFuse f{};
		f.z0 = (u32x4 *)c.small_set_other();
		f.n0 = Ctx::SMALL_BYTES / 16;
		f.z1 = (u32x4 *)c.ghist_other();
		f.n1 = Ctx::HIST_SET_BYTES / 16;
		f.z2 = (u32x4 *)c.status.p;
		f.n2 = status_total / 16;
		RSX_TRY(launch_hist<KT>(c, d_src, n, ka, c.ghist(), c.unsorted(), ~0u, &f));
		if (self_plan && *self_plan)
			return RSX_OK;
		hipLaunchKernelGGL((rsx_plan_all_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, d_src, (u64)n, c.ghist(), ka, c.kept(),
		                   c.hotd(), (const u32 *)c.unsorted(), c.plan(), c.dev_host_plan, caps);
		HIP_TRY(hipGetLastError());
		if (!c.plan_ev)
			HIP_TRY(hipEventCreateWithFlags(&c.plan_ev, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(c.plan_ev, c.stream));
		return RSX_OK;
	}
	if (self_plan)
		*self_plan = false;
	if (status_total) {
		// flags, histogram and the status words of every pass of this sort in one launch
		RSX_TRY(c.status.ensure(status_total));
		const u64 total16 = (256 + hist_bytes + status_total) / 16;
		const unsigned blocks = (unsigned)std::min<u64>((total16 + 255) / 256, 2048);
		hipLaunchKernelGGL(rsx_zero3_kernel, dim3(blocks), dim3(256), 0, c.stream, (u32x4 *)c.small_set(), (u64)(256 / 16),
		                   (u32x4 *)c.ghist(), (u64)(hist_bytes / 16), (u32x4 *)c.status.p, (u64)(status_total / 16),
		                   c.pass_gate ? &c.pass_gate->mode : (const u32 *)nullptr);
	} else {
		HIP_TRY(hipMemsetAsync(c.ghist(), 0, hist_bytes, c.stream));
		HIP_TRY(hipMemsetAsync(c.small_set(), 0, 256, c.stream));
	}
	RSX_TRY(launch_hist<KT>(c, d_src, n, ka, c.ghist(), c.unsorted()));
	hipLaunchKernelGGL((rsx_plan_all_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, d_src, (u64)n, c.ghist(), ka, c.kept(),
	                   c.hotd(), (const u32 *)c.unsorted(), c.plan(), c.dev_host_plan, caps,
	                   c.pass_gate ? &c.pass_gate->mode : (const u32 *)nullptr);
	HIP_TRY(hipGetLastError());
	if (!out) {   // the caller enqueues more work and collects the plan with plan_wait()
		if (c.small.external)
			return RSX_OK;   // (a caller-owned workspace: nobody waits for this plan on the host)
		if (!c.plan_ev)
			HIP_TRY(hipEventCreateWithFlags(&c.plan_ev, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(c.plan_ev, c.stream));
		return RSX_OK;
	}
	HIP_TRY(hipStreamSynchronize(c.stream));
	*out = *c.host_plan;
	return RSX_OK;
}

int plan_wait(Ctx &c, Plan *out)
{
	HIP_TRY(hipEventSynchronize(c.plan_ev));
	*out = *c.host_plan;
	return RSX_OK;
}

// the exit of the blocking drivers on sorted input (radix_sort.hpp:60-62): no column was sorted by, the result is where the input is
inline int finish_sorted(rsx_info *info, void **result = nullptr, void *where = nullptr)
{
	if (info) {
		info->early_exit = 2;
		info->ncols = 0;
	}
	if (result)
		*result = where;
	return RSX_OK;
}

// the flags of a pass over a column with hot digits (Plan::hot): the HOT kernel + the column, for its hotd word
inline u32 hot_flags(u32 hotmask, u32 col)
{
	if (env().no_hot)   // (diagnostic: the plain kernels on columns with hot digits)
		return 0u;
	return (hotmask >> col & 1u) ? ((u32)SCATTER_HOT | (col << SCATTER_COL_SHIFT)) : 0u;
}

// ---- phase 2: one scatter pass (radix_sort.hpp:83-90) -----------------------------
// gbase[digit]: exclusive offset of the digit for this pass's column
template <typename KT, typename VT, typename C2, typename KTO = KT>
int launch_scatter2(Ctx &c, const KT *kin, KTO *kout, const VT *vin, VT *vout, size_t n, u32 shift, const u64 *gbase,
                    KdfArgs<KT> ka, u32 flags, const Plan *dplan, int region, u32 pass_index, u32 oshift = 0)
{
	const u64 tiles = (n + C2::TILE - 1) / C2::TILE;
	const u32 tps = (u32)C2::TPS;   // 1: a tile is its own super-tile (32-bit cells leave no LDS for a second tile's counts)
	const bool wide = n >= (1ull << 30);   // counter width by n, as radix_sort.hpp:102-114 does
	const size_t st_bytes = 256 + tiles * 256 * (wide ? 8 : 4);
	char *base = (char *)c.status.p;
	if (region < 0) {   // own region, zeroed here
		RSX_TRY(c.status.ensure(st_bytes));
		HIP_TRY(hipMemsetAsync(c.status.p, 0, st_bytes, c.stream));
		base = (char *)c.status.p;
	} else {            // region `region` of a buffer the caller has sized (status_bytes) and zeroed (plan_phase)
		base += (size_t)region * st_bytes;
	}
	u32 *ticket = (u32 *)base;
	void *st = base + 256;
	ProfScope prof(1, (u64)n * (sizeof(KT) + sizeof(KTO) + 2 * val_bytes<VT>::value), c.stream);
	const dim3 grid((unsigned)tiles);
	// keys that are their own KDF (unsigned ascending, no bucket table) take the kernel without the KDF arithmetic;
	// columns with a hot digit (Plan::hot) take the instantiation that tests every round for a wave-uniform digit
	const bool integer = val_bytes<VT>::value == 0 && ka.fmask == 0;
	const bool plain = integer && ka.sflip == 0 && ka.desc == 0;
	const bool hot = (flags & SCATTER_HOT) != 0;
	flags &= ~(u32)SCATTER_HOT;
	// RSX_ELEM_LOADS=1: whole tiles are read with element loads instead of 16-byte loads + a transposition through the LDS
	// (measured on 2^28 u32 keys: 0.490-0.505 against 0.503-0.513 ms per pass in the probe; off by default)
	if (env().elem_loads)
		flags |= SCATTER_ELEM_LOADS;
#define RSX_LAUNCH2(ST, DIGV, HOTV)                                                                                        \
	hipLaunchKernelGGL((rsx_scatter2_kernel<KT, VT, ST, C2, false, DIGV, HOTV, KTO>), grid, dim3(C2::BLOCK), 0, c.stream, kin, kout, \
	                   vin, vout, (u64)n, shift, gbase, tps, (ST *)st, ticket, ka, flags, (u64 *)nullptr, dplan, pass_index,  \
	                   oshift, (const u32 *)c.hotd(), SegArgs{nullptr, c.pass_gate, nullptr, 0, 0, nullptr}, c.pass_alt, c.pass_sp)
	// quarter tiles are for arrays of a few million keys: never 2^30 of them, and hot digits cost little there -- those
	// instantiations are left out of the build
	constexpr bool SMALL_CFG = C2::KPT < Sc2Cfg<KT, VT>::KPT;
#define RSX_LAUNCH2_ST(DIGV)                           \
	do {                                               \
		if constexpr (SMALL_CFG) {                     \
			if (wide)                                  \
				return fail(RSX_EINVAL, "quarter tiles with 2^30 keys or more"); \
			RSX_LAUNCH2(u32, DIGV, false);             \
		} else if (wide) {                             \
			if (hot)                                   \
				RSX_LAUNCH2(u64, DIGV, true);          \
			else                                       \
				RSX_LAUNCH2(u64, DIGV, false);         \
		} else {                                       \
			if (hot)                                   \
				RSX_LAUNCH2(u32, DIGV, true);          \
			else                                       \
				RSX_LAUNCH2(u32, DIGV, false);         \
		}                                              \
	} while (0)
	bool launched = false;
	if constexpr (val_bytes<VT>::value == 0) {
		if (plain) {
			launched = true;
			RSX_LAUNCH2_ST(DIG_PLAIN);
		} else if (integer) {   // signed and / or descending integers: plain digit XOR a per-pass constant
			launched = true;
			RSX_LAUNCH2_ST(DIG_XOR);
		}
	}
	if (!launched)
		RSX_LAUNCH2_ST(DIG_GENERIC);
#undef RSX_LAUNCH2_ST
#undef RSX_LAUNCH2
	HIP_TRY(hipGetLastError());
	if (verify_mode() && dplan && tiles > 0 && !std::is_same<KTO, void>::value && sizeof(KTO) == sizeof(KT)) {
		// a device-scheduled pass (the *_inplace_async sorts): the same check, resolved from the device-side plan like the pass
		// itself; nothing is read back here -- the mismatches add up in a counter of their own until rsx_verify_poll() or the
		// next blocking sort on this stream looks at it
		if (!c.vasync.p) {
			RSX_TRY(c.vasync.ensure(8));
			HIP_TRY(hipMemsetAsync(c.vasync.p, 0, 8, c.stream));
		}
		const u32 vt = (u32)(((u64)(++g_verify_seq) * 2654435761ull) % tiles);
		const u32 kind = (flags & SCATTER_RANK_ASYNC) ? 2u : 1u;
#define RSX_VERIFY_ASYNC(ST)                                                                                            \
		hipLaunchKernelGGL((rsx_verify_tile_kernel<KT, ST>), dim3(1), dim3(64), 0, c.stream, kin, (const void *)kout,         \
		                   (const void *)vin, (const void *)vout, (u64)n, shift, gbase, (const ST *)st, vt, (u32)C2::TILE, ka,  \
		                   (u32)sizeof(KTO), oshift, (u32)val_bytes<VT>::value, 0u, (u64 *)c.vasync.p,                        \
		                   (u32)(env().verify_inject ? 1 : 0), dplan, pass_index, kind, c.pass_alt)
		if (wide)
			RSX_VERIFY_ASYNC(u64);
		else
			RSX_VERIFY_ASYNC(u32);
#undef RSX_VERIFY_ASYNC
		HIP_TRY(hipGetLastError());
	}
	if (verify_mode() && !dplan && tiles > 0) {
		const u32 vt = (u32)(((u64)(++g_verify_seq) * 2654435761ull) % tiles);
		const void *vi = (flags & SCATTER_GEN_INDEX) ? nullptr : (const void *)vin;
#define RSX_VERIFY_TILE(ST)                                                                                             \
		hipLaunchKernelGGL((rsx_verify_tile_kernel<KT, ST>), dim3(1), dim3(64), 0, c.stream, kin, (const void *)kout, vi,       \
		                   (const void *)vout, (u64)n, shift, gbase, (const ST *)st, vt, (u32)C2::TILE, ka, (u32)sizeof(KTO),  \
		                   oshift, (u32)val_bytes<VT>::value, (u32)((flags & SCATTER_SKIP_KEYS) ? 1 : 0), c.verify_bad(),           \
		                   (u32)(env().verify_inject ? 1 : 0))
		if (wide)
			RSX_VERIFY_TILE(u64);
		else
			RSX_VERIFY_TILE(u32);
#undef RSX_VERIFY_TILE
		HIP_TRY(hipGetLastError());
		u64 bad = 0, abad = 0;
		HIP_TRY(hipMemcpyAsync(&bad, c.verify_bad(), sizeof(bad), hipMemcpyDeviceToHost, c.stream));
		if (c.vasync.p)
			HIP_TRY(hipMemcpyAsync(&abad, c.vasync.p, sizeof(abad), hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
		if (abad) {
			HIP_TRY(hipMemsetAsync(c.vasync.p, 0, 8, c.stream));
			return fail(RSX_EVERIFY, "RSX_VERIFY: an earlier device-scheduled sort on this stream (rsx_sort*_inplace_async) had a pass "
			                         "whose checked tile differs from its ballot-ranked re-computation in %llu places",
			            (unsigned long long)abad);
		}
		if (bad)
			return fail(RSX_EVERIFY, "RSX_VERIFY: tile %u of a scatter pass (shift %u, %zu keys) differs from its ballot-ranked "
			                         "re-computation in %llu places: the LDS did not return same-address atomics in lane order",
			            vt, shift, n, (unsigned long long)bad);
	}
	return RSX_OK;
}

// quarter tiles? (default tiles for fewer than about a third of the CUs: 10^6 keys: 31 -> 123 tiles, 108 -> 91 us per sort;
// at 10^7 keys, 305 default tiles, quarter tiles are slower: 204 against 178 us)
template <typename KT, typename VT> bool use_small_tiles(size_t n)
{
	if constexpr (Sc2SmallCfg<KT, VT>::AVAILABLE)
		return n < (size_t)96 * Sc2Cfg<KT, VT>::TILE && !env().no_small_tiles;
	return false;
}

// bytes of status words (ticket included) one pass of the fast kernel takes for n elements
template <typename KT, typename VT> size_t status_bytes(size_t n)
{
	const size_t tile = use_small_tiles<KT, VT>(n) ? (size_t)Sc2SmallCfg<KT, VT>::type::TILE : (size_t)Sc2Cfg<KT, VT>::TILE;
	return 256 + (n + tile - 1) / tile * 256 * (n >= (1ull << 30) ? 8 : 4);
}

template <typename KT, typename VT>
int scatter_pass(Ctx &c, const KT *kin, KT *kout, const VT *vin, VT *vout, size_t n, u32 shift, const u64 *gbase,
                 KdfArgs<KT> ka, u32 flags, const Plan *dplan = nullptr, int region = -1, u32 pass_index = 0)
{
	if ((dplan || region >= 0) && !c.fast)
		return fail(RSX_EINVAL, "speculative pass / status regions without the fast kernel");
	if (c.fast) {
		typedef Sc2Cfg<KT, VT> C2;   // count-first kernel (rsx_scatter2.hpp), 32 Ki-key tiles
		typedef Sc2SmallCfg<KT, VT> Small;
		if constexpr (Small::AVAILABLE) {
			if (use_small_tiles<KT, VT>(n))
				return launch_scatter2<KT, VT, typename Small::type>(c, kin, kout, vin, vout, n, shift, gbase, ka, flags, dplan,
				                                                     region, pass_index);
		}
		return launch_scatter2<KT, VT, C2>(c, kin, kout, vin, vout, n, shift, gbase, ka, flags, dplan, region, pass_index);
	}
	typedef ScatterCfg<KT, VT> C1;   // table-ranked fallback (rsx_kernels.hpp)
	flags &= ~(u32)SCATTER_HOT;      // (its match tables do not care how many lanes share a digit)
	const size_t tile = (size_t)C1::TILE;
	const u64 tiles = (n + tile - 1) / tile;
	const u32 tps = choose_tps(n, tile);
	const u64 stiles = (tiles + tps - 1) / tps;
	const bool wide = n >= (1ull << 30);   // counter width by n, as radix_sort.hpp:102-114 does
	const size_t st_bytes = 256 + stiles * 256 * (wide ? 8 : 4);
	RSX_TRY(c.status.ensure(st_bytes));
	HIP_TRY(hipMemsetAsync(c.status.p, 0, st_bytes, c.stream));
	u32 *ticket = (u32 *)c.status.p;
	void *st = (char *)c.status.p + 256;
	ProfScope prof(1, (u64)n * 2 * (sizeof(KT) + val_bytes<VT>::value), c.stream);
	const dim3 grid((unsigned)stiles);
	if (wide)
		hipLaunchKernelGGL((rsx_scatter_kernel<KT, VT, u64>), grid, dim3(C1::BLOCK), 0, c.stream, kin, kout, vin, vout, (u64)n,
		                   shift, gbase, tps, (u64 *)st, ticket, ka, flags, (u64 *)nullptr);
	else
		hipLaunchKernelGGL((rsx_scatter_kernel<KT, VT, u32>), grid, dim3(C1::BLOCK), 0, c.stream, kin, kout, vin, vout, (u64)n,
		                   shift, gbase, tps, (u32 *)st, ticket, ka, flags, (u64 *)nullptr);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// ---- a rank-sort pass that writes its keys narrowed (fast kernel only; see KTO in rsx_scatter2.hpp) -------------------
template <typename KT, typename VT, typename KTO>
int scatter_pass_narrow(Ctx &c, const KT *kin, KTO *kout, const VT *vin, VT *vout, size_t n, u32 shift, const u64 *gbase,
                        KdfArgs<KT> ka, u32 flags, u32 oshift)
{
	typedef Sc2Cfg<KT, VT> C2;
	typedef Sc2SmallCfg<KT, VT> Small;
	if constexpr (Small::AVAILABLE) {
		if (use_small_tiles<KT, VT>(n))
			return launch_scatter2<KT, VT, typename Small::type, KTO>(c, kin, kout, vin, vout, n, shift, gbase, ka, flags,
			                                                          nullptr, -1, 0, oshift);
	}
	return launch_scatter2<KT, VT, C2, KTO>(c, kin, kout, vin, vout, n, shift, gbase, ka, flags, nullptr, -1, 0, oshift);
}

// keys of `out_bytes` bytes out of a pass over KT keys (out_bytes <= sizeof(KT))
template <typename KT, typename VT>
int scatter_pass_to(Ctx &c, const KT *kin, void *kout, u32 out_bytes, const VT *vin, VT *vout, size_t n, u32 shift,
                    const u64 *gbase, KdfArgs<KT> ka, u32 flags, u32 oshift)
{
	if (out_bytes == sizeof(KT) && oshift == 0)
		return scatter_pass<KT, VT>(c, kin, (KT *)kout, vin, vout, n, shift, gbase, ka, flags);
	if constexpr (sizeof(KT) >= 8)
		if (out_bytes == 8)
			return scatter_pass_narrow<KT, VT, u64>(c, kin, (u64 *)kout, vin, vout, n, shift, gbase, ka, flags, oshift);
	if constexpr (sizeof(KT) >= 4)
		if (out_bytes == 4)
			return scatter_pass_narrow<KT, VT, u32>(c, kin, (u32 *)kout, vin, vout, n, shift, gbase, ka, flags, oshift);
	if constexpr (sizeof(KT) >= 2)
		if (out_bytes == 2)
			return scatter_pass_narrow<KT, VT, uint16_t>(c, kin, (uint16_t *)kout, vin, vout, n, shift, gbase, ka, flags, oshift);
	if (out_bytes == 1)
		return scatter_pass_narrow<KT, VT, uint8_t>(c, kin, (uint8_t *)kout, vin, vout, n, shift, gbase, ka, flags, oshift);
	return fail(RSX_EINVAL, "scatter_pass_to: %u-byte keys out of %zu-byte keys", out_bytes, sizeof(KT));
}

// ---- 8-byte keys by (bit length, mantissa) digits: rsx_logroute.hpp ----------------------------------------------------------
// Tried where the sorts without a histogram do not go (their sample said no, or they are backing off): the route's own sample
// says at once whether it is worth the histogram; everything behind it is device-scheduled and the verdict is read once.
template <typename KT> bool log_wanted(Ctx &c, size_t n, const KT *src, const KT *aux)
{
	if constexpr (sizeof(KT) != 8)
		return false;
	if (env().no_log || !hybrid_enabled() || !c.fast || capture_armed() || verify_mode() || c.small.external || env().no_speculation)
		return false;
	// from 24 Mi keys: Zipf-like keys (BASELINE.json's cfg 3 (iv)) against one pass per kept column, one box, tools/log_sizes.py --
	// 16 Mi 0.49 against 0.43 ms (65536 leaf workgroups are a fixed 0.24 ms), 24 Mi 0.55 against 0.61, 32 Mi 0.63 against 0.78,
	// 64 Mi 0.89 against 1.46, 128 Mi 1.43 against 2.65, 256 Mi 2.46 against 5.09 (profiles/r06/log_sizes.txt)
	const size_t floor_keys = env().log_min_log2 ? (size_t)1 << env().log_min_log2 : (size_t)3 << 23;
	// (up to 2^29 + 2^25 keys: a level-1 bucket must fit 256 leaves -- of 5120 values up to 2^28 + 2^24 keys, of 10240 beyond; the
	// heaviest digits of Zipf-like keys hold 1 / 256 of the array -- and larger arrays would pay for the histogram before the plan
	// kernel says no)
	if (n < floor_keys || n > ((size_t)17 << 25))
		return false;
	if (((((uintptr_t)src) & 15) | (((uintptr_t)aux) & 63)) != 0)   // (16-byte loads of the input, 64-byte atoms into aux)
		return false;
	// an attempt that its sample refuses costs a memset, the sample and eight empty launches -- 65 us, 7 % of a sort of 24 Mi keys --,
	// a lost one the histogram and a pass or two: after either the next 1, 3, 7 .. 31 sorts of the context do not ask
	// (tools/log_overhead.py; rsx_reload_env() forgets, as for the sorts without a histogram)
	blind_refresh(c);
	if (c.log_skip) {
		--c.log_skip;
		return false;
	}
	return true;
}

template <typename KT>
int sort_keys_log(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, KT **result, rsx_info *info, int *done)
{
	*done = 0;
	if constexpr (sizeof(KT) == 8) {
		typedef LogP2Cfg P2;
		const size_t tiles_cap = n / P2::TILE + 257;
		const size_t cur2_off = sizeof(LogCtl), tabs_off = cur2_off + 2 * 65536 * sizeof(u32);
		const size_t tiles_off = (tabs_off + sizeof(LogTabs) + 255) & ~(size_t)255;
		const size_t zero_bytes = tabs_off + offsetof(LogTabs, offs_small);
		const size_t l2_cap = n + n / 8 + (size_t)65536 * 700;   // level-2 slots: values (rsx_log_plan_kernel checks the exact sum)
		if (c.logb.ensure(tiles_off + tiles_cap * sizeof(LogTile)) != RSX_OK ||
		    c.logslots.ensure((l2_cap + P2::TILE + 64) * sizeof(u32)) != RSX_OK) {
			(void)hipGetLastError();
			return RSX_OK;   // (no room: the ordinary path)
		}
		if (!c.host_logctl)
			HIP_TRY(hipHostMalloc((void **)&c.host_logctl, sizeof(LogCtl), hipHostMallocDefault));
		if (!c.log_ev)
			HIP_TRY(hipEventCreateWithFlags(&c.log_ev, hipEventDisableTiming));
		LogCtl *ctl = (LogCtl *)c.logb.p;
		u32 *cur2 = (u32 *)((char *)c.logb.p + cur2_off);
		LogTabs *tabs = (LogTabs *)((char *)c.logb.p + tabs_off);
		LogTile *tiles = (LogTile *)((char *)c.logb.p + tiles_off);
		u32 *slots = (u32 *)c.logslots.p;
		const size_t pmark = prof_mark();
		HIP_TRY(hipMemsetAsync(c.logb.p, 0, zero_bytes, c.stream));
		// the leaves' shape: 5120 values per slot (five workgroups of 256 threads per CU) up to 2^28 + 2^24 keys, 10240 beyond
		const bool big_leaves = n > ((size_t)17 << 24) || env().log_leaf_big;
		hipLaunchKernelGGL((rsx_log_sample_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, (const KT *)src, (u64)n, ka, ctl,
		                   big_leaves ? LOG_LEAF_CAP_BIG : LOG_LEAF_CAP);
		{
			ProfScope prof(0, (u64)n * sizeof(KT), c.stream);
			hipLaunchKernelGGL((rsx_log_hist_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, (const KT *)src, (u64)n, ka, ctl, tabs);
		}
		hipLaunchKernelGGL(rsx_log_plan_kernel, dim3(1), dim3(1024), 0, c.stream, ctl, tabs, tiles, (u64)n, (u32)n, (u32)l2_cap,
		                   (u32)tiles_cap, (u32)P2::TILE, (u32)P2::GRID, (Plan *)nullptr, c.dev_host_plan);
		{
			ProfScope prof(1, 0, c.stream);
			hipLaunchKernelGGL((rsx_log_pass1_kernel<KT>), dim3(256), dim3(LogP1Cfg::BLOCK), 0, c.stream, (const KT *)src, (u64)n, aux,
			                   ctl, tabs, ka);
		}
		{
			ProfScope prof(3, 0, c.stream);
			hipLaunchKernelGGL((rsx_log_pass2_kernel<KT>), dim3(P2::GRID), dim3(P2::BLOCK), 0, c.stream, (const KT *)aux, slots,
			                   (const LogTile *)tiles, ctl, (const LogTabs *)tabs, cur2, (u32)l2_cap, ka);
		}
		{
			ProfScope prof(2, 0, c.stream);
			hipLaunchKernelGGL((rsx_log_fill_kernel<KT>), dim3(2048), dim3(LOG_FILL_BLOCK), 0, c.stream, src, aux, (const LogCtl *)ctl,
			                   (const LogTabs *)tabs, ka);
			if (big_leaves)
				hipLaunchKernelGGL((rsx_log_leaf_kernel<KT, LogLeafCfgBig>), dim3(65536), dim3(LogLeafCfgBig::BLOCK), 0, c.stream, src, aux,
				                   (const u32 *)slots, (const LogCtl *)ctl, (const LogTabs *)tabs, (const u32 *)cur2, ka, 0u, 256u);
			else
				hipLaunchKernelGGL((rsx_log_leaf_kernel<KT, LogLeafCfg>), dim3(65536), dim3(LogLeafCfg::BLOCK), 0, c.stream, src, aux,
				                   (const u32 *)slots, (const LogCtl *)ctl, (const LogTabs *)tabs, (const u32 *)cur2, ka, 0u, 256u);
		}
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(c.host_logctl, ctl, sizeof(LogCtl), hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipEventRecord(c.log_ev, c.stream));
		HIP_TRY(hipEventSynchronize(c.log_ev));
		const LogCtl h = *c.host_logctl;
		if (!h.go || h.fail || (!h.ok && !h.sorted)) {
			prof_called_off(pmark, c.stream);   // (not this route's keys, or an attempt that was lost: the ordinary path)
			c.log_backoff = std::min<u32>(2 * c.log_backoff + 1, 31);
			c.log_skip = c.log_backoff;
			return RSX_OK;
		}
		c.log_backoff = 0;
		const Plan plan = *c.host_plan;
		info_from_plan(info, plan);
		*done = 1;
		if (h.sorted) {   // radix_sort.hpp:60-62
			prof_called_off(pmark, c.stream, 1);
			prof_called_off(pmark, c.stream, 2);
			prof_called_off(pmark, c.stream, 3);
			if (info) {
				info->early_exit = 2;
				info->ncols = 0;
			}
			*result = src;
			return RSX_OK;
		}
		const u64 nsmall = h.nsmall, nbig = n - nsmall;
		prof_rebook(pmark, c.stream, 1, (u64)n * sizeof(KT) + nbig * sizeof(KT));
		prof_rebook(pmark, c.stream, 3, nbig * (sizeof(KT) + 4));
		prof_rebook(pmark, c.stream, 2, nbig * (4 + sizeof(KT)) + nsmall * sizeof(KT));
		KT *final = (plan.ncols & 1) ? aux : src;   // radix_sort.hpp:92
		*result = final;
		if (info) {
			info->result_in_aux = final == aux;
			info->hybrid = 6u;
		}
	}
	return RSX_OK;
}

// ---- keys only -------------------------------------------------------------------
template <typename KT>
int sort_keys_device_impl(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void **result, rsx_info *info);

// RSX_VERIFY=2: the sort as it always runs (speculation, leaves, slack slots ...), bracketed by rsx_checksum_kernel on the
// input and on the result: not sorted, or not the same keys -> RSX_EVERIFY.  (RSX_VERIFY=1 re-ranks a tile of every PASS and
// therefore keeps to the pass kernels; this one is blind to where an error came from but covers every route.)
template <typename KT>
int sort_keys_device(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void **result, rsx_info *info)
{
	if (!env().verify_whole)
		return sort_keys_device_impl<KT>(c, src, aux, n, dtype, order, result, info);
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	RSX_TRY(c.vsum.ensure(6 * sizeof(u64)));
	u64 *vs = (u64 *)c.vsum.p;
	HIP_TRY(hipMemsetAsync(vs, 0, 6 * sizeof(u64), c.stream));
	hipLaunchKernelGGL((rsx_checksum_kernel<KT>), dim3(2048), dim3(256), 0, c.stream, (const KT *)src, (u64)n, ka, vs);
	HIP_TRY(hipGetLastError());
	RSX_TRY(sort_keys_device_impl<KT>(c, src, aux, n, dtype, order, result, info));
	hipLaunchKernelGGL((rsx_checksum_kernel<KT>), dim3(2048), dim3(256), 0, c.stream, (const KT *)*result, (u64)n, ka, vs + 3);
	HIP_TRY(hipGetLastError());
	u64 h[6];
	HIP_TRY(hipMemcpyAsync(h, vs, sizeof h, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	if (env().verify_inject)   // (test hook: the failure report end to end)
		h[5] ^= 1;
	if (h[3] != 0 || h[1] != h[4] || h[2] != h[5])
		return fail(RSX_EVERIFY, "RSX_VERIFY=2: the result of a sort of %zu keys (route %u) is %s: %llu descents, key sum %s, key mix %s",
		            n, info ? info->hybrid : 0u, h[3] ? "not sorted" : "not a permutation of the input", (unsigned long long)h[3],
		            h[1] == h[4] ? "kept" : "changed", h[2] == h[5] ? "kept" : "changed");
	return RSX_OK;
}

template <typename KT>
int sort_keys_device_impl(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void **result, rsx_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (c.fast && n * sizeof(KT) <= SMALL_SORT_BYTES && !env().no_small_sort && !capture_armed()) {
		// the whole sort in one workgroup and one launch (rsx_small.hpp)
		ProfScope prof(1, (u64)n * 2 * sizeof(KT), c.stream);
		hipLaunchKernelGGL((rsx_small_sort_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, src, aux, (u32)n, ka, c.dev_host_plan);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(c.stream));
		const Plan p = *c.host_plan;
		info_from_plan(info, p);
		if (info && p.sorted)
			info->early_exit = 2;
		*result = (p.ncols & 1) ? aux : src;     // radix_sort.hpp:92 (sorted input: no column, src)
		if (info)
			info->result_in_aux = *result == aux;
		return RSX_OK;
	}
	Plan plan;
	if constexpr (sizeof(KT) == 1) {
		// 1-byte keys: at most one column, so the sorted array is the histogram written out (rsx_fill_runs_kernel) -- a read
		// and a write of the keys instead of a read, a read and a scatter
		if (!env().no_fill_runs && (((uintptr_t)aux) & 15) == 0) {
			RSX_TRY(plan_phase<KT>(c, src, n, ka, nullptr, 0));
			const unsigned blocks = (unsigned)std::min<u64>((n / 16 + 255) / 256 + 1, 8192);
			hipLaunchKernelGGL((rsx_fill_runs_kernel<KT>), dim3(blocks), dim3(256), 0, c.stream, aux, (u64)n, (const u64 *)c.ghist(),
			                   (const KT *)src, ka, (const Plan *)c.plan());
			HIP_TRY(hipGetLastError());
			RSX_TRY(plan_wait(c, &plan));
			info_from_plan(info, plan);
			RSX_TRY(capture_hist(c, n, sizeof(KT)));
			if (plan.sorted)                     // radix_sort.hpp:60-62
				return finish_sorted(info, result, src);
			*result = aux;                       // one pass: radix_sort.hpp:92
			if (info)
				info->result_in_aux = 1;
			return RSX_OK;
		}
	}
	if constexpr (sizeof(KT) >= 4) {
		// large arrays: two MSB passes and leaves without the histogram, where a sample of the keys allows it (rsx_hybrid.hpp)
		if (blind_wanted<KT>(c, n)) {
			int done = 0;
			KT *res = nullptr;
			RSX_TRY(sort_keys_blind<KT>(c, src, aux, n, ka, &res, info, &done));
			if (done) {
				*result = res;
				return RSX_OK;
			}
		}
	}
	if constexpr (sizeof(KT) == 8) {
		// 8-byte keys the byte columns do not spread (heavy-tailed magnitudes): digits of (bit length, mantissa), rsx_logroute.hpp
		if (log_wanted<KT>(c, n, src, aux)) {
			int done = 0;
			KT *res = nullptr;
			RSX_TRY(sort_keys_log<KT>(c, src, aux, n, ka, &res, info, &done));
			if (done) {
				*result = res;
				return RSX_OK;
			}
		}
	}
	// The first pass is enqueued before the host knows the plan (it reads the device's copy and does nothing on
	// sorted input): the host's wait for the plan, 20-25 us of idle GPU otherwise, hides behind it.
	const bool spec = c.fast && !env().no_speculation && !verify_mode();
	// with the fast kernel every pass has its own region of status words, all zeroed together with the histogram
	const size_t status_total = c.fast ? status_bytes<KT, NoVal>(n) * sizeof(KT) : 0;
	if constexpr (sizeof(KT) == 2) {
		// 2-byte keys, large arrays: one 16-bit digit.  The sorted array is written from the joint histogram of the two bytes
		// (rsx_joint16_kernel ... rsx_fill16_kernel) into `src` -- where two passes end (radix_sort.hpp:92) --, from one
		// byte's histogram into `aux` if only one column is kept; the device-side plan decides, no kernel scatters.
		// (below 2^32 keys: the joint table counts in 32 bits, and one 16-bit value may occur n times; larger arrays take the
		// two scatter passes, whose status words are 64-bit from 2^30 keys on -- counter width by n, radix_sort.hpp:102-114)
		if (!env().no_fill_runs && n >= ((size_t)1 << 20) && n < ((size_t)1 << 32) && ((((uintptr_t)aux) | ((uintptr_t)src)) & 15) == 0) {
			RSX_TRY(c.joint.ensure(65536 * sizeof(u32) + 65537 * sizeof(u64) + 8));
			u32 *jt = (u32 *)c.joint.p;
			u64 *offs = (u64 *)((char *)c.joint.p + 65536 * sizeof(u32));
			HIP_TRY(hipMemsetAsync(jt, 0, 65536 * sizeof(u32), c.stream));
			RSX_TRY(plan_phase<KT>(c, src, n, ka, nullptr, 0));
			hipLaunchKernelGGL(rsx_joint16_kernel, dim3(512), dim3(1024), 0, c.stream, (const uint16_t *)src, (u64)n, ka, jt,
			                   (const Plan *)c.plan());
			hipLaunchKernelGGL(rsx_joint16_scan_kernel, dim3(1), dim3(1024), 0, c.stream, (const u32 *)jt, offs, (u64)n,
			                   (const Plan *)c.plan());
			const unsigned blocks = (unsigned)std::min<u64>((n / 8 + 255) / 256 + 1, 8192);
			hipLaunchKernelGGL(rsx_fill16_kernel, dim3(blocks), dim3(256), 0, c.stream, (uint16_t *)src, (u64)n, (const u64 *)offs, ka,
			                   (const Plan *)c.plan());
			hipLaunchKernelGGL((rsx_fill_runs_kernel<KT>), dim3(blocks), dim3(256), 0, c.stream, aux, (u64)n, (const u64 *)c.ghist(),
			                   (const KT *)src, ka, (const Plan *)c.plan());
			HIP_TRY(hipGetLastError());
			RSX_TRY(plan_wait(c, &plan));
			info_from_plan(info, plan);
			RSX_TRY(capture_hist(c, n, sizeof(KT)));
			if (plan.sorted)                     // radix_sort.hpp:60-62
				return finish_sorted(info, result, src);
			*result = plan.ncols == 1 ? aux : src;
			if (info)
				info->result_in_aux = plan.ncols == 1;
			return RSX_OK;
		}
	}
	// One kept column (keys that differ in one byte only): the sorted array is written from the histogram instead of
	// scattered (rsx_fill_runs_kernel).  With a speculative first pass both kernels are enqueued and the device-side plan
	// decides which of them works, which costs an empty launch (3 us) in the usual case: only from 16 Mi keys on, where that is 1 %.
	const bool fill_one = sizeof(KT) > 1 && !env().no_fill_runs && (((uintptr_t)aux) & 15) == 0 && (!spec || n >= ((size_t)1 << 24));
	auto launch_fill = [&]() {
		const unsigned blocks = (unsigned)std::min<u64>((n * sizeof(KT) / 16 + 255) / 256 + 1, 8192);
		hipLaunchKernelGGL((rsx_fill_runs_kernel<KT>), dim3(blocks), dim3(256), 0, c.stream, aux, (u64)n, (const u64 *)c.ghist(),
		                   (const KT *)src, ka, (const Plan *)c.plan());
		return hipGetLastError();
	};
	u32 spec_leaves = 0;
	bool self_planned = false;
	const size_t pmark = prof_mark();
	if (spec) {
		// (the device may choose one MSB pass and leaves, rsx_hybrid.hpp: pass 0 then goes by the highest kept column)
		const HybCaps caps = capture_armed() ? HybCaps{0, 0, 0, 0} : hybrid_caps<KT>(n);
		// Mid-size arrays: pass 0 derives the plan itself (SCATTER_SELF_PLAN, rsx_scatter2.hpp) -- no plan launch.  (Not
		// with a caller's histogram: its counts are read back from the scanned offsets a plan kernel leaves.)
		self_planned = sizeof(KT) >= 4 && caps.cap1 != 0 && n <= ((size_t)1 << 23) && !fill_one && !env().no_self_plan;
		RSX_TRY(plan_phase<KT>(c, src, n, ka, nullptr, status_total, caps, true, &self_planned));
		u32 flags0 = fill_one ? (u32)SCATTER_ONE_COL_FILLED : 0u;
		if (self_planned) {
			flags0 |= SCATTER_SELF_PLAN;
			c.pass_sp = SelfPlanArgs{(const u32 *)c.unsorted(), c.plan(), c.dev_host_plan, (u64 *)c.gscan.p, caps};
		}
		const int rc0 = scatter_pass<KT, NoVal>(c, src, aux, nullptr, nullptr, n, 0, c.ghist(), ka, flags0, c.plan(), 0);
		c.pass_sp = SelfPlanArgs{nullptr, nullptr, nullptr, nullptr, HybCaps{0, 0, 0, 0}};
		RSX_TRY(rc0);
		if (self_planned) {   // the plan is pass 0's workgroup 0's now
			if (!c.plan_ev)
				HIP_TRY(hipEventCreateWithFlags(&c.plan_ev, hipEventDisableTiming));
			HIP_TRY(hipEventRecord(c.plan_ev, c.stream));
		}
		if (fill_one)
			HIP_TRY(launch_fill());
		if constexpr (sizeof(KT) >= 4) {
			// one MSB pass and leaves, if the device-side plan says so: enqueued now, so that nothing waits for the host
			// (the large shape only where even spread keys would come near the small one's capacity; else after the wait)
			if (caps.cap1 && n <= (size_t)256 * caps.cap1) {
				spec_leaves = n / 256 > (size_t)LeafShapes<KT>::Small::CAP / 2 ? (LeafShapes<KT>::HAS_MEDIUM ? 7u : 3u) : 1u;
				RSX_TRY(launch_leaves<KT>(c, src, aux, n, ka, HYB_ONE_LEVEL, spec_leaves, self_planned ? (const u64 *)c.gscan.p : nullptr));
			}
		}
		RSX_TRY(plan_wait(c, &plan));
	} else {
		RSX_TRY(plan_phase<KT>(c, src, n, ka, &plan, status_total));
	}
	info_from_plan(info, plan);
	RSX_TRY(capture_hist(c, n, sizeof(KT)));
	// (the profile books what the device chose: leaves enqueued for a plan that did not come, a pass 0 that found the input sorted)
	if (spec_leaves && (plan.sorted || plan.hyb != HYB_ONE_LEVEL))
		prof_called_off(pmark, c.stream, 2);
	if (spec && plan.sorted)
		prof_called_off(pmark, c.stream, 1);
	if (plan.sorted)                         // radix_sort.hpp:60-62
		return finish_sorted(info, result, src);
	if (fill_one && plan.ncols == 1) {
		if (!spec)
			HIP_TRY(launch_fill());
		*result = aux;                       // one pass: radix_sort.hpp:92
		if (info)
			info->result_in_aux = 1;
		return RSX_OK;
	}
	if constexpr (sizeof(KT) >= 4) {
		if (plan.hyb == HYB_ONE_LEVEL || plan.hyb == HYB_TWO_LEVEL) {
			// pass 0 went by the highest kept column; the leaves put the result where an LSB-first sort of plan.ncols passes ends
			KT *final = (plan.ncols & 1) ? aux : src;
			u32 how = 1;
			if (plan.hyb == HYB_TWO_LEVEL) {
				RSX_TRY(sort_keys_two_level<KT>(c, src, aux, n, ka, plan, &final, &how));
			} else {
				// one level: the leaves are on their way, unless they need a shape that was not enqueued
				const u32 need = LeafShapes<KT>::shape_for(plan.max1);
				if (!(spec_leaves & need))
					RSX_TRY(launch_leaves<KT>(c, src, aux, n, ka, HYB_ONE_LEVEL, need, self_planned ? (const u64 *)c.gscan.p : nullptr));
			}
			*result = final;                     // radix_sort.hpp:92
			if (info) {
				info->result_in_aux = final == aux;
				info->hybrid = how;
			}
			return RSX_OK;
		}
	}
	if (self_planned && plan.ncols > 1) {
		// one pass per kept column after a self-planned pass 0: the other columns' scans (and the hot digits) are made now
		hipLaunchKernelGGL((rsx_plan_all_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, (const KT *)src, (u64)n, c.ghist(), ka, c.kept(),
		                   c.hotd(), (const u32 *)c.unsorted(), c.plan(), c.dev_host_plan, HybCaps{0, 0, 0, 0});
		HIP_TRY(hipGetLastError());
	}
	KT *cur = src, *oth = aux;
	if (spec)
		std::swap(cur, oth);                 // pass 0 is on its way
	for (u32 i = spec ? 1 : 0; i < plan.ncols; ++i) {   // radix_sort.hpp:83-90
		const u32 col = plan.cols[i];
		RSX_TRY((scatter_pass<KT, NoVal>(c, cur, oth, nullptr, nullptr, n, 8 * col, c.ghist() + 256 * col, ka,
		                                 hot_flags(plan.hot, col), nullptr, c.fast ? (int)i : -1)));
		std::swap(cur, oth);
	}
	*result = cur;                           // radix_sort.hpp:92
	if (info)
		info->result_in_aux = cur == aux;
	return RSX_OK;
}

// ---- keys only, no host synchronisation: every pass is device-scheduled, the result always ends in `buf` ------------
template <typename KT>
int sort_keys_inplace_async(Ctx &c, KT *buf, KT *scratch, size_t n, int dtype, int order)
{
	if (!c.fast)
		return fail(RSX_EHIP, "rsx_sort_inplace_async needs the fast scatter kernel (the device self-check failed on this device)");
	c.async_tried_blind = false;   // (rsx_async_route reports THIS call: set again below if an attempt is enqueued)
	c.async_small = false;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (n * sizeof(KT) <= SMALL_SORT_BYTES) {
		hipLaunchKernelGGL((rsx_small_sort_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, buf, scratch, (u32)n, ka, c.dev_host_plan, true);
		HIP_TRY(hipGetLastError());
		c.async_small = true;
		return RSX_OK;
	}
	const size_t status_total = status_bytes<KT, NoVal>(n) * sizeof(KT);
	// The routes of the blocking sort (rsx_hybrid.hpp), chosen on the device with nobody to read a verdict back:
	//  * arrays the sort without a histogram is for: the whole attempt is enqueued first -- sample, two MSB passes
	//    into slots, leaves -- and what follows (histogram, plan, one pass per kept column) looks at the attempt's verdict,
	//    SegCtl::mode, and does nothing if the keys are sorted by then; an attempt that is called off has only read `buf`.
	//    (The host never learns how an attempt went: a context's back-off after a LOST attempt -- one that passed the sample and
	//    then overflowed a slot -- is kept on the device, SegCtl::boff_skip.  An attempt the sample turns away costs a sample kernel
	//    and a few empty launches, one that goes through the empty launches of the histogram-first kernels.)
	//  * mid-size arrays: one MSB pass and leaves where the device-side plan says so (Plan::hyb) -- pass 0 then goes by the
	//    highest kept column, the leaf launches behind it do nothing otherwise, and the passes 1 .. do nothing if they do.
	// A caller-owned workspace (rsx_sort_inplace_async_ws) makes the attempt if it was sized for the slots (rsx_workspace_bytes_fast).
	HybCaps caps{0, 0, 0, 0};
	int blind = 0;
	ProfAsyncVerdict pverdict(c.stream);   // (rsx_profile books what the device chose: the attempt's launches or the ones behind it)
	if constexpr (sizeof(KT) >= 4) {
		if (hybrid_enabled() && !verify_mode() && !env().no_speculation) {
			caps = hybrid_caps<KT>(n);
			caps.cap2 = caps.min_cols2 = 0;
			if (async_blind_ok<KT>(c, n))
				RSX_TRY(blind_enqueue<KT>(c, buf, scratch, n, ka, &blind));
		}
	}
	if (blind)
		pverdict.attempt_enqueued(SegView(c).ctl());
	c.pass_gate = blind ? SegView(c).ctl() : nullptr;
	c.async_tried_blind = blind != 0;
	int rc = plan_phase<KT>(c, buf, n, ka, nullptr, status_total, caps);
	for (u32 i = 0; i < sizeof(KT) && rc == RSX_OK; ++i)   // pass i = the i-th kept column, if there is one (radix_sort.hpp:83-90)
		rc = scatter_pass<KT, NoVal>(c, buf, scratch, nullptr, nullptr, n, 0, c.ghist(), ka, 0, c.plan(), (int)i, i);
	c.pass_gate = nullptr;
	RSX_TRY(rc);
	if constexpr (sizeof(KT) >= 4) {
		if (caps.cap1 && n <= (size_t)256 * caps.cap1) {
			// (every shape: which one the largest bucket needs is only known on the device, and each does nothing unless the
			// plan's largest bucket is its size -- keys with 64 values in their top byte fill buckets four times the mean)
			const u32 shapes = LeafShapes<KT>::HAS_MEDIUM ? 7u : 3u;
			RSX_TRY(launch_leaves<KT>(c, buf, scratch, n, ka, HYB_ONE_LEVEL, shapes));
		}
	}
	pverdict.gated_enqueued();
	// an odd number of kept columns leaves the result in `scratch` (radix_sort.hpp:92): bring it home
	hipLaunchKernelGGL(rsx_copy_if_odd_kernel, dim3(2048), dim3(256), 0, c.stream, (unsigned char *)buf, (const unsigned char *)scratch,
	                   (u64)n * sizeof(KT), (const Plan *)c.plan());
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// ---- key + payload, no host synchronisation: as sort_keys_inplace_async, the result always in (k, v) -----------------------
template <typename KT, typename VT>
int sort_pairs_inplace_async(Ctx &c, KT *k, KT *ks, VT *v, VT *vs, size_t n, int dtype, int order)
{
	if (!c.fast)
		return fail(RSX_EHIP, "rsx_sort_pairs_inplace_async needs the fast scatter kernel (the device self-check failed on this device)");
	c.async_tried_blind = false;   // (rsx_async_route reports THIS call: set again below if an attempt is enqueued)
	c.async_small = false;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (n * 2 * (sizeof(KT) + sizeof(VT)) <= SMALL_PAIR_BYTES) {
		hipLaunchKernelGGL((rsx_small_pairs_kernel<KT, VT, false>), dim3(1), dim3(1024), 0, c.stream, (const KT *)k, ks, v, vs, (u32)n,
		                   ka, c.dev_host_plan, true);
		HIP_TRY(hipGetLastError());
		c.async_small = true;
		return RSX_OK;
	}
	const size_t status_total = status_bytes<KT, VT>(n) * sizeof(KT);
	// as sort_keys_inplace_async: the attempt without a histogram first (4-byte keys and payloads, 16 Mi .. 2^28 pairs: two MSB
	// passes into slots and the pairs' leaves, which write (k, v) -- an attempt that is called off has only read them), the
	// histogram-first kernels behind it gated on its verdict
	int blind = 0;
	ProfAsyncVerdict pverdict(c.stream);
	if constexpr (sizeof(KT) == 4 && sizeof(VT) == 4) {
		if (async_pairs_blind_ok<KT>(c, n, sizeof(VT)))
			RSX_TRY((pairs_blind_enqueue<KT, VT>(c, k, v, k, v, n, ka, &blind, ks, vs)));
	}
	if (blind)
		pverdict.attempt_enqueued(SegView(c).ctl());
	c.pass_gate = blind ? SegView(c).ctl() : nullptr;
	c.async_tried_blind = blind != 0;
	int rc = plan_phase<KT>(c, k, n, ka, nullptr, status_total);
	for (u32 i = 0; i < sizeof(KT) && rc == RSX_OK; ++i)
		rc = scatter_pass<KT, VT>(c, k, ks, v, vs, n, 0, c.ghist(), ka, 0, c.plan(), (int)i, i);
	c.pass_gate = nullptr;
	RSX_TRY(rc);
	pverdict.gated_enqueued();
	hipLaunchKernelGGL(rsx_copy_if_odd_kernel, dim3(2048), dim3(256), 0, c.stream, (unsigned char *)k, (const unsigned char *)ks,
	                   (u64)n * sizeof(KT), (const Plan *)c.plan());
	hipLaunchKernelGGL(rsx_copy_if_odd_kernel, dim3(2048), dim3(256), 0, c.stream, (unsigned char *)v, (const unsigned char *)vs,
	                   (u64)n * sizeof(VT), (const Plan *)c.plan());
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// ---- key + payload -----------------------------------------------------------------
template <typename KT, typename VT>
int sort_pairs_device_impl(Ctx &c, KT *k0, KT *k1, VT *v0, VT *v1, size_t n, int dtype, int order, rsx_info *info);

// RSX_VERIFY=2 (as for keys-only sorts): the sort on its usual route, bracketed by checksums of the PAIRS: the result's keys
// must not descend and its key sum and pair mix must be the input's.
template <typename KT, typename VT>
int sort_pairs_device(Ctx &c, KT *k0, KT *k1, VT *v0, VT *v1, size_t n, int dtype, int order, rsx_info *info)
{
	if (!env().verify_whole)
		return sort_pairs_device_impl<KT, VT>(c, k0, k1, v0, v1, n, dtype, order, info);
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	RSX_TRY(c.vsum.ensure(6 * sizeof(u64)));
	u64 *vs = (u64 *)c.vsum.p;
	HIP_TRY(hipMemsetAsync(vs, 0, 6 * sizeof(u64), c.stream));
	hipLaunchKernelGGL((rsx_checksum_pairs_kernel<KT, VT>), dim3(2048), dim3(256), 0, c.stream, (const KT *)k0, (const VT *)v0, (u64)n, ka, vs);
	HIP_TRY(hipGetLastError());
	rsx_info local;
	memset(&local, 0, sizeof(local));
	rsx_info *inf = info ? info : &local;
	RSX_TRY((sort_pairs_device_impl<KT, VT>(c, k0, k1, v0, v1, n, dtype, order, inf)));
	const KT *kr = inf->result_in_aux ? k1 : k0;
	const VT *vr = inf->result_in_aux ? v1 : v0;
	hipLaunchKernelGGL((rsx_checksum_pairs_kernel<KT, VT>), dim3(2048), dim3(256), 0, c.stream, kr, vr, (u64)n, ka, vs + 3);
	HIP_TRY(hipGetLastError());
	u64 h[6];
	HIP_TRY(hipMemcpyAsync(h, vs, sizeof h, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	if (env().verify_inject)
		h[5] ^= 1;
	if (h[3] != 0 || h[1] != h[4] || h[2] != h[5])
		return fail(RSX_EVERIFY, "RSX_VERIFY=2: the result of a key + payload sort of %zu pairs (route %u) is %s: %llu descents, key sum %s, pair mix %s",
		            n, inf->hybrid, h[3] ? "not sorted" : "not a permutation of the input's pairs", (unsigned long long)h[3],
		            h[1] == h[4] ? "kept" : "changed", h[2] == h[5] ? "kept" : "changed");
	return RSX_OK;
}

template <typename KT, typename VT>
int sort_pairs_device_impl(Ctx &c, KT *k0, KT *k1, VT *v0, VT *v1, size_t n, int dtype, int order, rsx_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (c.fast && n * 2 * (sizeof(KT) + sizeof(VT)) <= SMALL_PAIR_BYTES && !env().no_small_sort && !capture_armed()) {
		ProfScope prof(1, (u64)n * 2 * (sizeof(KT) + sizeof(VT)), c.stream);
		hipLaunchKernelGGL((rsx_small_pairs_kernel<KT, VT, false>), dim3(1), dim3(1024), 0, c.stream, (const KT *)k0, k1, v0, v1,
		                   (u32)n, ka, c.dev_host_plan);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(c.stream));
		const Plan p = *c.host_plan;
		info_from_plan(info, p);
		if (info) {
			info->early_exit = p.sorted ? 2 : 0;
			info->result_in_aux = p.ncols & 1;
		}
		return RSX_OK;
	}
	if constexpr (sizeof(KT) == 4 && sizeof(VT) == 4) {
		if (blind_wanted<KT>(c, n, sizeof(VT))) {
			// all sizeof(KT) columns kept (pairs_blind: the sample proves it): the result lies where an even number of passes ends
			int done = 0;
			RSX_TRY((pairs_blind<KT, VT>(c, k0, v0, k0, v0, n, ka, info, &done, k1, v1)));
			if (done) {
				if (info)
					info->result_in_aux = 0;
				return RSX_OK;
			}
		}
	}
	Plan plan;
	RSX_TRY(plan_phase<KT>(c, k0, n, ka, &plan, 0, (c.fast && !capture_armed() && !verify_mode()) ? hybrid_caps_pairs<KT>(n, sizeof(VT), true) : HybCaps{0, 0, 0, 0}));
	info_from_plan(info, plan);
	RSX_TRY(capture_hist(c, n, sizeof(KT)));
	if (plan.sorted)
		return finish_sorted(info);
	if constexpr (sizeof(KT) == 4 && sizeof(VT) == 4) {
		if (plan.hyb == HYB_ONE_LEVEL) {
			// one MSB pass and the pairs' leaves (mid-size arrays)
			const u32 top = plan.cols[plan.ncols - 1];
			RSX_TRY((scatter_pass<KT, VT>(c, k0, k1, v0, v1, n, 8 * top, c.ghist() + 256 * top, ka, 0u)));
			const bool in_aux = (plan.ncols & 1) != 0;
			RSX_TRY((pairs_one_level<KT, VT>(c, k1, v1, in_aux ? k1 : k0, in_aux ? v1 : v0, n, ka)));
			if (info) {
				info->result_in_aux = in_aux;
				info->hybrid = 1;
			}
			return RSX_OK;
		}
		if (plan.hyb == HYB_TWO_LEVEL) {
			// two MSB passes (the second into slots) and leaves; on a slot's overflow: one pass per column, from (k0, v0) again
			// (RSX_NO_SLACK=1: the second pass counted first and written to (k0, v0), which pass 1 has read; a bucket too large
			// for the leaves is known before that pass)
			const u32 top = plan.cols[plan.ncols - 1];
			RSX_TRY((scatter_pass<KT, VT>(c, k0, k1, v0, v1, n, 8 * top, c.ghist() + 256 * top, ka, 0u)));
			const bool in_aux = (plan.ncols & 1) != 0;
			bool ok = false;
			RSX_TRY((pairs_two_level<KT, VT>(c, k1, v1, in_aux ? k1 : k0, in_aux ? v1 : v0, n, ka, &ok, k0, v0)));
			if (ok) {
				if (info) {
					info->result_in_aux = in_aux;
					info->hybrid = env().no_slack ? 2 : 4;
				}
				return RSX_OK;
			}
		}
	}
	KT *kc = k0, *ko = k1;
	VT *vc = v0, *vo = v1;
	for (u32 i = 0; i < plan.ncols; ++i) {
		const u32 col = plan.cols[i];
		RSX_TRY((scatter_pass<KT, VT>(c, kc, ko, vc, vo, n, 8 * col, c.ghist() + 256 * col, ka, hot_flags(plan.hot, col))));
		std::swap(kc, ko);
		std::swap(vc, vo);
	}
	if (info)
		info->result_in_aux = kc == k1;
	return RSX_OK;
}

// ---- rank (stable argsort) ----------------------------------------------------------
// index halves H0 = ib, H1 = ib + n ping-pong exactly as radix_sort_rank.hpp:77-89;
// the keys travel with the indices through two workspace
// buffers instead of being gathered through the index as Listing 6 does.
// (a key type no wider than KT: keeps the instantiations of impossible combinations out of the build)
template <typename KT, typename N> using NarrowerOr = typename std::conditional<(sizeof(N) < sizeof(KT)), N, KT>::type;

// one pass of a rank sort over keys currently held as KCUR (the raw KT keys until the first narrowing, KDF-applied after)
template <typename KCUR, typename KT, typename IT>
int rank_pass(Ctx &c, const void *kin, void *kout, u32 out_bytes, const IT *vin, IT *vout, size_t n, u32 shift, const u64 *gbase,
              const KdfArgs<KT> &ka0, bool applied, u32 flags, u32 oshift)
{
	KdfArgs<KCUR> ka{0, 0, 0};
	if constexpr (std::is_same<KCUR, KT>::value)
		if (!applied)
			ka = ka0;
	return scatter_pass_to<KCUR, IT>(c, (const KCUR *)kin, kout, out_bytes, vin, vout, n, shift, gbase, ka, flags, oshift);
}

// want_half: -1 = the half the number of kept columns dictates (radix_sort_rank.hpp:91); 0 / 1 = leave the ranks in that half
// whatever the number of passes is (the first pass generates its indices, so it can write to either half).
template <typename KT, typename IT>
int sort_rank_device_impl(Ctx &c, const KT *src, IT *ib, size_t n, int dtype, int order, void **result, rsx_info *info, int want_half);

// RSX_VERIFY=2: the ranks must be a permutation of 0 .. n-1 (sum and mix) through which the keys do not descend, equal keys in
// index order (radix_sort_rank.hpp:82-90: stable) -- checked on the device, whatever route the sort took.
template <typename KT, typename IT>
int sort_rank_device(Ctx &c, const KT *src, IT *ib, size_t n, int dtype, int order, void **result, rsx_info *info, int want_half = -1)
{
	RSX_TRY((sort_rank_device_impl<KT, IT>(c, src, ib, n, dtype, order, result, info, want_half)));
	if (!env().verify_whole || n < 2)
		return RSX_OK;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	RSX_TRY(c.vsum.ensure(6 * sizeof(u64)));
	u64 *vs = (u64 *)c.vsum.p;
	HIP_TRY(hipMemsetAsync(vs, 0, 6 * sizeof(u64), c.stream));
	hipLaunchKernelGGL((rsx_check_ranks_kernel<KT, IT>), dim3(2048), dim3(256), 0, c.stream, (const KT *)nullptr, (const IT *)nullptr, (u64)n, ka, vs);
	hipLaunchKernelGGL((rsx_check_ranks_kernel<KT, IT>), dim3(2048), dim3(256), 0, c.stream, src, (const IT *)*result, (u64)n, ka, vs + 3);
	HIP_TRY(hipGetLastError());
	u64 h[6];
	HIP_TRY(hipMemcpyAsync(h, vs, sizeof h, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	if (env().verify_inject)
		h[5] ^= 1;
	if (h[3] != 0 || h[1] != h[4] || h[2] != h[5])
		return fail(RSX_EVERIFY, "RSX_VERIFY=2: the ranks of a sort of %zu keys (route %u) are %s: %llu places out of order, rank sum %s, rank mix %s",
		            n, info ? info->hybrid : 0u, h[3] ? "not the stable order" : "not a permutation of 0 .. n-1", (unsigned long long)h[3],
		            h[1] == h[4] ? "right" : "wrong", h[2] == h[5] ? "right" : "wrong");
	return RSX_OK;
}

template <typename KT, typename IT>
int sort_rank_device_impl(Ctx &c, const KT *src, IT *ib, size_t n, int dtype, int order, void **result, rsx_info *info, int want_half)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (c.fast && n * 2 * (sizeof(KT) + sizeof(IT)) <= SMALL_PAIR_BYTES && !env().no_small_sort && !capture_armed() &&
	    want_half < 0) {
		ProfScope prof(1, (u64)n * (sizeof(KT) + 2 * sizeof(IT)), c.stream);
		hipLaunchKernelGGL((rsx_small_pairs_kernel<KT, IT, true>), dim3(1), dim3(1024), 0, c.stream, src, (KT *)nullptr, ib, ib + n,
		                   (u32)n, ka, c.dev_host_plan);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(c.stream));
		const Plan p = *c.host_plan;
		info_from_plan(info, p);
		if (info) {
			info->early_exit = p.sorted ? 2 : 0;
			info->result_in_aux = p.ncols & 1;
		}
		*result = (p.ncols & 1) ? ib + n : ib;   // radix_sort_rank.hpp:91 (sorted: first half = iota)
		return RSX_OK;
	}
	if constexpr (sizeof(KT) == 4 && sizeof(IT) == 4) {
		if (want_half < 0 && !env().compact_bits && blind_wanted<KT>(c, n, sizeof(IT), true)) {
			int done = 0;
			// (spare buffers: the index buffer's two halves -- the second one, which the reference's passes ping-pong through
			// (radix_sort_rank.hpp:77-91), for the keys' level-1 slots)
			RSX_TRY((pairs_blind<KT, IT>(c, src, (const IT *)nullptr, (KT *)nullptr, ib, n, ka, info, &done, (KT *)(ib + n), ib)));
			if (done) {   // four kept columns: the ranks are in the first half (radix_sort_rank.hpp:91)
				*result = ib;
				if (info)
					info->result_in_aux = 0;
				return RSX_OK;
			}
		}
	}
	Plan plan;
	RSX_TRY(plan_phase<KT>(c, src, n, ka, &plan, 0,
	                       (c.fast && want_half < 0 && !capture_armed() && !verify_mode() && !env().compact_bits)
	                           ? hybrid_caps_pairs<KT>(n, sizeof(IT)) : HybCaps{0, 0, 0, 0}));
	info_from_plan(info, plan);
	RSX_TRY(capture_hist(c, n, sizeof(KT)));
	if constexpr (sizeof(KT) == 4 && sizeof(IT) == 4) {
		if (!plan.sorted && plan.hyb == HYB_ONE_LEVEL && want_half < 0) {
			// mid-size arrays: one MSB pass of (key, index), which makes the indices, and the pairs' leaves write the ranks
			const u32 P = plan.ncols, top = plan.cols[P - 1];
			RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
			IT *fin = (P & 1) ? ib + n : ib, *scratch = (P & 1) ? ib : ib + n;
			RSX_TRY((scatter_pass<KT, IT>(c, src, (KT *)c.keys[0].p, (const IT *)fin, scratch, n, 8 * top, c.ghist() + 256 * top, ka,
			                              (u32)SCATTER_GEN_INDEX)));
			RSX_TRY((pairs_one_level<KT, IT>(c, (const KT *)c.keys[0].p, (const IT *)scratch, (KT *)nullptr, fin, n, ka)));
			*result = fin;
			if (info) {
				info->result_in_aux = fin != ib;
				info->hybrid = 1;
			}
			return RSX_OK;
		}
		if (!plan.sorted && plan.hyb == HYB_TWO_LEVEL && want_half < 0) {
			// Keys spread over their top two columns (cfg 4 (i)): two MSB passes of (key, index) -- the first makes the indices,
			// the second goes into slots -- and leaves that write the ranks where the parity rule says (radix_sort_rank.hpp:91).
			// On a slot's overflow nothing has been written to that half: the ordinary passes follow.
			const u32 P = plan.ncols, top = plan.cols[P - 1];
			RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
			IT *fin = (P & 1) ? ib + n : ib, *scratch = (P & 1) ? ib : ib + n;
			RSX_TRY((scatter_pass<KT, IT>(c, src, (KT *)c.keys[0].p, (const IT *)fin, scratch, n, 8 * top, c.ghist() + 256 * top, ka,
			                              (u32)SCATTER_GEN_INDEX)));
			bool ok = false;
			RSX_TRY((pairs_two_level<KT, IT>(c, (const KT *)c.keys[0].p, (const IT *)scratch, (KT *)nullptr, fin, n, ka, &ok)));
			if (ok) {
				*result = fin;
				if (info) {
					info->result_in_aux = fin != ib;
					info->hybrid = 4;
				}
				return RSX_OK;
			}
		}
	}
	if (plan.sorted) {                       // radix_sort_rank.hpp:52,:55-57: first half = iota
		hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, ib, (u64)n);
		HIP_TRY(hipGetLastError());
		return finish_sorted(info, result, ib);
	}
	const u32 P = plan.ncols;
	// README.md:716-758, "key compaction" (SURVEY.md 8 f4), behind RSX_COMPACT_BITS=1: when the bits that vary among the
	// keys (plan.vary, read off the histograms) fit fewer bytes than there are varying byte columns, the keys' varying bits
	// are packed together (one elementwise pass) and the packed values are rank-sorted instead: ceil(bits / 8) passes over
	// narrower keys.  The ranks are the same (all other bits are equal in every key) and they are left in the half the
	// reference's number of passes dictates.
	if (want_half < 0 && c.fast && sizeof(IT) == 4 && P > 1) {
		const bool compact_on = env().compact_bits;
		const u64 vary = ((u64)plan.vary_hi << 32) | plan.vary_lo;
		const u32 bits = (u32)__builtin_popcountll(vary), P2 = (bits + 7) / 8;
		BitRuns runs;
		if (compact_on && vary && P2 < P && bit_runs(vary, &runs)) {
			const u32 ob = P2 <= 1 ? 1 : P2 <= 2 ? 2 : P2 <= 4 ? 4 : 8;
			RSX_TRY(c.ckeys.ensure(n * ob));
			const dim3 grid(4096), block(256);
			rsx_info inner;
			int rc = RSX_EINVAL;
			const int half = (int)(P & 1);
			if (ob == 1) {
				hipLaunchKernelGGL((rsx_compact_bits_kernel<KT, uint8_t>), grid, block, 0, c.stream, src, (uint8_t *)c.ckeys.p, (u64)n, ka, runs);
				rc = sort_rank_device<uint8_t, IT>(c, (const uint8_t *)c.ckeys.p, ib, n, RSX_U8, RSX_ASCENDING, result, &inner, half);
			} else if (ob == 2) {
				hipLaunchKernelGGL((rsx_compact_bits_kernel<KT, uint16_t>), grid, block, 0, c.stream, src, (uint16_t *)c.ckeys.p, (u64)n, ka, runs);
				rc = sort_rank_device<uint16_t, IT>(c, (const uint16_t *)c.ckeys.p, ib, n, RSX_U16, RSX_ASCENDING, result, &inner, half);
			} else if (ob == 4) {
				hipLaunchKernelGGL((rsx_compact_bits_kernel<KT, u32>), grid, block, 0, c.stream, src, (u32 *)c.ckeys.p, (u64)n, ka, runs);
				rc = sort_rank_device<u32, IT>(c, (const u32 *)c.ckeys.p, ib, n, RSX_U32, RSX_ASCENDING, result, &inner, half);
			} else {
				hipLaunchKernelGGL((rsx_compact_bits_kernel<KT, u64>), grid, block, 0, c.stream, src, (u64 *)c.ckeys.p, (u64)n, ka, runs);
				rc = sort_rank_device<u64, IT>(c, (const u64 *)c.ckeys.p, ib, n, RSX_U64, RSX_ASCENDING, result, &inner, half);
			}
			RSX_TRY(rc);
			if (info)
				info->result_in_aux = P & 1;   // (ncols / cols stay the reference's: those of the original keys)
			return RSX_OK;
		}
	}
	if (P > 1) {
		RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
		if (P > 2)
			RSX_TRY(c.keys[1].ensure(n * sizeof(KT)));
	}
	// want_half: the halves swap roles when the number of passes would leave the ranks in the other one
	const bool swap_halves = want_half >= 0 && (int)(P & 1) != want_half;
	IT *H[2] = {swap_halves ? ib + n : ib, swap_halves ? ib : ib + n};
	if (c.fast && sizeof(IT) == 4 && !env().no_narrow_keys) {
		// The ranks are the only output, so a pass hands on just the key bytes that later passes look at: once those fit a
		// narrower type the keys are written as kdf(key) >> (8 * next column) in that type, and the passes after it read
		// it with the identity KDF.  `base_col`: the column that sits in the low byte of the current representation.
		const void *kin = src;
		u32 in_bytes = sizeof(KT), base_col = 0;
		bool applied = false;
		for (u32 i = 0; i < P; ++i) {
			const u32 col = plan.cols[i];
			u32 flags = hot_flags(plan.hot, col);
			if (i == 0)
				flags |= SCATTER_GEN_INDEX;
			if (i == P - 1)
				flags |= SCATTER_SKIP_KEYS;
			u32 out_bytes = in_bytes, oshift = 0, next = base_col;
			if (i + 1 < P) {
				const u32 need = (u32)sizeof(KT) - plan.cols[i + 1];   // bytes from the next kept column up
				const u32 fit = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
				if (fit < in_bytes) {
					out_bytes = fit;
					next = plan.cols[i + 1];
					oshift = 8 * (next - base_col);
				}
			}
			void *kout = c.keys[i & 1].p;
			const u32 shift = 8 * (col - base_col);
			const u64 *gb = c.ghist() + 256 * col;
			int rc = RSX_EINVAL;
			if (in_bytes == sizeof(KT))
				rc = rank_pass<KT, KT, IT>(c, kin, kout, out_bytes, H[i & 1], H[(i + 1) & 1], n, shift, gb, ka, applied, flags, oshift);
			else if (in_bytes == 4)
				rc = rank_pass<NarrowerOr<KT, u32>, KT, IT>(c, kin, kout, out_bytes, H[i & 1], H[(i + 1) & 1], n, shift, gb, ka, true,
				                                           flags, oshift);
			else if (in_bytes == 2)
				rc = rank_pass<NarrowerOr<KT, uint16_t>, KT, IT>(c, kin, kout, out_bytes, H[i & 1], H[(i + 1) & 1], n, shift, gb, ka,
				                                                true, flags, oshift);
			else if (in_bytes == 1)
				rc = rank_pass<uint8_t, KT, IT>(c, kin, kout, out_bytes, H[i & 1], H[(i + 1) & 1], n, shift, gb, ka, true, flags,
				                                oshift);
			RSX_TRY(rc);
			if (out_bytes != in_bytes) {
				in_bytes = out_bytes;
				base_col = next;
				applied = true;
			}
			kin = kout;
		}
	} else
	for (u32 i = 0; i < P; ++i) {
		const u32 col = plan.cols[i];
		const KT *kin = i == 0 ? src : (const KT *)c.keys[(i - 1) & 1].p;
		KT *kout = (KT *)c.keys[i & 1].p;
		u32 flags = hot_flags(plan.hot, col);
		if (i == 0)
			flags |= SCATTER_GEN_INDEX;
		if (i == P - 1)
			flags |= SCATTER_SKIP_KEYS;
		RSX_TRY((scatter_pass<KT, IT>(c, kin, kout, H[i & 1], H[(i + 1) & 1], n, 8 * col, c.ghist() + 256 * col, ka, flags)));
	}
	*result = H[P & 1];                      // radix_sort_rank.hpp:91
	if (info)
		info->result_in_aux = *result != (void *)ib;
	return RSX_OK;
}

// ---- stable argsort, no host synchronisation: every pass is device-scheduled, the ranks always end in the FIRST half -----------
// radix_sort_rank.hpp:97-112 for callers that cannot wait (graphs, the multi-GPU chunk pipeline).  The number of passes is only
// known on the device, so the passes take their buffers from the plan (SCATTER_RANK_ASYNC): the last one writes the first
// half.  Keys travel at full width (which narrower type a pass could write is a choice of kernel, i.e. the host's).
template <typename KT, typename IT>
int sort_rank_inplace_async(Ctx &c, const KT *src, IT *ib, size_t n, int dtype, int order)
{
	if (!c.fast)
		return fail(RSX_EHIP, "rsx_sort_rank_inplace_async needs the fast scatter kernel (the device self-check failed on this device)");
	c.async_tried_blind = false;   // (rsx_async_route reports THIS call: set again below if an attempt is enqueued)
	c.async_small = false;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (n * 2 * (sizeof(KT) + sizeof(IT)) <= SMALL_PAIR_BYTES) {
		hipLaunchKernelGGL((rsx_small_pairs_kernel<KT, IT, true>), dim3(1), dim3(1024), 0, c.stream, src, (KT *)nullptr, ib, ib + n,
		                   (u32)n, ka, c.dev_host_plan, true);
		HIP_TRY(hipGetLastError());
		c.async_small = true;
		return RSX_OK;
	}
	RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
	RSX_TRY(c.keys[1].ensure(n * sizeof(KT)));
	const size_t status_total = status_bytes<KT, IT>(n) * sizeof(KT);
	// the attempt without a histogram first (4-byte keys, 4-byte indices, 16 Mi .. 2^28 keys: its leaves write the ranks to the
	// first half), the histogram-first kernels behind it gated on its verdict -- as sort_keys_inplace_async
	int blind = 0;
	ProfAsyncVerdict pverdict(c.stream);
	if constexpr (sizeof(KT) == 4 && sizeof(IT) == 4) {
		if (async_pairs_blind_ok<KT>(c, n, sizeof(IT)))
			RSX_TRY((pairs_blind_enqueue<KT, IT>(c, src, (const IT *)nullptr, (KT *)nullptr, ib, n, ka, &blind, (KT *)(ib + n), ib)));
	}
	if (blind)
		pverdict.attempt_enqueued(SegView(c).ctl());
	c.pass_gate = blind ? SegView(c).ctl() : nullptr;
	c.async_tried_blind = blind != 0;
	int rc = plan_phase<KT>(c, src, n, ka, nullptr, status_total);
	c.pass_alt = c.keys[1].p;
	for (u32 i = 0; i < sizeof(KT) && rc == RSX_OK; ++i)   // pass i = the i-th kept column, if there is one
		rc = scatter_pass<KT, IT>(c, src, (KT *)c.keys[0].p, ib, ib + n, n, 0, c.ghist(), ka, SCATTER_RANK_ASYNC, c.plan(), (int)i, i);
	c.pass_alt = nullptr;
	c.pass_gate = nullptr;
	RSX_TRY(rc);
	pverdict.gated_enqueued();
	// sorted keys: no pass ran, the ranks are 0 .. n-1 (radix_sort_rank.hpp:52,:55-57)
	hipLaunchKernelGGL((rsx_iota_if_sorted_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, ib, (u64)n, (const Plan *)c.plan());
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

bool is_device_ptr(const void *p)
{
	hipPointerAttribute_t attr;
	hipError_t e = hipPointerGetAttributes(&attr, p);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return false;
	}
	return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// dispatch on key width
// ---- one plain scatter pass by the top KDF byte (rsx_msd_split_device) ---------------------------------------------
template <typename KT>
int msd_split(Ctx &c, const KT *src, KT *dst, size_t n, int dtype, int order, u32 col, uint64_t *top_hist)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u64 *top = c.ghist() + 256 * col;
	RSX_TRY(launch_hist<KT>(c, src, n, ka, c.ghist(), c.unsorted(), 1u << col));   // only the column split by
	HIP_TRY(hipMemcpyAsync(c.host_hist, top, 256 * sizeof(u64), hipMemcpyDeviceToHost, c.stream));   // counts, before the scan
	hipLaunchKernelGGL((rsx_plan_kernel<KT>), dim3(sizeof(KT)), dim3(256), 0, c.stream, src, (u64)n, c.ghist(), ka, c.kept(),
	                   c.hotd());
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c.stream));
	u64 total = 0;
	u64 most = 0;
	for (int i = 0; i < 256; ++i) {
		top_hist[i] = c.host_hist[i];
		total += top_hist[i];
		most = std::max<u64>(most, top_hist[i]);
	}
	if (total != n)
		return fail(RSX_EHIP, "rsx_msd_split_device: digit counts sum to %llu, n = %zu", (unsigned long long)total, n);
	const u32 flags = most >= (u64)n / 8 + 1 ? hot_flags(1u << col, col) : 0u;   // as Plan::hot (rsx_plan_kernel)
	return scatter_pass<KT, NoVal>(c, src, dst, nullptr, nullptr, n, 8 * col, top, ka, flags);
}

// The same pass for a caller that HAS the shard's column counts (rsx_histogram_device: one read gave every column): nothing
// is counted again and nothing waits for the host.
template <typename KT>
int msd_split_known(Ctx &c, const KT *src, KT *dst, size_t n, int dtype, int order, u32 col, const u64 *d_counts, bool hot)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	HIP_TRY(hipMemcpyAsync(c.ghist(), d_counts, sizeof(KT) * 256 * sizeof(u64), hipMemcpyDeviceToDevice, c.stream));
	hipLaunchKernelGGL((rsx_plan_kernel<KT>), dim3(sizeof(KT)), dim3(256), 0, c.stream, src, (u64)n, c.ghist(), ka, c.kept(),
	                   c.hotd());   // (the exclusive scans, radix_sort.hpp:72-80)
	HIP_TRY(hipGetLastError());
	// (a dominant digit -- the caller has the counts on the host and says so: the ballot-ranked kernel, as msd_split's;
	// its hot digits are rsx_plan_kernel's, on the device)
	return scatter_pass<KT, NoVal>(c, src, dst, nullptr, nullptr, n, 8 * col, c.ghist() + 256 * col, ka,
	                               hot ? hot_flags(1u << col, col) : 0u);
}

#include "rsx_multi_state.hpp"   // rsx_sort_multi: per-rank streams, buffers, phases, peer access

}  // namespace

#include "rsx_api.hpp"   // what the entry points share: dispatch by type, argument checks, host staging

// =================================================================================
// extern "C" surface
// =================================================================================

extern "C" {

int rsx_device_count(void)
{
	std::lock_guard<std::mutex> lock(g_mu);
	return probe_devices();
}

const char *rsx_last_error(void) { return g_err; }
const char *rsx_version(void) { return "rsx 0.1 (gfx950)"; }
size_t rsx_dtype_size(rsx_dtype dtype) { return dtype_size(dtype); }

size_t rsx_workspace_bytes(size_t n, rsx_dtype dtype, size_t payload_bytes)
{
	const size_t kb = dtype_size(dtype);
	if (!kb)
		return 0;
	// upper bound over the kernels' shapes: quarter tiles (8 Ki elements, 4 Ki with an 8-byte element), a region of status
	// words per pass, the histogram kernel's rows (at most 512 workgroups)
	const size_t elem = kb > payload_bytes ? kb : payload_bytes;
	const size_t tile = elem == 8 ? 4096 : 8192;
	const size_t tiles = (n + tile - 1) / tile;
	const size_t status = (256 + tiles * 256 * (n >= (1ull << 30) ? 8 : 4)) * kb;
	return 512 + kb * 256 * 8 + ((status + 255) & ~(size_t)255) + (size_t)512 * kb * 256 * 4 + 256;
}

void rsx_release(void)
{
	std::lock_guard<std::mutex> lock(g_mu);
	for (auto &kv : g_ctx) {
		(void)hipSetDevice(kv.first.first);
		kv.second->release();
		delete kv.second;
	}
	g_ctx.clear();
	for (auto &kv : g_multi_streams) {
		(void)hipSetDevice(kv.first.first);
		(void)hipStreamDestroy(kv.second);
	}
	g_multi_streams.clear();
	for (auto &kv : g_multi_bufs) {
		(void)hipSetDevice(kv.first.first);
		kv.second.shard.release();
		kv.second.part.release();
		kv.second.recv.release();
		kv.second.aux.release();
		kv.second.misc.release();
	}
	g_multi_bufs.clear();
}

namespace {

// A context whose device state lies in the caller's workspace: [flags 256][plan 64 + pad][histogram][status regions]
// [histogram rows].  Everything a captured graph of the *_ws entry points refers to is inside that workspace.
int borrow_ctx(Ctx &v, void *stream, void *ws, size_t ws_bytes, size_t n, size_t kb, size_t status_total, char **end = nullptr)
{
	// (no context of the library's own is created or touched: the call may be inside a stream capture, where nothing may
	// be allocated; the device self-check has run when any other entry point was used before, otherwise it runs now)
	int dev = 0;
	{
		std::lock_guard<std::mutex> lock(g_mu);
		if (probe_devices() <= 0)
			return fail(RSX_ENODEVICE, "no gfx950 (MI355X) device visible to HIP; this library has no CPU path");
		HIP_TRY(hipGetDevice(&dev));
		hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
		if (g_lds_order_ok.find(dev) == g_lds_order_ok.end() && hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess &&
		    cap != hipStreamCaptureStatusNone)
			return fail(RSX_EINVAL, "the library's first use on this device is inside a stream capture: call rsx_device_count() "
			                        "and any sort (or rsx_sort_inplace_async_ws itself) once before capturing -- the device "
			                        "self-check cannot run inside a capture");
		(void)hipGetLastError();
		if (!lds_order_selfcheck(dev))
			return fail(RSX_EHIP, "the device-scheduled sorts need the fast scatter kernel (the device self-check failed on this device)");
	}
	if (((uintptr_t)ws & 255) != 0)
		return fail(RSX_EINVAL, "the workspace must be 256-byte aligned");
	const size_t hist_bytes = kb * 256 * sizeof(u64), hpart_bytes = (size_t)512 * kb * 256 * sizeof(u32);
	const size_t need = 512 + hist_bytes + ((status_total + 255) & ~(size_t)255) + hpart_bytes;
	if (!ws || ws_bytes < need)
		return fail(RSX_EINVAL, "workspace of %zu bytes, %zu needed for %zu keys (rsx_workspace_bytes gives an upper bound)", ws_bytes, need, n);
	char *p = (char *)ws;
	v.device = dev;
	v.stream = (hipStream_t)stream;
	v.fast = true;
	v.small.borrow(p, 256);
	v.dev_host_plan = (Plan *)(p + 256);          // (the kernels' second copy of the plan: nobody reads it on the host)
	v.host_plan = nullptr;
	p += 512;
	v.hist.borrow(p, hist_bytes);
	p += hist_bytes;
	v.status.borrow(p, (status_total + 255) & ~(size_t)255);
	p += (status_total + 255) & ~(size_t)255;
	v.hpart.borrow(p, hpart_bytes);
	if (end)
		*end = p + hpart_bytes;
	return RSX_OK;
}

}  // namespace

int rsx_capture_histogram(uint64_t *hist, size_t entries)
{
	g_capture_dst = (u64 *)hist;
	g_capture_entries = hist ? entries : 0;
	return RSX_OK;
}

int rsx_sort_inplace_async(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *stream)
{
	if (!dtype_size(dtype) || (n && (!d_buf || !d_scratch)))
		return fail(RSX_EINVAL, "rsx_sort_inplace_async: bad argument");
	if (n < 2)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	AsyncScope async_scope((hipStream_t)stream);
	AsyncSetScope set_scope(*c);
	RSX_DISPATCH_KT(dtype, return sort_keys_inplace_async<KT>(*c, (KT *)d_buf, (KT *)d_scratch, n, dtype, order));
	return RSX_OK;
}

int rsx_sort_inplace_async_hint(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *stream, uint32_t hints)
{
	if (!dtype_size(dtype) || (n && (!d_buf || !d_scratch)))
		return fail(RSX_EINVAL, "rsx_sort_inplace_async_hint: bad argument");
	if (n < 2)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	AsyncScope async_scope((hipStream_t)stream);
	AsyncSetScope set_scope(*c);
	struct HintScope {   // (the sample kernel of the attempt enqueued by this call reads them: blind_enqueue)
		Ctx &c;
		HintScope(Ctx &c_, u32 h) : c(c_) { c.hints = h; }
		~HintScope() { c.hints = 0; }
	} hint_scope(*c, (u32)hints);
	RSX_DISPATCH_KT(dtype, return sort_keys_inplace_async<KT>(*c, (KT *)d_buf, (KT *)d_scratch, n, dtype, order));
	return RSX_OK;
}

int rsx_sort_inplace_async_ws(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *d_workspace,
                              size_t workspace_bytes, void *stream)
{
	const size_t kb = dtype_size(dtype);
	if (!kb || (n && (!d_buf || !d_scratch)))
		return fail(RSX_EINVAL, "rsx_sort_inplace_async_ws: bad argument");
	if (n < 2)
		return RSX_OK;
	Ctx view;
	size_t status_total = 0;
	RSX_DISPATCH_KT(dtype, status_total = (status_bytes<KT, NoVal>(n) * sizeof(KT)));
	char *end = nullptr;
	RSX_TRY(borrow_ctx(view, stream, d_workspace, workspace_bytes, n, kb, status_total, &end));
	// a workspace sized by rsx_workspace_bytes_fast also holds the slots of a sort without a histogram: the attempt is made in it
	RSX_DISPATCH_KT(dtype, borrow_blind<KT>(view, end, (char *)d_workspace + workspace_bytes, n));
	AsyncScope async_scope((hipStream_t)stream);
	RSX_DISPATCH_KT(dtype, return sort_keys_inplace_async<KT>(view, (KT *)d_buf, (KT *)d_scratch, n, dtype, order));
	return RSX_OK;
}

size_t rsx_workspace_bytes_fast(size_t n, rsx_dtype dtype)
{
	const size_t kb = dtype_size(dtype);
	if (!kb)
		return 0;
	size_t g = 0, sg = 0, s1 = 0, s2 = 0;
	if (kb >= 4 && n >= ((size_t)1 << 22) && n < ((size_t)1 << 30)) {
		if (kb == 4)
			blind_sizes<u32>(n, &g, &sg, &s1, &s2);
		else
			blind_sizes<u64>(n, &g, &sg, &s1, &s2);
	}
	return ((rsx_workspace_bytes(n, dtype, 0) + 255) & ~(size_t)255) + 256 + g + sg + s1 + s2;
}

int rsx_async_route_ws(const void *d_workspace, size_t workspace_bytes, size_t n, rsx_dtype dtype, void *stream, uint32_t *route)
{
	const size_t kb = dtype_size(dtype);
	if (!route || !d_workspace || !kb)
		return fail(RSX_EINVAL, "rsx_async_route_ws: bad argument");
	*route = 0;
	HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
	Plan plan;
	HIP_TRY(hipMemcpy(&plan, (const char *)d_workspace + 64, sizeof(plan), hipMemcpyDeviceToHost));
	// (the layout of borrow_ctx / borrow_blind: the control block of the attempt lies behind the histogram kernel's rows and gscan)
	size_t status_total = 0;
	RSX_DISPATCH_KT(dtype, status_total = (status_bytes<KT, NoVal>(n) * sizeof(KT)));
	const size_t minimal = 512 + kb * 256 * sizeof(u64) + ((status_total + 255) & ~(size_t)255) + (size_t)512 * kb * 256 * sizeof(u32);
	if (kb >= 4 && workspace_bytes >= rsx_workspace_bytes_fast(n, dtype) && n >= ((size_t)1 << 22) && n < ((size_t)1 << 30)) {
		const char *p = (const char *)(((uintptr_t)d_workspace + minimal + 255) & ~(uintptr_t)255) + 256 * sizeof(u64);
		SegCtl ctl;
		HIP_TRY(hipMemcpy(&ctl, p, sizeof(ctl), hipMemcpyDeviceToHost));
		if (ctl.mode == SEG_MODE_LEAVES && ctl.blind == BLIND_GO) {
			*route = 5;
			return RSX_OK;
		}
	}
	if (!plan.sorted && plan.hyb == HYB_ONE_LEVEL)
		*route = 1;
	return RSX_OK;
}

int rsx_sort_pairs_inplace_async_ws(void *d_keys, void *d_keys_scratch, void *d_vals, void *d_vals_scratch, size_t n, rsx_dtype dtype,
                                    size_t payload_bytes, rsx_order order, void *d_workspace, size_t workspace_bytes, void *stream)
{
	const size_t kb = dtype_size(dtype);
	if (!kb || (payload_bytes != 4 && payload_bytes != 8) || (n && (!d_keys || !d_keys_scratch || !d_vals || !d_vals_scratch)))
		return fail(RSX_EINVAL, "rsx_sort_pairs_inplace_async_ws: bad argument");
	if (n < 2)
		return RSX_OK;
	Ctx view;
	size_t status_total = 0;
	RSX_DISPATCH_KT_W(dtype, payload_bytes, VT, status_total = (status_bytes<KT, VT>(n) * sizeof(KT)));
	RSX_TRY(borrow_ctx(view, stream, d_workspace, workspace_bytes, n, kb, status_total));
	RSX_DISPATCH_KT_W(dtype, payload_bytes, VT, return (sort_pairs_inplace_async<KT, VT>(view, (KT *)d_keys, (KT *)d_keys_scratch, (VT *)d_vals,
	                                                                                     (VT *)d_vals_scratch, n, dtype, order)));
	return RSX_OK;
}

void rsx_release_stream(void *stream)
{
	// Lock order everywhere else: a context's mutex, then g_mu (the host wrappers hold the context and look contexts up
	// again).  So the context is taken out of the table under g_mu alone, and only then locked, drained and freed.  The
	// caller must not have another thread inside the library on this (device, stream) -- see rsx.h.
	Ctx *c = nullptr;
	{
		std::lock_guard<std::mutex> lock(g_mu);
		int dev = 0;
		if (hipGetDevice(&dev) != hipSuccess) {
			(void)hipGetLastError();
			return;
		}
		auto it = g_ctx.find(std::make_pair(dev, stream));
		if (it == g_ctx.end())
			return;
		c = it->second;
		g_ctx.erase(it);
	}
	{
		std::lock_guard<std::recursive_mutex> ctx_lock(c->mu);   // (a call that was already running on it finishes first)
		(void)hipStreamSynchronize(c->stream);
		c->release();
	}
	delete c;
}

int rsx_sort_pairs_inplace_async(void *d_keys, void *d_keys_scratch, void *d_vals, void *d_vals_scratch, size_t n, rsx_dtype dtype,
                                 size_t payload_bytes, rsx_order order, void *stream)
{
	if (!dtype_size(dtype) || (payload_bytes != 4 && payload_bytes != 8) ||
	    (n && (!d_keys || !d_keys_scratch || !d_vals || !d_vals_scratch)))
		return fail(RSX_EINVAL, "rsx_sort_pairs_inplace_async: bad argument");
	if (n < 2)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	AsyncScope async_scope((hipStream_t)stream);
	AsyncSetScope set_scope(*c);
	RSX_DISPATCH_KT_W(dtype, payload_bytes, VT, return (sort_pairs_inplace_async<KT, VT>(*c, (KT *)d_keys, (KT *)d_keys_scratch, (VT *)d_vals,
	                                                                                     (VT *)d_vals_scratch, n, dtype, order)));
	return RSX_OK;
}

int rsx_sort_device(void *d_src, void *d_aux, size_t n, rsx_dtype dtype, rsx_order order, void *stream, void **result,
                    rsx_info *info)
{
	info_clear(info, dtype);
	if (!dtype_size(dtype) || !result || (n && (!d_src || !d_aux)))
		return fail(RSX_EINVAL, "rsx_sort_device: bad argument");
	if (n < 2) {                             // radix_sort.hpp:100-101
		*result = d_src;
		if (info)
			info->early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_DISPATCH_KT(dtype, return sort_keys_device<KT>(*c, (KT *)d_src, (KT *)d_aux, n, dtype, order, result, info));
	return RSX_OK;
}

int rsx_sort_pairs_device(void *d_keys, void *d_keys_aux, void *d_vals, void *d_vals_aux, size_t n, rsx_dtype dtype,
                          size_t payload_bytes, rsx_order order, void *stream, rsx_info *info)
{
	info_clear(info, dtype);
	if (!dtype_size(dtype) || (payload_bytes != 4 && payload_bytes != 8) ||
	    (n && (!d_keys || !d_keys_aux || !d_vals || !d_vals_aux)))
		return fail(RSX_EINVAL, "rsx_sort_pairs_device: bad argument");
	if (n < 2) {
		if (info)
			info->early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_DISPATCH_KT_W(dtype, payload_bytes, VT, return (sort_pairs_device<KT, VT>(*c, (KT *)d_keys, (KT *)d_keys_aux, (VT *)d_vals,
	                                                                              (VT *)d_vals_aux, n, dtype, order, info)));
	return RSX_OK;
}

int rsx_sort_rank_inplace_async(const void *d_src, void *d_index_buffer, size_t n, rsx_dtype dtype, size_t idx_bytes,
                                rsx_order order, void *stream)
{
	if (!dtype_size(dtype) || (idx_bytes != 4 && idx_bytes != 8) || (n && (!d_src || !d_index_buffer)))
		return fail(RSX_EINVAL, "rsx_sort_rank_inplace_async: bad argument");
	if (idx_bytes == 4 && n > (1ull << 32))
		return fail(RSX_EINVAL, "rsx_sort_rank_inplace_async: n does not fit a 4-byte index");
	if (n == 0)
		return RSX_OK;                       // radix_sort_rank.hpp:28-32
	RSX_LOCKED_CTX(c, stream);
	AsyncScope async_scope((hipStream_t)stream);
	AsyncSetScope set_scope(*c);
	if (n == 1) {
		HIP_TRY(hipMemsetAsync(d_index_buffer, 0, idx_bytes, c->stream));
		return RSX_OK;
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT, return (sort_rank_inplace_async<KT, IT>(*c, (const KT *)d_src, (IT *)d_index_buffer, n, dtype, order)));
	return RSX_OK;
}

int rsx_verify_poll(void *stream, uint64_t *mismatches)
{
	if (mismatches)
		*mismatches = 0;
	RSX_LOCKED_CTX(c, stream);
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (!c->vasync.p)
		return RSX_OK;
	u64 bad = 0;
	HIP_TRY(hipMemcpy(&bad, c->vasync.p, sizeof(bad), hipMemcpyDeviceToHost));
	if (mismatches)
		*mismatches = bad;
	if (bad) {
		HIP_TRY(hipMemset(c->vasync.p, 0, 8));
		return fail(RSX_EVERIFY, "RSX_VERIFY: a device-scheduled sort on this stream had a pass whose checked tile differs from its "
		                         "ballot-ranked re-computation in %llu places", (unsigned long long)bad);
	}
	return RSX_OK;
}

int rsx_async_route(void *stream, uint32_t *route)
{
	if (!route)
		return fail(RSX_EINVAL, "rsx_async_route: bad argument");
	*route = 0;
	RSX_LOCKED_CTX(c, stream);
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (c->async_small)
		return RSX_OK;   // (the one-launch sort writes no device-side plan: what lies there is an earlier sort's)
	Plan plan;
	HIP_TRY(hipMemcpy(&plan, c->async_plan(), sizeof(plan), hipMemcpyDeviceToHost));
	if (c->async_tried_blind && c->seg.p) {
		SegCtl ctl;
		HIP_TRY(hipMemcpy(&ctl, c->seg.p, sizeof(ctl), hipMemcpyDeviceToHost));
		if (getenv("RSX_DEBUG_ROUTE"))   // (what the device left behind: which test ended an attempt)
			fprintf(stderr, "rsx_async_route: blind %u mode %u overflow %u ntiles %u nleaf %u maxleaf %u shift1 %u shift2 %u cmask %08x%08x "
			                "narrow %u compact %u leaf16 %u boff_skip %u boff_next %u slots in the second buffer %u cap1 %u cap2 %u\n",
			        ctl.blind, ctl.mode, ctl.overflow, ctl.ntiles, ctl.nleaf, ctl.maxleaf, ctl.shift1, ctl.shift2, ctl.cmask_hi, ctl.cmask_lo,
			        ctl.narrow, ctl.compact, ctl.leaf16, ctl.boff_skip, ctl.boff_next, c->slack1_lo, c->slack1_cap, c->slack_cap);
		if (ctl.mode == SEG_MODE_LEAVES) {
			*route = 5;
			return RSX_OK;
		}
	}
	if (!plan.sorted && plan.hyb == HYB_ONE_LEVEL)
		*route = 1;
	return RSX_OK;
}

int rsx_sort_rank_device(const void *d_src, void *d_index_buffer, size_t n, rsx_dtype dtype, size_t idx_bytes,
                         rsx_order order, void *stream, void **result, rsx_info *info)
{
	info_clear(info, dtype);
	if (!dtype_size(dtype) || (idx_bytes != 4 && idx_bytes != 8) || !result || (n && (!d_src || !d_index_buffer)))
		return fail(RSX_EINVAL, "rsx_sort_rank_device: bad argument");
	if (idx_bytes == 4 && n > (1ull << 32))
		return fail(RSX_EINVAL, "rsx_sort_rank_device: n does not fit a 4-byte index");
	*result = d_index_buffer;
	if (n == 0) {                            // radix_sort_rank.hpp:28-32
		if (info)
			info->early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	if (n == 1) {
		HIP_TRY(hipMemsetAsync(d_index_buffer, 0, idx_bytes, c->stream));
		if (info)
			info->early_exit = 1;
		return RSX_OK;
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT, return (sort_rank_device<KT, IT>(*c, (const KT *)d_src, (IT *)d_index_buffer, n, dtype, order,
	                                                                         result, info)));
	return RSX_OK;
}

// host arrays the one-launch kernels take (sort_keys_device, sort_rank_device: the same conditions)
static bool host_small_path(const Ctx &c, size_t key_bytes)
{
	return c.fast && key_bytes <= SMALL_SORT_BYTES && !env().no_small_sort && !env().no_host_small && !capture_armed();
}

int rsx_sort(void *src, void *aux, size_t n, rsx_dtype dtype, rsx_order order, void **result, rsx_info *info)
{
	info_clear(info, dtype);
	const size_t kb = dtype_size(dtype);
	if (!kb || !result || (n && (!src || !aux)))
		return fail(RSX_EINVAL, "rsx_sort: bad argument");
	if (n < 2) {                             // radix_sort.hpp:100-101
		*result = src;
		if (info)
			info->early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	if (is_device_ptr(src)) {
		if (!is_device_ptr(aux))
			return fail(RSX_EINVAL, "rsx_sort: src is a device pointer but aux is not");
		RSX_TRY(rsx_sort_device(src, aux, n, dtype, order, nullptr, result, info));
		HIP_TRY(hipStreamSynchronize(c->stream));
		return RSX_OK;
	}
	if (host_small_path(*c, n * kb)) {
		// small host arrays: the one-launch kernel reads the keys from pinned memory and writes the result there
		RSX_TRY(c->ensure_hstage());
		memcpy(c->hstage, src, n * kb);
		void *dres = nullptr;
		rsx_info li;
		RSX_TRY(rsx_sort_device(c->hstage_dev, c->hstage_dev + SMALL_SORT_BYTES, n, dtype, order, nullptr, &dres, &li));
		if (info)
			*info = li;
		if (li.early_exit) {
			*result = src;
			return RSX_OK;
		}
		void *hres = li.result_in_aux ? aux : src;
		memcpy(hres, c->hstage + ((char *)dres - c->hstage_dev), n * kb);
		*result = hres;
		return RSX_OK;
	}
	// host buffers: stage over PCIe, sort in HBM, bring the result back into the
	// buffer the returned-pointer rule names (the other one is left as it was)
	RSX_TRY(c->keys[0].ensure(n * kb));
	RSX_TRY(c->keys[1].ensure(n * kb));
	HostRegScope reg_src(src, n * kb), reg_aux(aux, n * kb);   // (RSX_HOST_REGISTER=1: pinned until this call returns)
	HIP_TRY(hipMemcpyAsync(c->keys[0].p, src, n * kb, hipMemcpyHostToDevice, c->stream));
	void *dres = nullptr;
	rsx_info li;
	RSX_TRY(rsx_sort_device(c->keys[0].p, c->keys[1].p, n, dtype, order, nullptr, &dres, &li));
	if (info)
		*info = li;
	if (li.early_exit) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		*result = src;
		return RSX_OK;
	}
	void *hres = li.result_in_aux ? aux : src;
	HIP_TRY(hipMemcpyAsync(hres, dres, n * kb, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	*result = hres;
	return RSX_OK;
}

int rsx_sort_rank(const void *src, void *index_buffer, size_t n, rsx_dtype dtype, size_t idx_bytes, rsx_order order,
                  void **result, rsx_info *info)
{
	info_clear(info, dtype);
	const size_t kb = dtype_size(dtype);
	if (!kb || !result || (idx_bytes != 1 && idx_bytes != 2 && idx_bytes != 4 && idx_bytes != 8) ||
	    (n && (!src || !index_buffer)))
		return fail(RSX_EINVAL, "rsx_sort_rank: bad argument");
	if (idx_bytes < 8 && n > (1ull << (8 * idx_bytes)))
		return fail(RSX_EINVAL, "rsx_sort_rank: n = %zu does not fit a %zu-byte index", n, idx_bytes);
	*result = index_buffer;
	if (n == 0) {
		if (info)
			info->early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const bool dev = is_device_ptr(src);
	if (dev != is_device_ptr(index_buffer))
		return fail(RSX_EINVAL, "rsx_sort_rank: src and index_buffer must both be host or both be device pointers");
	if (dev && idx_bytes >= 4) {
		RSX_TRY(rsx_sort_rank_device(src, index_buffer, n, dtype, idx_bytes, order, nullptr, result, info));
		HIP_TRY(hipStreamSynchronize(c->stream));
		return RSX_OK;
	}
	const size_t wide = idx_bytes == 8 ? 8 : 4;
	if (!dev && host_small_path(*c, 0) && n * 2 * (kb + wide) <= SMALL_PAIR_BYTES) {
		// small host arrays: keys read from and ranks written to pinned memory by the one-launch kernel, narrowed here
		RSX_TRY(c->ensure_hstage());
		memcpy(c->hstage, src, n * kb);
		char *hib = c->hstage + SMALL_SORT_BYTES, *dib = c->hstage_dev + SMALL_SORT_BYTES;
		void *dres = nullptr;
		rsx_info li;
		RSX_TRY(rsx_sort_rank_device(c->hstage_dev, dib, n, dtype, wide, order, nullptr, &dres, &li));
		if (info)
			*info = li;
		const bool second = dres != (void *)dib;
		char *out = (char *)index_buffer + (second ? n * idx_bytes : 0);
		const char *from = hib + ((char *)dres - dib);
		if (idx_bytes >= 4) {
			memcpy(out, from, n * idx_bytes);
		} else if (idx_bytes == 2) {
			for (size_t i = 0; i < n; ++i)
				((uint16_t *)out)[i] = (uint16_t)((const u32 *)from)[i];
		} else {
			for (size_t i = 0; i < n; ++i)
				((uint8_t *)out)[i] = (uint8_t)((const u32 *)from)[i];
		}
		*result = out;
		return RSX_OK;
	}
	// staged path: keys in recs[0] (host keys) or in place (device keys); indices computed
	// as 4- or 8-byte values in vals[0], narrowed into vals[1] when IdxType is 1 or 2 bytes
	const void *dkeys = src;
	if (!dev) {
		RSX_TRY(c->recs[0].ensure(n * kb));
		HIP_TRY(hipMemcpyAsync(c->recs[0].p, src, n * kb, hipMemcpyHostToDevice, c->stream));
		dkeys = c->recs[0].p;
	}
	RSX_TRY(c->vals[0].ensure(2 * n * wide));
	void *dres = nullptr;
	rsx_info li;
	RSX_TRY(rsx_sort_rank_device(dkeys, c->vals[0].p, n, dtype, wide, order, nullptr, &dres, &li));
	if (info)
		*info = li;
	const bool second = dres != c->vals[0].p;
	char *out = (char *)index_buffer + (second ? n * idx_bytes : 0);
	const void *from = dres;
	if (idx_bytes < 4) {
		RSX_TRY(c->vals[1].ensure(n * idx_bytes));
		if (idx_bytes == 1)
			hipLaunchKernelGGL((rsx_convert_kernel<uint8_t, u32>), dim3(256), dim3(256), 0, c->stream, (uint8_t *)c->vals[1].p,
			                   (const u32 *)dres, (u64)n);
		else
			hipLaunchKernelGGL((rsx_convert_kernel<uint16_t, u32>), dim3(256), dim3(256), 0, c->stream,
			                   (uint16_t *)c->vals[1].p, (const u32 *)dres, (u64)n);
		HIP_TRY(hipGetLastError());
		from = c->vals[1].p;
	}
	HIP_TRY(hipMemcpyAsync(out, from, n * idx_bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	*result = out;
	return RSX_OK;
}

}  // extern "C"

// one file per feature: its host driver (anonymous namespace) and its entry points (extern "C")
#include "rsx_keybits_api.hpp"   // what the next three share: the sample and the plan, the bitmap, the heads, the index sort
#include "rsx_unique_api.hpp"    // rsx_sort_unique[_device]
#include "rsx_group_api.hpp"     // rsx_sort_group[_device]
#include "rsx_rankdata_api.hpp"  // rsx_sort_rankdata[_device]
#include "rsx_topk_api.hpp"      // rsx_sort_topk[_device]
#include "rsx_nth_api.hpp"       // rsx_sort_nth[_device]
#include "rsx_lex_api.hpp"       // rsx_sort_lex[_device]

extern "C" {

#include "rsx_records.hpp"       // rsx_sort_rank_keys, rsx_sort_records, rsx_sort_records_tagged[_device]

#include "rsx_multi_entry.hpp"   // rsx_sort_multi

int rsx_histogram_device(const void *d_src, size_t n, rsx_dtype dtype, rsx_order order, uint64_t *d_hist,
                         uint32_t *d_unsorted, void *stream)
{
	const size_t kb = dtype_size(dtype);
	if (!kb || !d_hist || !d_unsorted || (n && !d_src))
		return fail(RSX_EINVAL, "rsx_histogram_device: bad argument");
	RSX_LOCKED_CTX(c, stream);
	HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * kb * sizeof(u64), c->stream));
	HIP_TRY(hipMemsetAsync(d_unsorted, 0, sizeof(u32), c->stream));
	if (n == 0)
		return RSX_OK;
	RSX_DISPATCH_KT(dtype, return launch_hist<KT>(*c, (const KT *)d_src, n, make_kdf<KT>(dtype, order), (u64 *)d_hist,
	                                              (u32 *)d_unsorted));
	return RSX_OK;
}

// The MSD split of the multi-GPU sort as ONE ordinary scatter pass on the top KDF byte.  The destinations of the exchange are
// contiguous ranges of that byte (multi.py, choose_splitters), so a stable pass by the byte itself leaves every
// destination's keys contiguous in d_dst -- with 256 digits instead of G buckets there is no crowd of lanes on a handful
// of LDS counters, and the pass runs on the plain-digit kernel.  Keys of one destination arrive ordered by (top byte,
// original index) instead of by original index; equal keys have equal top bytes, so the stable order of the final result
// is the same.  top_hist (host, 256 uint64) receives the counts of the byte; the pass itself is only enqueued.  `column`
// picks another byte than the top one (a caller that knows the top bytes to be constant splits by the highest varying one).
int rsx_msd_split_device(const void *d_src, void *d_dst, size_t n, rsx_dtype dtype, rsx_order order, int column,
                         uint64_t *top_hist, void *stream)
{
	const size_t kb = dtype_size(dtype);
	if (!kb || !top_hist || column >= (int)kb || (n && (!d_src || !d_dst)))
		return fail(RSX_EINVAL, "rsx_msd_split_device: bad argument");
	const u32 col = column < 0 ? (u32)kb - 1 : (u32)column;
	for (int i = 0; i < 256; ++i)
		top_hist[i] = 0;
	if (n == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	const size_t hist_bytes = kb * 256 * sizeof(u64);
	HIP_TRY(hipMemsetAsync(c->ghist(), 0, hist_bytes, c->stream));
	HIP_TRY(hipMemsetAsync(c->small_set(), 0, 256, c->stream));
	RSX_DISPATCH_KT(dtype, return msd_split<KT>(*c, (const KT *)d_src, (KT *)d_dst, n, dtype, order, col, top_hist));
	return RSX_OK;
}

int rsx_msd_split_async(const void *d_src, void *d_dst, size_t n, rsx_dtype dtype, rsx_order order, int column,
                        const uint64_t *d_hist, void *stream)
{
	const size_t kb = dtype_size(dtype);
	const bool hot = column >= 0 && (column & RSX_SPLIT_HOT) != 0;
	if (column >= 0)
		column &= ~RSX_SPLIT_HOT;
	if (!kb || !d_hist || column >= (int)kb || (n && (!d_src || !d_dst)))
		return fail(RSX_EINVAL, "rsx_msd_split_async: bad argument");
	const u32 col = column < 0 ? (u32)kb - 1 : (u32)column;
	if (n == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	AsyncScope async_scope((hipStream_t)stream);
	AsyncSetScope set_scope(*c);
	HIP_TRY(hipMemsetAsync(c->small_set(), 0, 256, c->stream));
	RSX_DISPATCH_KT(dtype, return msd_split_known<KT>(*c, (const KT *)d_src, (KT *)d_dst, n, dtype, order, col, (const u64 *)d_hist, hot));
	return RSX_OK;
}

void rsx_reload_env(void)
{
	std::lock_guard<std::mutex> lock(g_mu);
	(void)env();
	g_env.load();
	g_env_epoch.fetch_add(1u);   // (contexts forget what they have learnt about their inputs: sort_keys_blind's back-off)
}

int rsx_profile_begin(void)
{
	std::lock_guard<std::mutex> lock(g_mu);
	for (auto &r : g_prof) {
		(void)hipEventDestroy(r.start);
		(void)hipEventDestroy(r.stop);
	}
	g_prof.clear();
	g_prof_on = true;
	return RSX_OK;
}

int rsx_profile_end(rsx_profile *out)
{
	std::lock_guard<std::mutex> lock(g_mu);
	g_prof_on = false;
	if (!out)
		return fail(RSX_EINVAL, "rsx_profile_end: null output");
	memset(out, 0, sizeof(*out));
	for (auto &r : g_prof) {
		float ms = 0.f;
		HIP_TRY(hipEventSynchronize(r.stop));
		HIP_TRY(hipEventElapsedTime(&ms, r.start, r.stop));
		if (r.verdict && ((r.valid_if == 1) != (*r.verdict == SEG_MODE_LEAVES)))
			r.called_off = true;
		if (r.called_off) {
			out->called_off_ms += ms;
			out->called_off_launches += 1;
		} else if (r.kind == 0) {
			out->hist_ms += ms;
			out->hist_launches += 1;
			out->hist_bytes += r.bytes;
		} else if (r.kind == 3) {
			out->narrow_ms += ms;
			out->narrow_launches += 1;
			out->narrow_bytes += r.bytes;
		} else if (r.kind == 2) {
			out->leaf_ms += ms;
			out->leaf_launches += 1;
			out->leaf_bytes += r.bytes;
		} else {
			out->scatter_ms += ms;
			out->scatter_launches += 1;
			out->scatter_bytes += r.bytes;
		}
		(void)hipEventDestroy(r.start);
		(void)hipEventDestroy(r.stop);
	}
	g_prof.clear();
	g_prof_vnext = 0;
	return RSX_OK;
}

int rsx_fill_splitmix_device(void *d_dst, size_t n, size_t elem_bytes, uint64_t seed, uint64_t mask, uint64_t first_index,
                             void *stream)
{
	if (n && !d_dst)
		return fail(RSX_EINVAL, "rsx_fill_splitmix_device: null destination");
	RSX_LOCKED_CTX(c, stream);
	if (n == 0)
		return RSX_OK;
	const dim3 grid(2048), block(256);
	switch (elem_bytes) {
	case 1: hipLaunchKernelGGL((rsx_fill_splitmix_kernel<uint8_t>), grid, block, 0, c->stream, (uint8_t *)d_dst, (u64)n, (u64)seed, (u64)mask, (u64)first_index); break;
	case 2: hipLaunchKernelGGL((rsx_fill_splitmix_kernel<uint16_t>), grid, block, 0, c->stream, (uint16_t *)d_dst, (u64)n, (u64)seed, (u64)mask, (u64)first_index); break;
	case 4: hipLaunchKernelGGL((rsx_fill_splitmix_kernel<u32>), grid, block, 0, c->stream, (u32 *)d_dst, (u64)n, (u64)seed, (u64)mask, (u64)first_index); break;
	case 8: hipLaunchKernelGGL((rsx_fill_splitmix_kernel<u64>), grid, block, 0, c->stream, (u64 *)d_dst, (u64)n, (u64)seed, (u64)mask, (u64)first_index); break;
	default: return fail(RSX_EINVAL, "rsx_fill_splitmix_device: elem_bytes must be 1, 2, 4 or 8");
	}
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

int rsx_spin_device(uint64_t microseconds, void *stream)
{
	if (microseconds > 1000000)
		return fail(RSX_EINVAL, "rsx_spin_device: at most one second");
	Ctx *c;
	RSX_TRY(get_ctx(stream, &c));
	hipLaunchKernelGGL(rsx_spin_kernel, dim3(1), dim3(64), 0, c->stream, (u64)microseconds * 100);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

}  // extern "C"
