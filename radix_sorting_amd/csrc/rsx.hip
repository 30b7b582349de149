// rsx.hip -- host side of librsx.so: the extern "C" surface declared in
// include/rsx.h on top of the kernels in rsx_kernels.hpp.
//
// The control flow mirrors rs_sort_main (radix_sort.hpp:31-93): histogram +
// pre-sorted test -> early exit -> column probe -> exclusive scan -> one stable
// scatter pass per kept column, ping-ponging two buffers -> "returned pointer".
// There is deliberately no CPU path here: if HIP cannot give us a gfx950
// device, every entry point fails with RSX_ENODEVICE.
// This file holds the passes themselves -- launch_hist, plan_phase, scatter_pass and their kin -- and the list of the parts
// that make up the host side (one translation unit: the kernel instantiations are shared); the drivers of the plain sorts are in
// rsx_sort_plain.hpp and rsx_sort_async.hpp, their entry points in rsx_plain_api.hpp, every feature in a file of its own.
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
#include "rsx_locate.hpp"
#include "rsx_partition.hpp"
#include "rsx_lex.hpp"
#include "rsx_reduce.hpp"
#include "rsx_join.hpp"
#include "rsx_segments.hpp"

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
#include "rsx_ws_layout.hpp"    // WsLayout: where the parts of a caller-owned workspace lie
#include "rsx_stage.hpp"        // stage_layout: where the arrays of a blocking call on host buffers lie in Ctx::stage
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

}  // namespace

#include "rsx_sort_plain.hpp"  // the blocking drivers: sort_keys_device, sort_pairs_device, sort_rank_device; the RSX_VERIFY=2 bracket
#include "rsx_sort_async.hpp"  // the device-scheduled ones: sort_*_inplace_async and the skeleton they share

namespace {

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

int rsx_capture_histogram(uint64_t *hist, size_t entries)
{
	g_capture_dst = (u64 *)hist;
	g_capture_entries = hist ? entries : 0;
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

}  // extern "C"

#include "rsx_plain_api.hpp"    // the plain sorts' entry points: rsx_sort*, rsx_sort_pairs*, rsx_sort_rank*, their *_inplace_async forms, the workspace

// one file per feature: its host driver (anonymous namespace) and its entry points (extern "C")
#include "rsx_keybits_api.hpp"   // what the next three share: the sample and the plan, the bitmap, the heads, the index sort
#include "rsx_unique_api.hpp"    // rsx_sort_unique[_device]
#include "rsx_group_api.hpp"     // rsx_sort_group[_device]
#include "rsx_rankdata_api.hpp"  // rsx_sort_rankdata[_device]
#include "rsx_topk_api.hpp"      // rsx_sort_topk[_device]
#include "rsx_nth_api.hpp"       // rsx_sort_nth[_device]
#include "rsx_locate_api.hpp"    // rsx_sort_locate[_device]
#include "rsx_partition_api.hpp" // rsx_sort_partition[_device]
#include "rsx_lex_api.hpp"       // rsx_sort_lex[_device]
#include "rsx_reduce_api.hpp"    // rsx_sort_reduce[_device]
#include "rsx_join_api.hpp"      // rsx_sort_join[_device], rsx_join_pairs[_device]
#include "rsx_segments_api.hpp"  // rsx_sort_segments[_device]

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
	RSX_ASYNC_CTX(c, stream);
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
