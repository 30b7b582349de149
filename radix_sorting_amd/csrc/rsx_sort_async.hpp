// rsx_sort_async.hpp: the device-scheduled drivers of the three plain sorts (sort_keys_inplace_async, sort_pairs_inplace_async,
// sort_rank_inplace_async: enqueue only, no host synchronisation, the stream may be capturing) and the skeleton they share; part of
// librsx.so's host side, included by rsx.hip behind rsx_sort_plain.hpp.
#pragma once

namespace {

// The routes of the blocking sort (rsx_hybrid.hpp), chosen on the device with nobody to read a verdict back:
//  * arrays the sort without a histogram is for: the whole attempt is enqueued first -- sample, two MSB passes
//    into slots, leaves -- and what follows (histogram, plan, one pass per kept column) looks at the attempt's verdict,
//    SegCtl::mode, and does nothing if the keys are sorted by then; an attempt that is called off has only read its input.
//    (The host never learns how an attempt went: a context's back-off after a LOST attempt -- one that passed the sample and
//    then overflowed a slot -- is kept on the device, SegCtl::boff_skip.  An attempt the sample turns away costs a sample kernel
//    and a few empty launches, one that goes through the empty launches of the histogram-first kernels.)
//  * mid-size arrays: one MSB pass and leaves where the device-side plan says so (Plan::hyb) -- pass 0 then goes by the
//    highest kept column, the leaf launches behind it do nothing otherwise, and the passes 1 .. do nothing if they do.
// A driver is: async_enter; the one-launch sort of a small array, which ends it; async_gated(attempt, gated work); its tail kernels.

// the refusal without the fast kernel, and the flags rsx_async_route reads, which report THIS call (set again by the small exit
// and by async_gated)
inline int async_enter(Ctx &c, const char *who)
{
	if (!c.fast)
		return fail(RSX_EHIP, "%s needs the fast scatter kernel (the device self-check failed on this device)", who);
	c.async_tried_blind = false;
	c.async_small = false;
	return RSX_OK;
}

// The histogram-first launches between its constructor and its destructor look at the attempt's verdict (Ctx::pass_gate; a null
// gate: no attempt, they always work).  However the launches end, no later sort of the context is gated, and none reads pass_alt.
struct GateScope {
	Ctx &c;
	GateScope(Ctx &c_, const SegCtl *gate) : c(c_) { c.pass_gate = gate; }
	~GateScope()
	{
		c.pass_gate = nullptr;
		c.pass_alt = nullptr;
	}
	GateScope(const GateScope &) = delete;
	GateScope &operator=(const GateScope &) = delete;
};

// attempt(&enqueued): the sort without a histogram, if this sort may try one (*enqueued = 1: it is on the stream);
// gated(): the histogram, the plan and the passes behind it.  rsx_profile books what the device chose: the attempt's
// launches or the ones behind it (ProfAsyncVerdict).
template <typename Attempt, typename Gated>
int async_gated(Ctx &c, Attempt attempt, Gated gated)
{
	ProfAsyncVerdict pverdict(c.stream);
	int blind = 0;
	RSX_TRY(attempt(&blind));
	if (blind)
		pverdict.attempt_enqueued(SegView(c).ctl());
	c.async_tried_blind = blind != 0;
	{
		GateScope gate(c, blind ? SegView(c).ctl() : nullptr);
		RSX_TRY(gated());
	}
	pverdict.gated_enqueued();
	return RSX_OK;
}

// ---- keys only: every pass is device-scheduled, the result always ends in `buf` ---------------------------------------------------
// A caller-owned workspace (rsx_sort_inplace_async_ws) makes the attempt if it was sized for the slots (rsx_workspace_bytes_fast).
template <typename KT>
int sort_keys_inplace_async(Ctx &c, KT *buf, KT *scratch, size_t n, int dtype, int order)
{
	RSX_TRY(async_enter(c, "rsx_sort_inplace_async"));
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (n * sizeof(KT) <= SMALL_SORT_BYTES) {
		hipLaunchKernelGGL((rsx_small_sort_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, buf, scratch, (u32)n, ka, c.dev_host_plan, true);
		HIP_TRY(hipGetLastError());
		c.async_small = true;
		return RSX_OK;
	}
	const size_t status_total = status_bytes<KT, NoVal>(n) * sizeof(KT);
	HybCaps caps{0, 0, 0, 0};
	RSX_TRY(async_gated(
	    c,
	    [&](int *enqueued) -> int {
		    if constexpr (sizeof(KT) >= 4) {
			    if (hybrid_enabled() && !verify_mode() && !env().no_speculation) {
				    caps = hybrid_caps<KT>(n);
				    caps.cap2 = caps.min_cols2 = 0;
				    if (async_blind_ok<KT>(c, n))
					    RSX_TRY(blind_enqueue<KT>(c, buf, scratch, n, ka, enqueued));
			    }
		    }
		    return RSX_OK;
	    },
	    [&]() -> int {
		    RSX_TRY(plan_phase<KT>(c, buf, n, ka, nullptr, status_total, caps));
		    for (u32 i = 0; i < sizeof(KT); ++i)   // pass i = the i-th kept column, if there is one (radix_sort.hpp:83-90)
			    RSX_TRY((scatter_pass<KT, NoVal>(c, buf, scratch, nullptr, nullptr, n, 0, c.ghist(), ka, 0, c.plan(), (int)i, i)));
		    if constexpr (sizeof(KT) >= 4) {
			    if (caps.cap1 && n <= (size_t)256 * caps.cap1) {
				    // (every shape: which one the largest bucket needs is only known on the device, and each does nothing unless the
				    // plan's largest bucket is its size -- keys with 64 values in their top byte fill buckets four times the mean)
				    const u32 shapes = LeafShapes<KT>::HAS_MEDIUM ? 7u : 3u;
				    RSX_TRY(launch_leaves<KT>(c, buf, scratch, n, ka, HYB_ONE_LEVEL, shapes));
			    }
		    }
		    return RSX_OK;
	    }));
	// an odd number of kept columns leaves the result in `scratch` (radix_sort.hpp:92): bring it home
	hipLaunchKernelGGL(rsx_copy_if_odd_kernel, dim3(2048), dim3(256), 0, c.stream, (unsigned char *)buf, (const unsigned char *)scratch,
	                   (u64)n * sizeof(KT), (const Plan *)c.plan());
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// ---- key + payload: as sort_keys_inplace_async, the result always in (k, v) --------------------------------------------------------
// The attempt without a histogram first (4-byte keys and payloads, 16 Mi .. 2^28 pairs: two MSB passes into slots and the pairs'
// leaves, which write (k, v) -- an attempt that is called off has only read them), the histogram-first kernels behind it gated
// on its verdict.
template <typename KT, typename VT>
int sort_pairs_inplace_async(Ctx &c, KT *k, KT *ks, VT *v, VT *vs, size_t n, int dtype, int order)
{
	RSX_TRY(async_enter(c, "rsx_sort_pairs_inplace_async"));
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (n * 2 * (sizeof(KT) + sizeof(VT)) <= SMALL_PAIR_BYTES) {
		hipLaunchKernelGGL((rsx_small_pairs_kernel<KT, VT, false>), dim3(1), dim3(1024), 0, c.stream, (const KT *)k, ks, v, vs, (u32)n,
		                   ka, c.dev_host_plan, true);
		HIP_TRY(hipGetLastError());
		c.async_small = true;
		return RSX_OK;
	}
	const size_t status_total = status_bytes<KT, VT>(n) * sizeof(KT);
	RSX_TRY(async_gated(
	    c,
	    [&](int *enqueued) -> int {
		    if constexpr (sizeof(KT) == 4 && sizeof(VT) == 4) {
			    if (async_pairs_blind_ok<KT>(c, n, sizeof(VT)))
				    RSX_TRY((pairs_blind_enqueue<KT, VT>(c, k, v, k, v, n, ka, enqueued, ks, vs)));
		    }
		    return RSX_OK;
	    },
	    [&]() -> int {
		    RSX_TRY(plan_phase<KT>(c, k, n, ka, nullptr, status_total));
		    for (u32 i = 0; i < sizeof(KT); ++i)
			    RSX_TRY((scatter_pass<KT, VT>(c, k, ks, v, vs, n, 0, c.ghist(), ka, 0, c.plan(), (int)i, i)));
		    return RSX_OK;
	    }));
	hipLaunchKernelGGL(rsx_copy_if_odd_kernel, dim3(2048), dim3(256), 0, c.stream, (unsigned char *)k, (const unsigned char *)ks,
	                   (u64)n * sizeof(KT), (const Plan *)c.plan());
	hipLaunchKernelGGL(rsx_copy_if_odd_kernel, dim3(2048), dim3(256), 0, c.stream, (unsigned char *)v, (const unsigned char *)vs,
	                   (u64)n * sizeof(VT), (const Plan *)c.plan());
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// ---- stable argsort: every pass is device-scheduled, the ranks always end in the FIRST half ------------------------------------
// radix_sort_rank.hpp:97-112 for callers that cannot wait (graphs, the multi-GPU chunk pipeline).  The number of passes is only
// known on the device, so the passes take their buffers from the plan (SCATTER_RANK_ASYNC): the last one writes the first
// half.  Keys travel at full width (which narrower type a pass could write is a choice of kernel, i.e. the host's).
// The attempt without a histogram first (4-byte keys, 4-byte indices, 16 Mi .. 2^28 keys: its leaves write the ranks to the
// first half), the histogram-first kernels behind it gated on its verdict -- as sort_keys_inplace_async.
template <typename KT, typename IT>
int sort_rank_inplace_async(Ctx &c, const KT *src, IT *ib, size_t n, int dtype, int order)
{
	RSX_TRY(async_enter(c, "rsx_sort_rank_inplace_async"));
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
	RSX_TRY(async_gated(
	    c,
	    [&](int *enqueued) -> int {
		    if constexpr (sizeof(KT) == 4 && sizeof(IT) == 4) {
			    if (async_pairs_blind_ok<KT>(c, n, sizeof(IT)))
				    RSX_TRY((pairs_blind_enqueue<KT, IT>(c, src, (const IT *)nullptr, (KT *)nullptr, ib, n, ka, enqueued, (KT *)(ib + n), ib)));
		    }
		    return RSX_OK;
	    },
	    [&]() -> int {
		    RSX_TRY(plan_phase<KT>(c, src, n, ka, nullptr, status_total));
		    c.pass_alt = c.keys[1].p;   // (to the end of the gated launches: GateScope)
		    for (u32 i = 0; i < sizeof(KT); ++i)   // pass i = the i-th kept column, if there is one
			    RSX_TRY((scatter_pass<KT, IT>(c, src, (KT *)c.keys[0].p, ib, ib + n, n, 0, c.ghist(), ka, SCATTER_RANK_ASYNC, c.plan(), (int)i, i)));
		    return RSX_OK;
	    }));
	// sorted keys: no pass ran, the ranks are 0 .. n-1 (radix_sort_rank.hpp:52,:55-57)
	hipLaunchKernelGGL((rsx_iota_if_sorted_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, ib, (u64)n, (const Plan *)c.plan());
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

}  // namespace
