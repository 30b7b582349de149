// rsx_sort_plain.hpp: the blocking drivers of the three plain sorts -- keys (sort_keys_device), key + payload (sort_pairs_device),
// rank (sort_rank_device) -- and what they share: the RSX_VERIFY=2 bracket, the exit of the one-launch sorts, dispatch by key
// width; part of librsx.so's host side, included by rsx.hip behind the passes (launch_hist, plan_phase, scatter_pass) and the routes.
#pragma once

namespace {

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

// ---- RSX_VERIFY=2 ---------------------------------------------------------------------------------------------------------------
// The sort as it always runs (speculation, leaves, slack slots ...), bracketed by a check kernel "before" and one "after": each
// leaves [descents, sum, mix] in its three words, and the result must have no descent and the sum and mix of the input.
// (RSX_VERIFY=1 re-ranks a tile of every PASS and therefore keeps to the pass kernels; this one is blind to where an error came
// from but covers every route.)  A kind of sort's report -- n, the route, what is wrong, the descents, sum and mix -- and its words:
struct VerifyNouns {
	const char *report;
	const char *disorder, *altered;   // what is wrong: descents, or a sum or mix that differs
	const char *same, *differs;
};
constexpr VerifyNouns VERIFY_KEYS = {"RSX_VERIFY=2: the result of a sort of %zu keys (route %u) is %s: %llu descents, key sum %s, key mix %s",
                                     "not sorted", "not a permutation of the input", "kept", "changed"};
constexpr VerifyNouns VERIFY_PAIRS = {"RSX_VERIFY=2: the result of a key + payload sort of %zu pairs (route %u) is %s: %llu descents, key sum %s, pair mix %s",
                                      "not sorted", "not a permutation of the input's pairs", "kept", "changed"};
constexpr VerifyNouns VERIFY_RANKS = {"RSX_VERIFY=2: the ranks of a sort of %zu keys (route %u) are %s: %llu places out of order, rank sum %s, rank mix %s",
                                      "not the stable order", "not a permutation of 0 .. n-1", "right", "wrong"};

// before(words) and after(words) enqueue a check kernel each (`after` runs the sort first where it lies between them) and
// return an rsx error code; the route in the report is info's, once `after` has returned
template <typename Before, typename After>
int verify_bracket(Ctx &c, size_t n, const rsx_info *info, const VerifyNouns &w, Before before, After after)
{
	RSX_TRY(c.vsum.ensure(6 * sizeof(u64)));
	u64 *vs = (u64 *)c.vsum.p;
	HIP_TRY(hipMemsetAsync(vs, 0, 6 * sizeof(u64), c.stream));
	RSX_TRY(before(vs));
	HIP_TRY(hipGetLastError());
	RSX_TRY(after(vs + 3));
	HIP_TRY(hipGetLastError());
	u64 h[6];
	HIP_TRY(hipMemcpyAsync(h, vs, sizeof h, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	if (env().verify_inject)   // (test hook: the failure report end to end)
		h[5] ^= 1;
	if (h[3] != 0 || h[1] != h[4] || h[2] != h[5])
		return fail(RSX_EVERIFY, w.report, n, info ? info->hybrid : 0u, h[3] ? w.disorder : w.altered, (unsigned long long)h[3],
		            h[1] == h[4] ? w.same : w.differs, h[2] == h[5] ? w.same : w.differs);
	return RSX_OK;
}

// ---- the one-launch sorts (rsx_small.hpp) -----------------------------------------------------------------------------------------
// Behind the launch: the kernel has written the plan to pinned memory; the number of kept columns says where the result lies
// (radix_sort.hpp:92, radix_sort_rank.hpp:91; sorted input: no column, the first buffer).
inline int small_sort_exit(Ctx &c, rsx_info *info, bool *in_second)
{
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c.stream));
	const Plan p = *c.host_plan;
	info_from_plan(info, p);
	*in_second = (p.ncols & 1) != 0;
	if (info) {
		info->early_exit = p.sorted ? 2 : 0;
		info->result_in_aux = *in_second;
	}
	return RSX_OK;
}

// ---- dispatch by width ------------------------------------------------------------------------------------------------------------
// f(T()) for the unsigned type T of `bytes` bytes
template <typename F> int by_width(u32 bytes, F f)
{
	switch (bytes) {
	case 1: return f(uint8_t());
	case 2: return f(uint16_t());
	case 4: return f(u32());
	case 8: return f(u64());
	}
	return fail(RSX_EINVAL, "no key type of %u bytes", bytes);
}
inline int unsigned_dtype(size_t bytes) { return bytes == 1 ? RSX_U8 : bytes == 2 ? RSX_U16 : bytes == 4 ? RSX_U32 : RSX_U64; }

// ---- keys only -------------------------------------------------------------------
template <typename KT>
int sort_keys_device_impl(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void **result, rsx_info *info);

template <typename KT>
int sort_keys_device(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void **result, rsx_info *info)
{
	if (!env().verify_whole)
		return sort_keys_device_impl<KT>(c, src, aux, n, dtype, order, result, info);
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	auto check = [&](const KT *keys, u64 *words) {
		hipLaunchKernelGGL((rsx_checksum_kernel<KT>), dim3(2048), dim3(256), 0, c.stream, keys, (u64)n, ka, words);
		return (int)RSX_OK;
	};
	return verify_bracket(c, n, info, VERIFY_KEYS, [&](u64 *words) { return check(src, words); }, [&](u64 *words) {
		RSX_TRY(sort_keys_device_impl<KT>(c, src, aux, n, dtype, order, result, info));
		return check((const KT *)*result, words);
	});
}

// the sorted array written from one column's histogram into `aux` (a column the device-side plan names; it may say no)
template <typename KT> hipError_t launch_fill_runs(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka)
{
	const unsigned blocks = (unsigned)std::min<u64>((n * sizeof(KT) / 16 + 255) / 256 + 1, 8192);
	hipLaunchKernelGGL((rsx_fill_runs_kernel<KT>), dim3(blocks), dim3(256), 0, c.stream, aux, (u64)n, (const u64 *)c.ghist(),
	                   (const KT *)src, ka, (const Plan *)c.plan());
	return hipGetLastError();
}

// ... behind the fill kernels of 1- and 2-byte keys: the plan; sorted input ends the sort here (*sorted)
template <typename KT> int fill_plan(Ctx &c, KT *src, size_t n, Plan *plan, void **result, rsx_info *info, bool *sorted)
{
	RSX_TRY(plan_wait(c, plan));
	info_from_plan(info, *plan);
	RSX_TRY(capture_hist(c, n, sizeof(KT)));
	*sorted = plan->sorted != 0;
	return *sorted ? finish_sorted(info, result, src) : (int)RSX_OK;   // radix_sort.hpp:60-62
}

// The routes of a keys-only sort that need no plan of the ordinary kind, each "done / not mine" (*done = 1: *result and info are
// set) like sort_keys_blind (rsx_route_blind.hpp) and sort_keys_log above.

// the whole sort in one workgroup and one launch (rsx_small.hpp)
template <typename KT>
int sort_keys_small(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, void **result, rsx_info *info, int *done)
{
	if (!(c.fast && n * sizeof(KT) <= SMALL_SORT_BYTES && !env().no_small_sort && !capture_armed()))
		return RSX_OK;
	ProfScope prof(1, (u64)n * 2 * sizeof(KT), c.stream);
	hipLaunchKernelGGL((rsx_small_sort_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, src, aux, (u32)n, ka, c.dev_host_plan);
	bool in_aux = false;
	RSX_TRY(small_sort_exit(c, info, &in_aux));
	*result = in_aux ? aux : src;
	*done = 1;
	return RSX_OK;
}

// 1-byte keys: at most one column, so the sorted array is the histogram written out (rsx_fill_runs_kernel) -- a read
// and a write of the keys instead of a read, a read and a scatter
template <typename KT>
int sort_keys_fill8(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, void **result, rsx_info *info, int *done)
{
	if constexpr (sizeof(KT) == 1) {
		if (env().no_fill_runs || (((uintptr_t)aux) & 15) != 0)
			return RSX_OK;
		*done = 1;
		Plan plan;
		bool sorted = false;
		RSX_TRY(plan_phase<KT>(c, src, n, ka, nullptr, 0));
		HIP_TRY(launch_fill_runs<KT>(c, src, aux, n, ka));
		RSX_TRY(fill_plan<KT>(c, src, n, &plan, result, info, &sorted));
		if (sorted)
			return RSX_OK;
		*result = aux;                       // one pass: radix_sort.hpp:92
		if (info)
			info->result_in_aux = 1;
	}
	return RSX_OK;
}

// 2-byte keys, large arrays: one 16-bit digit.  The sorted array is written from the joint histogram of the two bytes
// (rsx_joint16_kernel ... rsx_fill16_kernel) into `src` -- where two passes end (radix_sort.hpp:92) --, from one
// byte's histogram into `aux` if only one column is kept; the device-side plan decides, no kernel scatters.
// (below 2^32 keys: the joint table counts in 32 bits, and one 16-bit value may occur n times; larger arrays take the
// two scatter passes, whose status words are 64-bit from 2^30 keys on -- counter width by n, radix_sort.hpp:102-114)
template <typename KT>
int sort_keys_fill16(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, void **result, rsx_info *info, int *done)
{
	if constexpr (sizeof(KT) == 2) {
		if (env().no_fill_runs || n < ((size_t)1 << 20) || n >= ((size_t)1 << 32) || ((((uintptr_t)aux) | ((uintptr_t)src)) & 15) != 0)
			return RSX_OK;
		*done = 1;
		Plan plan;
		bool sorted = false;
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
		HIP_TRY(launch_fill_runs<KT>(c, src, aux, n, ka));
		RSX_TRY(fill_plan<KT>(c, src, n, &plan, result, info, &sorted));
		if (sorted)
			return RSX_OK;
		*result = plan.ncols == 1 ? aux : src;
		if (info)
			info->result_in_aux = plan.ncols == 1;
	}
	return RSX_OK;
}

// One MSB pass (or two) and leaves where the plan says so: pass 0 went by the highest kept column; the leaves put the result
// where an LSB-first sort of plan.ncols passes ends.  spec_leaves: the leaf shapes that are on their way already.
template <typename KT>
int sort_keys_msb_leaves(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, const Plan &plan, u32 spec_leaves, bool self_planned,
                         void **result, rsx_info *info, int *done)
{
	if constexpr (sizeof(KT) >= 4) {
		if (plan.hyb != HYB_ONE_LEVEL && plan.hyb != HYB_TWO_LEVEL)
			return RSX_OK;
		*done = 1;
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
	}
	return RSX_OK;
}

// The histogram-first sort: the plan, then one pass per kept column (or the plan's MSB pass and leaves) -- with the first pass,
// and the leaves a mid-size array may want, enqueued before the host knows the plan.
template <typename KT>
int sort_keys_planned(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, void **result, rsx_info *info)
{
	Plan plan;
	// The first pass is enqueued before the host knows the plan (it reads the device's copy and does nothing on
	// sorted input): the host's wait for the plan, 20-25 us of idle GPU otherwise, hides behind it.
	const bool spec = c.fast && !env().no_speculation && !verify_mode();
	// with the fast kernel every pass has its own region of status words, all zeroed together with the histogram
	const size_t status_total = c.fast ? status_bytes<KT, NoVal>(n) * sizeof(KT) : 0;
	// One kept column (keys that differ in one byte only): the sorted array is written from the histogram instead of
	// scattered (rsx_fill_runs_kernel).  With a speculative first pass both kernels are enqueued and the device-side plan
	// decides which of them works, which costs an empty launch (3 us) in the usual case: only from 16 Mi keys on, where that is 1 %.
	const bool fill_one = sizeof(KT) > 1 && !env().no_fill_runs && (((uintptr_t)aux) & 15) == 0 && (!spec || n >= ((size_t)1 << 24));
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
			HIP_TRY(launch_fill_runs<KT>(c, src, aux, n, ka));
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
			HIP_TRY(launch_fill_runs<KT>(c, src, aux, n, ka));
		*result = aux;                       // one pass: radix_sort.hpp:92
		if (info)
			info->result_in_aux = 1;
		return RSX_OK;
	}
	int done = 0;
	RSX_TRY(sort_keys_msb_leaves<KT>(c, src, aux, n, ka, plan, spec_leaves, self_planned, result, info, &done));
	if (done)
		return RSX_OK;
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

// the ladder: each route takes the sort or leaves it to the next
template <typename KT>
int sort_keys_device_impl(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void **result, rsx_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	int done = 0;
	RSX_TRY(sort_keys_small<KT>(c, src, aux, n, ka, result, info, &done));
	if (!done)
		RSX_TRY(sort_keys_fill8<KT>(c, src, aux, n, ka, result, info, &done));
	if constexpr (sizeof(KT) >= 4) {
		// large arrays: two MSB passes and leaves without the histogram, where a sample of the keys allows it (rsx_hybrid.hpp)
		// 8-byte keys the byte columns do not spread (heavy-tailed magnitudes): digits of (bit length, mantissa), rsx_logroute.hpp
		KT *res = nullptr;
		if (!done && blind_wanted<KT>(c, n))
			RSX_TRY(sort_keys_blind<KT>(c, src, aux, n, ka, &res, info, &done));
		if (!done && log_wanted<KT>(c, n, src, aux))
			RSX_TRY(sort_keys_log<KT>(c, src, aux, n, ka, &res, info, &done));
		if (done && res)
			*result = res;
	}
	if (!done)
		RSX_TRY(sort_keys_fill16<KT>(c, src, aux, n, ka, result, info, &done));
	if (!done)
		RSX_TRY(sort_keys_planned<KT>(c, src, aux, n, ka, result, info));
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
	rsx_info local;   // (where the result lies is read from the info: a caller that gave none gets one here)
	memset(&local, 0, sizeof(local));
	rsx_info *inf = info ? info : &local;
	auto check = [&](const KT *keys, const VT *vals, u64 *words) {
		hipLaunchKernelGGL((rsx_checksum_pairs_kernel<KT, VT>), dim3(2048), dim3(256), 0, c.stream, keys, vals, (u64)n, ka, words);
		return (int)RSX_OK;
	};
	return verify_bracket(c, n, inf, VERIFY_PAIRS, [&](u64 *words) { return check(k0, v0, words); }, [&](u64 *words) {
		RSX_TRY((sort_pairs_device_impl<KT, VT>(c, k0, k1, v0, v1, n, dtype, order, inf)));
		return inf->result_in_aux ? check(k1, v1, words) : check(k0, v0, words);
	});
}

template <typename KT, typename VT>
int sort_pairs_device_impl(Ctx &c, KT *k0, KT *k1, VT *v0, VT *v1, size_t n, int dtype, int order, rsx_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	if (c.fast && n * 2 * (sizeof(KT) + sizeof(VT)) <= SMALL_PAIR_BYTES && !env().no_small_sort && !capture_armed()) {
		ProfScope prof(1, (u64)n * 2 * (sizeof(KT) + sizeof(VT)), c.stream);
		hipLaunchKernelGGL((rsx_small_pairs_kernel<KT, VT, false>), dim3(1), dim3(1024), 0, c.stream, (const KT *)k0, k1, v0, v1,
		                   (u32)n, ka, c.dev_host_plan);
		bool in_aux = false;
		return small_sort_exit(c, info, &in_aux);
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
		if (plan.hyb == HYB_ONE_LEVEL || plan.hyb == HYB_TWO_LEVEL) {
			// one MSB pass and the pairs' leaves (mid-size arrays) -- or two MSB passes (the second into slots) and leaves; on a
			// slot's overflow: one pass per column, from (k0, v0) again
			// (RSX_NO_SLACK=1: the second pass counted first and written to (k0, v0), which pass 1 has read; a bucket too large
			// for the leaves is known before that pass)
			const u32 top = plan.cols[plan.ncols - 1];
			RSX_TRY((scatter_pass<KT, VT>(c, k0, k1, v0, v1, n, 8 * top, c.ghist() + 256 * top, ka, 0u)));
			const bool in_aux = (plan.ncols & 1) != 0, one = plan.hyb == HYB_ONE_LEVEL;
			bool ok = true;
			if (one)
				RSX_TRY((pairs_one_level<KT, VT>(c, k1, v1, in_aux ? k1 : k0, in_aux ? v1 : v0, n, ka)));
			else
				RSX_TRY((pairs_two_level<KT, VT>(c, k1, v1, in_aux ? k1 : k0, in_aux ? v1 : v0, n, ka, &ok, k0, v0)));
			if (ok) {
				if (info) {
					info->result_in_aux = in_aux;
					info->hybrid = one ? 1 : env().no_slack ? 2 : 4;
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
	// (before: what 0 .. n-1 sum and mix to -- no keys, no ranks; after: the ranks themselves)
	auto check = [&](const KT *keys, const IT *ranks, u64 *words) {
		hipLaunchKernelGGL((rsx_check_ranks_kernel<KT, IT>), dim3(2048), dim3(256), 0, c.stream, keys, ranks, (u64)n, ka, words);
		return (int)RSX_OK;
	};
	return verify_bracket(c, n, info, VERIFY_RANKS, [&](u64 *words) { return check(nullptr, nullptr, words); },
	                      [&](u64 *words) { return check(src, (const IT *)*result, words); });
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
		bool second = false;
		RSX_TRY(small_sort_exit(c, info, &second));
		*result = second ? ib + n : ib;   // radix_sort_rank.hpp:91 (sorted: first half = iota)
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
		if (!plan.sorted && (plan.hyb == HYB_ONE_LEVEL || plan.hyb == HYB_TWO_LEVEL) && want_half < 0) {
			// mid-size arrays: one MSB pass of (key, index), which makes the indices, and the pairs' leaves write the ranks.
			// Keys spread over their top two columns (cfg 4 (i)): two MSB passes of (key, index) -- the first makes the indices,
			// the second goes into slots -- and leaves that write the ranks where the parity rule says (radix_sort_rank.hpp:91).
			// On a slot's overflow nothing has been written to that half: the ordinary passes follow.
			const u32 P = plan.ncols, top = plan.cols[P - 1];
			RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
			IT *fin = (P & 1) ? ib + n : ib, *scratch = (P & 1) ? ib : ib + n;
			RSX_TRY((scatter_pass<KT, IT>(c, src, (KT *)c.keys[0].p, (const IT *)fin, scratch, n, 8 * top, c.ghist() + 256 * top, ka,
			                              (u32)SCATTER_GEN_INDEX)));
			const bool one = plan.hyb == HYB_ONE_LEVEL;
			bool ok = true;
			if (one)
				RSX_TRY((pairs_one_level<KT, IT>(c, (const KT *)c.keys[0].p, (const IT *)scratch, (KT *)nullptr, fin, n, ka)));
			else
				RSX_TRY((pairs_two_level<KT, IT>(c, (const KT *)c.keys[0].p, (const IT *)scratch, (KT *)nullptr, fin, n, ka, &ok)));
			if (ok) {
				*result = fin;
				if (info) {
					info->result_in_aux = fin != ib;
					info->hybrid = one ? 1 : 4;
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
			rsx_info inner;
			const int half = (int)(P & 1);
			RSX_TRY(by_width(ob, [&](auto w) {
				typedef decltype(w) CK;   // the packed keys' type
				hipLaunchKernelGGL((rsx_compact_bits_kernel<KT, CK>), dim3(4096), dim3(256), 0, c.stream, src, (CK *)c.ckeys.p, (u64)n, ka, runs);
				return sort_rank_device<CK, IT>(c, (const CK *)c.ckeys.p, ib, n, unsigned_dtype(sizeof(CK)), RSX_ASCENDING, result, &inner, half);
			}));
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
		bool applied = false;   // (true exactly when in_bytes < sizeof(KT))
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
			RSX_TRY(by_width(in_bytes, [&](auto w) {
				typedef NarrowerOr<KT, decltype(w)> KCUR;   // (in_bytes == sizeof(KT): KT itself)
				return rank_pass<KCUR, KT, IT>(c, kin, kout, out_bytes, H[i & 1], H[(i + 1) & 1], n, shift, gb, ka, applied, flags, oshift);
			}));
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

}  // namespace
