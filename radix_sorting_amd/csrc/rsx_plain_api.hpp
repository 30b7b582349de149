// rsx_plain_api.hpp: the entry points of the three plain sorts -- rsx_sort[_device], rsx_sort_pairs_device, rsx_sort_rank[_device],
// their device-scheduled forms (*_inplace_async[_hint|_ws]) with rsx_async_route[_ws] and rsx_verify_poll, and the caller-owned
// workspace (rsx_workspace_bytes[_fast], borrow_ctx); part of librsx.so's host side, included by rsx.hip behind rsx_api.hpp.
#pragma once

namespace {

// A context whose device state lies in the caller's workspace (WsLayout, rsx_ws_layout.hpp).  Everything a captured graph of
// the *_ws entry points refers to is inside that workspace.
int borrow_ctx(Ctx &v, void *stream, void *ws, size_t ws_bytes, size_t n, const WsLayout &l)
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
	if (!ws || ws_bytes < l.minimal)
		return fail(RSX_EINVAL, "workspace of %zu bytes, %zu needed for %zu keys (rsx_workspace_bytes gives an upper bound)", ws_bytes, l.minimal, n);
	char *p = (char *)ws;
	v.device = dev;
	v.stream = (hipStream_t)stream;
	v.fast = true;
	v.small.borrow(p + l.flags_off, WS_FLAGS_BYTES);
	v.dev_host_plan = (Plan *)(p + l.plan2_off);
	v.host_plan = nullptr;
	v.hist.borrow(p + l.hist_off, l.hist_bytes);
	v.status.borrow(p + l.status_off, l.status_bytes);
	v.hpart.borrow(p + l.hpart_off, l.hpart_bytes);
	return RSX_OK;
}

// the layout of a keys-only sort's workspace: with the part of a sort without a histogram where one is attempted in a workspace
int ws_layout_keys(size_t n, rsx_dtype dtype, WsLayout *l)
{
	size_t status_total = 0;
	WsBlind blind;
	RSX_DISPATCH_KT(dtype, {
		status_total = status_bytes<KT, NoVal>(n) * sizeof(KT);
		if constexpr (sizeof(KT) >= 4)
			if (ws_blind_window(sizeof(KT), n))
				blind = blind_sizes<KT>(n);
	});
	*l = ws_layout_for(dtype_size(dtype), status_total, blind);
	return RSX_OK;
}

// rsx_sort_inplace_async[_hint]
int keys_inplace_async(const char *who, void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *stream, uint32_t hints)
{
	RSX_TRY(sort_args(who, dtype, n, d_buf && d_scratch));
	if (n < 2)
		return RSX_OK;
	RSX_ASYNC_CTX(c, stream);
	struct HintScope {   // (the sample kernel of the attempt enqueued by this call reads them: blind_enqueue)
		Ctx &c;
		HintScope(Ctx &c_, u32 h) : c(c_) { c.hints = h; }
		~HintScope() { c.hints = 0; }
	} hint_scope(*c, (u32)hints);
	RSX_DISPATCH_KT(dtype, return sort_keys_inplace_async<KT>(*c, (KT *)d_buf, (KT *)d_scratch, n, dtype, order));
	return RSX_OK;
}

// host arrays the one-launch kernels take (sort_keys_device, sort_rank_device: the same conditions)
bool host_small_path(const Ctx &c, size_t key_bytes)
{
	return c.fast && key_bytes <= SMALL_SORT_BYTES && !env().no_small_sort && !env().no_host_small && !capture_armed();
}

}  // namespace

extern "C" {

// an upper bound over the kernels' shapes (ws_status_bound), so that it holds for every payload a caller may pair the keys with
size_t rsx_workspace_bytes(size_t n, rsx_dtype dtype, size_t payload_bytes)
{
	const size_t kb = dtype_size(dtype);
	if (!kb)
		return 0;
	return ws_layout_for(kb, ws_status_bound(n, kb, payload_bytes)).bound();
}

size_t rsx_workspace_bytes_fast(size_t n, rsx_dtype dtype)
{
	const size_t kb = dtype_size(dtype);
	if (!kb)
		return 0;
	WsBlind blind;
	if (ws_blind_window(kb, n))
		blind = kb == 4 ? blind_sizes<u32>(n) : blind_sizes<u64>(n);
	return ws_layout_for(kb, ws_status_bound(n, kb, 0), blind).bound_fast();
}

int rsx_sort_inplace_async(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *stream)
{
	return keys_inplace_async("rsx_sort_inplace_async", d_buf, d_scratch, n, dtype, order, stream, 0);
}

int rsx_sort_inplace_async_hint(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *stream, uint32_t hints)
{
	return keys_inplace_async("rsx_sort_inplace_async_hint", d_buf, d_scratch, n, dtype, order, stream, hints);
}

int rsx_sort_inplace_async_ws(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order, void *d_workspace,
                              size_t workspace_bytes, void *stream)
{
	RSX_TRY(sort_args("rsx_sort_inplace_async_ws", dtype, n, d_buf && d_scratch));
	if (n < 2)
		return RSX_OK;
	Ctx view;
	WsLayout l;
	RSX_TRY(ws_layout_keys(n, dtype, &l));
	RSX_TRY(borrow_ctx(view, stream, d_workspace, workspace_bytes, n, l));
	// a workspace sized by rsx_workspace_bytes_fast also holds the slots of a sort without a histogram: the attempt is made in it
	borrow_blind(view, (char *)d_workspace, workspace_bytes, l);
	AsyncScope async_scope((hipStream_t)stream);
	RSX_DISPATCH_KT(dtype, return sort_keys_inplace_async<KT>(view, (KT *)d_buf, (KT *)d_scratch, n, dtype, order));
	return RSX_OK;
}

int rsx_async_route_ws(const void *d_workspace, size_t workspace_bytes, size_t n, rsx_dtype dtype, void *stream, uint32_t *route)
{
	const size_t kb = dtype_size(dtype);
	if (!route || !d_workspace || !kb)
		return fail(RSX_EINVAL, "rsx_async_route_ws: bad argument");
	*route = 0;
	HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
	WsLayout l;
	RSX_TRY(ws_layout_keys(n, dtype, &l));
	Plan plan;
	HIP_TRY(hipMemcpy(&plan, (const char *)d_workspace + l.plan_off, sizeof(plan), hipMemcpyDeviceToHost));
	// (a workspace of the size rsx_workspace_bytes_fast names: the attempt was made in it, its control block opens Ctx::seg)
	if (ws_blind_window(kb, n) && workspace_bytes >= rsx_workspace_bytes_fast(n, dtype)) {
		SegCtl ctl;
		HIP_TRY(hipMemcpy(&ctl, (const char *)d_workspace + l.seg_off, sizeof(ctl), hipMemcpyDeviceToHost));
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
	RSX_TRY(sort_args("rsx_sort_pairs_inplace_async_ws", dtype, n, d_keys && d_keys_scratch && d_vals && d_vals_scratch, payload_bytes));
	if (n < 2)
		return RSX_OK;
	Ctx view;
	size_t status_total = 0;
	RSX_DISPATCH_KT_W(dtype, payload_bytes, VT, status_total = (status_bytes<KT, VT>(n) * sizeof(KT)));
	RSX_TRY(borrow_ctx(view, stream, d_workspace, workspace_bytes, n, ws_layout_for(dtype_size(dtype), status_total)));
	RSX_DISPATCH_KT_W(dtype, payload_bytes, VT, return (sort_pairs_inplace_async<KT, VT>(view, (KT *)d_keys, (KT *)d_keys_scratch, (VT *)d_vals,
	                                                                                     (VT *)d_vals_scratch, n, dtype, order)));
	return RSX_OK;
}

int rsx_sort_pairs_inplace_async(void *d_keys, void *d_keys_scratch, void *d_vals, void *d_vals_scratch, size_t n, rsx_dtype dtype,
                                 size_t payload_bytes, rsx_order order, void *stream)
{
	RSX_TRY(sort_args("rsx_sort_pairs_inplace_async", dtype, n, d_keys && d_keys_scratch && d_vals && d_vals_scratch, payload_bytes));
	if (n < 2)
		return RSX_OK;
	RSX_ASYNC_CTX(c, stream);
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
	RSX_TRY(sort_args("rsx_sort_pairs_device", dtype, n, d_keys && d_keys_aux && d_vals && d_vals_aux, payload_bytes));
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
	RSX_TRY(sort_args("rsx_sort_rank_inplace_async", dtype, n, d_src && d_index_buffer, idx_bytes));
	if (idx_bytes == 4 && n > (1ull << 32))
		return fail(RSX_EINVAL, "rsx_sort_rank_inplace_async: n does not fit a 4-byte index");
	if (n == 0)
		return RSX_OK;                       // radix_sort_rank.hpp:28-32
	RSX_ASYNC_CTX(c, stream);
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
	// Host buffers.  Small arrays: the one-launch kernel reads the keys from pinned memory and writes the result there.  Others:
	// staged over PCIe, sorted in HBM.  Either way the result is brought into the buffer the returned-pointer rule names (the
	// other one is left as it was).
	const bool pinned = host_small_path(*c, n * kb);
	char *dsrc, *daux;
	if (pinned) {
		RSX_TRY(c->ensure_hstage());
		dsrc = c->hstage_dev;
		daux = c->hstage_dev + SMALL_SORT_BYTES;
	} else {
		RSX_TRY(c->keys[0].ensure(n * kb));
		RSX_TRY(c->keys[1].ensure(n * kb));
		dsrc = (char *)c->keys[0].p;
		daux = (char *)c->keys[1].p;
	}
	HostRegScope reg_src(src, n * kb), reg_aux(aux, n * kb);   // (RSX_HOST_REGISTER=1, arrays of a MiB and more: pinned until this call returns)
	if (pinned)
		memcpy(c->hstage, src, n * kb);
	else
		HIP_TRY(hipMemcpyAsync(dsrc, src, n * kb, hipMemcpyHostToDevice, c->stream));
	void *dres = nullptr;
	rsx_info li;
	RSX_TRY(rsx_sort_device(dsrc, daux, n, dtype, order, nullptr, &dres, &li));
	if (info)
		*info = li;
	void *hres = (!li.early_exit && li.result_in_aux) ? aux : src;
	if (pinned) {
		if (!li.early_exit)
			memcpy(hres, c->hstage + ((char *)dres - c->hstage_dev), n * kb);
	} else {
		if (!li.early_exit)
			HIP_TRY(hipMemcpyAsync(hres, dres, n * kb, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
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
