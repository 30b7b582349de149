// rsx_locate_api.hpp: rsx_sort_locate[_device] -- the host driver (the count tables of 1- and 2-byte keys, the search over at most
// 4096 distinct values held in LDS, or sorts and binary searches, over the kernels of rsx_locate.hpp and rsx_rankdata.hpp) and its
// entry points; part of librsx.so's host side, included by rsx.hip behind rsx_nth_api.hpp.
#pragma once

namespace {

static_assert((unsigned)LOCATE_MAX_VALUES == (unsigned)RSX_LOCATE_MAX_SEARCH_VALUES, "rsx.h and rsx_locate_shape.hpp disagree");

// ---- rsx_sort_locate_device: where given values fall in the sorted order of the keys (rsx_locate.hpp) -------------
// what the call writes: each may be nullptr
template <typename IT> struct LocateOut {
	IT *less;    // m entries
	IT *equal;   // m entries
	IT *bin;     // n entries
	bool below;  // RSX_LOCATE_BINS_BELOW
};

// route 2, keys of 1 or 2 bytes: the counts of the derived keys (one byte: the histogram kernel; two: rsx_rankdata_count16_kernel),
// scanned; less / equal are rsx_rankdata_lookup_kernel over the VALUES in the keys' offsets, the bins the same kernel over the
// KEYS in the values' offsets (BELOW: its `less`; else the entry behind it).  *done = 0: no room, or too many for 32-bit counts.
template <typename KT, typename IT>
int locate_table(Ctx &c, const KT *src, size_t n, const KT *vals, size_t m, KdfArgs<KT> ka, const LocateOut<IT> &out, rsx_locate_info *info, int *done)
{
	*done = 0;
	if constexpr (sizeof(KT) <= 2) {
		constexpr bool ONE = sizeof(KT) == 1;
		constexpr size_t ENTRIES = ONE ? 256 : 65536;
		// per side (keys, values): [counts][offsets ENTRIES + 2]
		constexpr size_t CNT_BYTES = ONE ? 256 * sizeof(u64) + 256 : 65536 * sizeof(u32);
		constexpr size_t SIDE = CNT_BYTES + (ENTRIES + 2) * sizeof(u64);
		if ((u64)n >= (1ull << 32) || (u64)m >= (1ull << 32) || c.loctab.ensure(2 * SIDE) != RSX_OK)
			return RSX_OK;
		BitRuns runs = column_runs(0);
		if (!ONE)
			(void)bit_runs(0xFFFFull, &runs);
		// the exclusive offsets of the derived keys of a[0 .. count) in side `s`
		auto offsets = [&](const KT *a, size_t count, int s, u64 **offs) {
			char *base = (char *)c.loctab.p + (size_t)s * SIDE;
			*offs = (u64 *)(base + CNT_BYTES);
			HIP_TRY(hipMemsetAsync(base, 0, SIDE, c.stream));
			if constexpr (ONE) {
				RSX_TRY(launch_hist<KT>(c, a, count, ka, (u64 *)base, (u32 *)(base + 256 * sizeof(u64))));
				hipLaunchKernelGGL(rsx_locate_scan256_kernel, dim3(1), dim3(256), 0, c.stream, (const u64 *)base, *offs, (u64)count);
			} else {
				hipLaunchKernelGGL((rsx_rankdata_count16_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, a, (u64)count, ka, runs, (u32 *)base);
				hipLaunchKernelGGL(rsx_rankdata_scan16_kernel, dim3(1), dim3(1024), 0, c.stream, (const u32 *)base, *offs, (u64)count);
			}
			HIP_TRY(hipGetLastError());
			return (int)RSX_OK;
		};
		auto lookup = [&](const KT *a, size_t count, const u64 *offs, IT *o_less, IT *o_equal) {
			const unsigned grid = sweep_grid(count, sizeof(KT));
			// (the offsets are read from device memory for one byte too: the kernel's LDS form ends its table at the number of elements it looks up)
			hipLaunchKernelGGL((rsx_rankdata_lookup_kernel<KT, IT, false>), dim3(grid), dim3(1024), 0, c.stream, a, (u64)count, ka, runs, offs, o_less,
			                   o_equal);
			HIP_TRY(hipGetLastError());
			return (int)RSX_OK;
		};
		u64 *offs = nullptr;
		if (out.less || out.equal) {
			RSX_TRY(offsets(src, n, 0, &offs));
			RSX_TRY(lookup(vals, m, offs, out.less, out.equal));
			info->input_reads += 1;
		}
		if (out.bin) {
			RSX_TRY(offsets(vals, m, 1, &offs));
			RSX_TRY(lookup(src, n, out.below ? offs : offs + 1, out.bin, (IT *)nullptr));
			info->input_reads += 1;
		}
		info->route = RSX_LOCATE_TABLE;
		*done = 1;
	}
	return RSX_OK;
}

// the m values or edges of `src` in sorted order (a workspace copy through the ordinary keys-only sort): buf = [m][m] (locvals; partvals)
template <typename KT> int sorted_copy(Ctx &c, DevBuf &buf, const KT *src, size_t m, int dtype, int order, const KT **sorted)
{
	const size_t mpad = (m + 63) & ~(size_t)63;
	RSX_TRY(buf.ensure(2 * mpad * sizeof(KT)));
	KT *v0 = (KT *)buf.p, *v1 = v0 + mpad;
	HIP_TRY(hipMemcpyAsync(v0, src, m * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
	void *res = v0;
	if (m >= 2) {
		rsx_info si;
		info_clear(&si, dtype);
		RSX_TRY(sort_keys_device<KT>(c, v0, v1, m, dtype, order, &res, &si));
	}
	*sorted = (const KT *)res;
	return RSX_OK;
}

// where the parts of the search route's table lie in loctab
struct LocateTab {
	LocateHdr *hdr;
	u32 *start;
	u64 *cum, *tot, *rows;
	void *edges;
};
inline size_t locate_tab_bytes(u32 max_d, size_t key_bytes, u32 wgs)
{
	return 2048 + (((size_t)max_d * key_bytes + 7) & ~(size_t)7) + ((size_t)max_d + 1) * sizeof(u64) + (size_t)locate_counters(max_d) * sizeof(u64) * ((size_t)wgs + 1);
}
// the sorted values `sv` prepared for the search: the distinct ones as edges, their cumulative counts and the start table, and the
// header that says how many there are -- read back into *h, once the stream is through
template <typename KT>
int locate_prepared(Ctx &c, const KT *sv, size_t m, KdfArgs<KT> ka, u32 max_d, void *edges, u64 *cum, u32 *start, LocateHdr *hdr, LocateHdr *h)
{
	hipLaunchKernelGGL((rsx_locate_prepare_kernel<KT>), dim3(1), dim3(LOCATE_THREADS), 0, c.stream, sv, (u64)m, ka, max_d, (KT *)edges, cum, start, hdr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h, hdr, sizeof *h, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	return RSX_OK;
}
inline LocateTab locate_tab(void *p, u32 max_d, size_t key_bytes)
{
	LocateTab t;
	char *b = (char *)p;
	t.hdr = (LocateHdr *)b;
	t.start = (u32 *)(b + 256);
	t.edges = b + 2048;
	t.cum = (u64 *)(b + 2048 + (((size_t)max_d * key_bytes + 7) & ~(size_t)7));
	t.tot = t.cum + max_d + 1;
	t.rows = t.tot + locate_counters(max_d);
	return t;
}

// route 3, keys of 4 or 8 bytes.  The values are sorted and prepared (*sv: they stay sorted for the sort route); *done = 0: more
// than the cut-off distinct values, or no room.
template <typename KT, typename IT>
int locate_search_route(Ctx &c, const KT *src, size_t n, const KT *vals, size_t m, int dtype, int order, const LocateOut<IT> &out,
                        rsx_locate_info *info, const KT **sv, int *done)
{
	*done = 0;
	if constexpr (sizeof(KT) >= 4) {
		const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
		const u32 max_d = env().locate_max_values;
		const u64 head = std::min<u64>(n, ((16u - (u32)((uintptr_t)src & 15u)) & 15u) / sizeof(KT));
		const LocateGrid g = locate_grid((u64)n - head);
		if ((out.bin && (u64)m > 0xFFFFFFFFull && sizeof(IT) == 4) || c.loctab.ensure(locate_tab_bytes(max_d, sizeof(KT), g.wgs)) != RSX_OK ||
		    c.locvals.ensure(2 * ((m + 63) & ~(size_t)63) * sizeof(KT)) != RSX_OK)
			return RSX_OK;
		RSX_TRY(sorted_copy<KT>(c, c.locvals, vals, m, dtype, order, sv));
		const LocateTab t = locate_tab(c.loctab.p, max_d, sizeof(KT));
		LocateHdr h;
		RSX_TRY(locate_prepared<KT>(c, *sv, m, ka, max_d, t.edges, t.cum, t.start, t.hdr, &h));
		info->distinct_values = h.distinct;
		if (h.distinct == 0 || h.distinct > max_d)
			return RSX_OK;
		const LocateLds lds = locate_lds(h.distinct, (u32)sizeof(KT), (u32)sizeof(IT), out.bin != nullptr, env().locate_counter_sets);
		const u32 ncnt = locate_counters(h.distinct);
#define RSX_LOCATE_LAUNCH(WANT, BELOW)                                                                                              \
		hipLaunchKernelGGL((rsx_locate_search_kernel<KT, IT, WANT, BELOW>), dim3(g.wgs), dim3(LOCATE_THREADS), 0, c.stream, src, (u64)n, ka, \
		                   (const KT *)t.edges, (const u64 *)t.cum, (const u32 *)t.start, h.distinct, h.shift, h.steps, lds, g.share_tiles, \
		                   locate_flush_tiles(), t.rows, out.bin)
		if (!out.bin)
			RSX_LOCATE_LAUNCH(false, false);
		else if (out.below)
			RSX_LOCATE_LAUNCH(true, true);
		else
			RSX_LOCATE_LAUNCH(true, false);
#undef RSX_LOCATE_LAUNCH
		HIP_TRY(hipGetLastError());
		if (out.less || out.equal) {
			hipLaunchKernelGGL(rsx_locate_colsum_kernel, dim3((ncnt + 63u) / 64u), dim3(1024), 0, c.stream, (const u64 *)t.rows, g.wgs, ncnt, t.tot);
			hipLaunchKernelGGL((rsx_locate_finish_kernel<KT, IT>), dim3(small_grid(m, 1024, 1024)), dim3(1024), 0, c.stream, vals, (u64)m, ka,
			                   (const KT *)t.edges, h.distinct, (const u64 *)t.tot, out.less, out.equal);
			HIP_TRY(hipGetLastError());
		}
		info->route = RSX_LOCATE_SEARCH;
		info->input_reads = 1;
		info->search_steps = h.steps;
		info->counter_sets = lds.sets;
		*done = 1;
	}
	return RSX_OK;
}

// route 4: a workspace copy of the keys through the ordinary keys-only sort (none where the keys are in order already) and two
// binary searches per value; for the bins the values sorted (`sv`: they are already) and one binary search per key
template <typename KT, typename IT>
int locate_by_sort(Ctx &c, const KT *src, size_t n, const KT *vals, size_t m, int dtype, int order, const LocateOut<IT> &out, const KT *sv,
                   rsx_locate_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	info->route = RSX_LOCATE_SORT;
	info->input_reads = 0;
	info->search_steps = info->counter_sets = 0;
	if (out.less || out.equal) {
		const KT *sk = src;
		u32 descents = 0;
		if (n >= 2) {
			RSX_TRY(c.urecs.ensure(64));
			u32 *flag = (u32 *)c.urecs.p;
			HIP_TRY(hipMemsetAsync(flag, 0, sizeof(u32), c.stream));
			hipLaunchKernelGGL((rsx_locate_descents_kernel<KT>), dim3(small_grid(n, 256 * 16, 1024)), dim3(256), 0, c.stream, src, (u64)n, ka, flag);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(&descents, flag, sizeof descents, hipMemcpyDeviceToHost, c.stream));
			HIP_TRY(hipStreamSynchronize(c.stream));
		}
		if (descents) {
			RSX_TRY(keybits_keys_sort<KT>(c, src, n, dtype, order, &info->sort, &sk));
		} else {
			info->sort.early_exit = n < 2 ? 1 : 2;
		}
		hipLaunchKernelGGL((rsx_locate_sorted_values_kernel<KT, IT>), dim3(small_grid(m, 256, 1024)), dim3(256), 0, c.stream, sk, (u64)n, vals, (u64)m,
		                   ka, out.less, out.equal);
		HIP_TRY(hipGetLastError());
	}
	if (out.bin) {
		if (!sv)
			RSX_TRY(sorted_copy<KT>(c, c.locvals, vals, m, dtype, order, &sv));
		const u64 block = ((u64)m + 4095) / 4096;
		const unsigned grid = small_grid(n, 1024 * 8, 1024);
		if (out.below)
			hipLaunchKernelGGL((rsx_locate_sorted_bins_kernel<KT, IT, true>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, sv, (u64)m, block, ka, out.bin);
		else
			hipLaunchKernelGGL((rsx_locate_sorted_bins_kernel<KT, IT, false>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, sv, (u64)m, block, ka, out.bin);
		HIP_TRY(hipGetLastError());
	}
	return RSX_OK;
}

template <typename KT, typename IT>
int sort_locate_device(Ctx &c, const KT *src, size_t n, const KT *vals, size_t m, int dtype, int order, const LocateOut<IT> &out,
                       rsx_locate_info *info)
{
	const KT *sv = nullptr;
	if (env().locate_force != 2) {
		int done = 0;
		if (sizeof(KT) <= 2)
			RSX_TRY((locate_table<KT, IT>(c, src, n, vals, m, make_kdf<KT>(dtype, order), out, info, &done)));
		else
			RSX_TRY((locate_search_route<KT, IT>(c, src, n, vals, m, dtype, order, out, info, &sv, &done)));
		if (done)
			return RSX_OK;
	}
	return locate_by_sort<KT, IT>(c, src, n, vals, m, dtype, order, out, sv, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_locate: where given values fall in the sorted order (rsx_locate.hpp) ---- */
static int locate_args(const char *who, const void *src, size_t n, const void *vals, size_t m, rsx_dtype dtype, rsx_order order, const void *less,
                       const void *equal, const void *bin, size_t idx_bytes, uint32_t flags)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || (n && !src) || (m && !vals) || (flags & ~(uint32_t)RSX_LOCATE_BINS_BELOW))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!less && !equal && !bin)
		return fail(RSX_EINVAL, "%s: all three outputs are NULL", who);
	RSX_TRY(idx_args(who, idx_bytes, n, (less || equal) ? n : 0));   // (less and equal may be n itself)
	if (bin && idx_bytes == 4 && (uint64_t)m > 0xFFFFFFFFull)
		return fail(RSX_EINVAL, "%s: m = %zu does not fit a 4-byte index", who, m);
	return RSX_OK;
}

// nothing to compute and nothing to write: no values and no bins wanted (or no keys to write bins for)
static bool locate_nothing(size_t n, size_t m, const void *bin) { return m == 0 && (!bin || n == 0); }

int rsx_sort_locate_device(const void *d_src, size_t n, const void *d_vals, size_t m, rsx_dtype dtype, rsx_order order, void *d_less,
                           void *d_equal, void *d_bin, size_t idx_bytes, uint32_t flags, void *stream, rsx_locate_info *info)
{
	rsx_locate_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	RSX_TRY(locate_args("rsx_sort_locate_device", d_src, n, d_vals, m, dtype, order, d_less, d_equal, d_bin, idx_bytes, flags));
	if (locate_nothing(n, m, d_bin))
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_locate_device", "the call waits for the number of distinct values"));
	if (n == 0 || m == 0) {
		// (no keys: nothing is below or equal to any value; no values: every key falls in bin 0)
		if (d_less && m)
			HIP_TRY(hipMemsetAsync(d_less, 0, m * idx_bytes, c->stream));
		if (d_equal && m)
			HIP_TRY(hipMemsetAsync(d_equal, 0, m * idx_bytes, c->stream));
		if (d_bin && n)
			HIP_TRY(hipMemsetAsync(d_bin, 0, n * idx_bytes, c->stream));
		return RSX_OK;
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_locate_device<KT, IT>(*c, (const KT *)d_src, n, (const KT *)d_vals, m, dtype, order,
	                                                     LocateOut<IT>{(IT *)d_less, (IT *)d_equal, (IT *)d_bin, (flags & RSX_LOCATE_BINS_BELOW) != 0},
	                                                     info)));
	return RSX_OK;
}

int rsx_sort_locate(const void *src, size_t n, const void *vals, size_t m, rsx_dtype dtype, rsx_order order, void *less, void *equal, void *bin,
                    size_t idx_bytes, uint32_t flags, rsx_locate_info *info)
{
	rsx_locate_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(locate_args("rsx_sort_locate", src, n, vals, m, dtype, order, less, equal, bin, idx_bytes, flags));
	if (locate_nothing(n, m, bin))
		return RSX_OK;
	RSX_LOCKED_CTX(c, nullptr);
	const size_t mb = m * idx_bytes, nb = n * idx_bytes;
	const StageRow rows[5] = {{src, n * kb, n * kb, STAGE_RECS0}, {vals, m * kb, m * kb}, {less, 0, mb}, {equal, 0, mb}, {bin, 0, nb}};
	return staged_call(*c, "rsx_sort_locate", rows, [&](void *const *d, size_t *back) {
		back[2] = back[3] = mb, back[4] = nb;
		return rsx_sort_locate_device(d[0], n, d[1], m, dtype, order, d[2], d[3], d[4], idx_bytes, flags, nullptr, info);
	});
}

}  // extern "C"
