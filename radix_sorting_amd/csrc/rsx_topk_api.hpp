// rsx_topk_api.hpp: rsx_sort_topk[_device] -- the host driver (MSD radix select over the kernels of rsx_topk.hpp, or the rank sort)
// and its entry points; part of librsx.so's host side, included by rsx.hip behind the routes and rsx_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_topk_device: the first k of the stable sorted order by MSD radix select (rsx_topk.hpp) --------------------
// Default route: select from TOPK_MIN_N keys on while k <= n / TOPK_MAX_K_DIV; the ordinary rank sort otherwise.
// The candidate buffer takes a selected bucket of at most n / 8 + 1024 elements (topk_cap); a larger one is narrowed by
// further histograms over the input.
constexpr size_t TOPK_MIN_N = (size_t)1 << 18, TOPK_MAX_K_DIV = 8;
inline size_t topk_cap(size_t n) { return n / 8 + 1024; }

struct TopkLayout {
	u64 groups, chunk;     // the input: workgroups and elements of each one's range
	u64 cgroups, cchunk;   // the candidate buffer at its capacity
	size_t rows, crows, goff, cgoff, bytes;
};

template <typename KT> TopkLayout topk_layout(size_t n)
{
	const u64 tile = topk_tile<KT>();
	auto split = [&](u64 m, u64 *groups, u64 *chunk) {
		const u64 tiles = std::max<u64>(1, (m + tile - 1) / tile);
		*groups = std::min<u64>(TOPK_MAX_GROUPS, tiles);
		*chunk = (tiles + *groups - 1) / *groups * tile;
	};
	TopkLayout L;
	split(n, &L.groups, &L.chunk);
	split(topk_cap(n), &L.cgroups, &L.cchunk);
	L.rows = sizeof(TopkCtl);
	L.crows = L.rows + (size_t)L.groups * TOPK_ROW * sizeof(u32);
	L.goff = L.crows + (size_t)L.cgroups * TOPK_ROW * sizeof(u32);
	L.cgoff = L.goff + (size_t)L.groups * 2 * sizeof(u64);
	L.bytes = L.cgoff + (size_t)L.cgroups * 2 * sizeof(u64);
	return L;
}

inline void topk_info_from_ctl(rsx_topk_info *info, const TopkCtl &h)
{
	info->input_reads = h.input_reads;
	info->digit_passes = h.digit_passes;
	info->n_less = h.n_less;
	info->n_equal = h.bucket;
	info->kth_key = h.kth_raw;
}

// *done = 0: no room for the buffers (not an error: the caller takes the sort route)
template <typename KT, typename IT>
int topk_select(Ctx &c, const KT *src, size_t n, size_t k, int dtype, int order, KT *out_keys, IT *out_idx, rsx_topk_info *info, int *done)
{
	*done = 0;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const TopkLayout L = topk_layout<KT>(n);
	const size_t cap = topk_cap(n);
	const size_t kpad = (k + 15) & ~(size_t)15, cpad = (cap + 15) & ~(size_t)15;   // (every array a multiple of 16 bytes)
	if (c.tkctl.ensure(L.bytes) != RSX_OK || c.tkpairs.ensure(2 * kpad * (sizeof(KT) + sizeof(IT))) != RSX_OK ||
	    c.tkcand.ensure(cpad * (sizeof(KT) + sizeof(IT))) != RSX_OK)
		return RSX_OK;
	char *base = (char *)c.tkctl.p;
	TopkCtl *ctl = (TopkCtl *)base;
	u32 *rows = (u32 *)(base + L.rows), *crows = (u32 *)(base + L.crows);
	u64 *goff = (u64 *)(base + L.goff), *cgoff = (u64 *)(base + L.cgoff);
	KT *pk = (KT *)c.tkpairs.p, *pk2 = pk + kpad;
	IT *pi = (IT *)(pk2 + kpad), *pi2 = pi + kpad;
	KT *ck = (KT *)c.tkcand.p;
	IT *ci = (IT *)(ck + cpad);
	(void)ck, (void)ci, (void)crows, (void)cgoff;   // (1-byte keys never fill candidates)
	TopkCtl h;
	memset(&h, 0, sizeof h);
	h.k_rem = k;
	HIP_TRY(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, c.stream));
	const dim3 grid((unsigned)L.groups), cgrid((unsigned)L.cgroups), threads(TOPK_THREADS);
	const dim3 rgrid((unsigned)((L.groups + 15) / 16)), crgrid((unsigned)((L.cgroups + 15) / 16));
	const u32 top = 8 * ((u32)sizeof(KT) - 1);
	// the top digit of every key; a bucket that fits the candidate buffer is moved there by one more pass over the input
	hipLaunchKernelGGL((rsx_topk_hist_kernel<KT, 0>), grid, threads, 0, c.stream, src, (u64)n, ka, ctl, rows, L.chunk, top);
	hipLaunchKernelGGL((rsx_topk_pick_kernel<KT>), dim3(1), dim3(256), 0, c.stream, ctl, top, (u64)cap, sizeof(KT) > 1 ? 1u : 0u, ka);
	if constexpr (sizeof(KT) > 1) {
		hipLaunchKernelGGL(rsx_topk_rows_kernel, rgrid, dim3(1024), 0, c.stream, (const TopkCtl *)ctl, (const u32 *)rows, (u32)L.groups, top,
		                   1u, goff);
		hipLaunchKernelGGL((rsx_topk_write_kernel<KT, IT, 0, 0>), grid, threads, 0, c.stream, src, (const IT *)nullptr, (u64)n, ka, ctl,
		                   (const u64 *)goff, L.chunk, pk, pi, (u64)k, ck, ci, (u64)cap);
		// the other digits: in the candidates (mode 1), or in the input under the prefix (mode 0) -- each kernel knows which
		for (u32 shift = top - 8;; shift -= 8) {
			hipLaunchKernelGGL((rsx_topk_hist_kernel<KT, 0>), grid, threads, 0, c.stream, src, (u64)n, ka, ctl, rows, L.chunk, shift);
			hipLaunchKernelGGL((rsx_topk_hist_kernel<KT, 1>), cgrid, threads, 0, c.stream, (const KT *)ck, (u64)0, ka, ctl, crows, L.cchunk,
			                   shift);
			hipLaunchKernelGGL((rsx_topk_pick_kernel<KT>), dim3(1), dim3(256), 0, c.stream, ctl, shift, (u64)cap, 0u, ka);
			if (!shift)
				break;
		}
	}
	// the final filter: exactly k pairs -- everything below the k-th key, then the first k - n_less elements equal to it
	hipLaunchKernelGGL(rsx_topk_rows_kernel, rgrid, dim3(1024), 0, c.stream, (const TopkCtl *)ctl, (const u32 *)rows, (u32)L.groups, 0u, 0u,
	                   goff);
	hipLaunchKernelGGL((rsx_topk_write_kernel<KT, IT, 0, 1>), grid, threads, 0, c.stream, src, (const IT *)nullptr, (u64)n, ka, ctl,
	                   (const u64 *)goff, L.chunk, pk, pi, (u64)k, (KT *)nullptr, (IT *)nullptr, (u64)0);
	if constexpr (sizeof(KT) > 1) {
		hipLaunchKernelGGL(rsx_topk_rows_kernel, crgrid, dim3(1024), 0, c.stream, (const TopkCtl *)ctl, (const u32 *)crows, (u32)L.cgroups,
		                   0u, 1u, cgoff);
		hipLaunchKernelGGL((rsx_topk_write_kernel<KT, IT, 1, 1>), cgrid, threads, 0, c.stream, (const KT *)ck, (const IT *)ci, (u64)0, ka, ctl,
		                   (const u64 *)cgoff, L.cchunk, pk, pi, (u64)k, (KT *)nullptr, (IT *)nullptr, (u64)0);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(&h, ctl, offsetof(TopkCtl, table), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	topk_info_from_ctl(info, h);
	// the k pairs sorted by the library's stable sorts (their scratch is the context's other buffers), and copied out
	KT *rk = pk;
	IT *ri = pi;
	if (k > 1) {
		rsx_info si;
		info_clear(&si, dtype);
		if (out_idx) {
			RSX_TRY((sort_pairs_device<KT, IT>(c, pk, pk2, pi, pi2, k, dtype, order, &si)));
			if (si.result_in_aux) {
				rk = pk2;
				ri = pi2;
			}
		} else {
			void *res = nullptr;
			RSX_TRY(sort_keys_device<KT>(c, pk, pk2, k, dtype, order, &res, &si));
			rk = (KT *)res;
		}
	}
	if (out_keys)
		HIP_TRY(hipMemcpyAsync(out_keys, rk, k * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
	if (out_idx)
		HIP_TRY(hipMemcpyAsync(out_idx, ri, k * sizeof(IT), hipMemcpyDeviceToDevice, c.stream));
	info->route = RSX_TOPK_SELECT;
	*done = 1;
	return RSX_OK;
}

// the sort route: rsx_sort_rank_device's machinery on a workspace copy, the first k ranks and the keys gathered through them
template <typename KT, typename IT>
int topk_by_sort(Ctx &c, const KT *src, size_t n, size_t k, int dtype, int order, KT *out_keys, IT *out_idx, rsx_topk_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	RSX_TRY(c.vals[0].ensure(2 * n * sizeof(IT)));
	RSX_TRY(c.tkctl.ensure(sizeof(TopkCtl)));
	TopkCtl *ctl = (TopkCtl *)c.tkctl.p;
	void *res = nullptr;
	rsx_info ri;
	info_clear(&ri, dtype);
	RSX_TRY((sort_rank_device<KT, IT>(c, src, (IT *)c.vals[0].p, n, dtype, order, &res, &ri)));
	HIP_TRY(hipMemsetAsync(ctl, 0, offsetof(TopkCtl, table), c.stream));
	hipLaunchKernelGGL((rsx_topk_gather_kernel<KT, IT>), dim3((unsigned)std::min<u64>(1024, ((u64)k + 255) / 256)), dim3(256), 0, c.stream, src,
	                   (const IT *)res, (u64)k, out_keys, out_idx, ka, ctl);
	const u64 sweep = (u64)TOPK_THREADS * (16 / sizeof(KT));
	hipLaunchKernelGGL((rsx_topk_count_kernel<KT>), dim3((unsigned)std::min<u64>(1024, ((u64)n + sweep - 1) / sweep)), dim3(TOPK_THREADS), 0,
	                   c.stream, src, (u64)n, ka, ctl);
	HIP_TRY(hipGetLastError());
	TopkCtl h;
	HIP_TRY(hipMemcpyAsync(&h, ctl, offsetof(TopkCtl, table), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	topk_info_from_ctl(info, h);
	info->route = RSX_TOPK_SORT;
	return RSX_OK;
}

template <typename KT, typename IT>
int sort_topk_device(Ctx &c, const KT *src, size_t n, size_t k, int dtype, int order, KT *out_keys, IT *out_idx, rsx_topk_info *info)
{
	const unsigned force = env().topk_force;
	if (force == 1 || (force == 0 && n >= TOPK_MIN_N && k <= n / TOPK_MAX_K_DIV)) {
		int done = 0;
		RSX_TRY((topk_select<KT, IT>(c, src, n, k, dtype, order, out_keys, out_idx, info, &done)));
		if (done)
			return RSX_OK;
	}
	return topk_by_sort<KT, IT>(c, src, n, k, dtype, order, out_keys, out_idx, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_topk: the first k of the sorted order (rsx_topk.hpp) ---- */
static int topk_args(const char *who, const void *src, size_t n, size_t k, rsx_dtype dtype, rsx_order order, const void *out_keys,
                     const void *out_idx, size_t idx_bytes)
{
	RSX_TRY(select_args(who, src, n, dtype, order, out_keys, out_idx, idx_bytes));
	if (k > n)
		return fail(RSX_EINVAL, "%s: k exceeds n (k = %zu, n = %zu)", who, k, n);
	return RSX_OK;
}

int rsx_sort_topk_device(const void *d_src, size_t n, size_t k, rsx_dtype dtype, rsx_order order, void *d_out_keys, void *d_out_idx,
                         size_t idx_bytes, void *stream, rsx_topk_info *info)
{
	rsx_topk_info local;
	info = info_or(info, &local);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	RSX_TRY(topk_args("rsx_sort_topk_device", d_src, n, k, dtype, order, d_out_keys, d_out_idx, idx_bytes));
	if (k == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_topk_device", "the call waits for what the selection found"));
	if (n == 1) {
		// (one key: itself, at index 0)
		const size_t kb = dtype_size(dtype);
		uint64_t key = 0;
		HIP_TRY(hipMemcpyAsync(&key, d_src, kb, hipMemcpyDeviceToHost, c->stream));
		if (d_out_keys)
			HIP_TRY(hipMemcpyAsync(d_out_keys, d_src, kb, hipMemcpyDeviceToDevice, c->stream));
		if (d_out_idx)
			HIP_TRY(hipMemsetAsync(d_out_idx, 0, idx_bytes, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		info->n_equal = 1;
		info->kth_key = key;   // (little-endian: the low kb bytes)
		return RSX_OK;
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_topk_device<KT, IT>(*c, (const KT *)d_src, n, k, dtype, order, (KT *)d_out_keys, (IT *)d_out_idx, info)));
	return RSX_OK;
}

int rsx_sort_topk(const void *src, size_t n, size_t k, rsx_dtype dtype, rsx_order order, void *out_keys, void *out_idx, size_t idx_bytes,
                  rsx_topk_info *info)
{
	rsx_topk_info local;
	info = info_or(info, &local);
	const size_t kb = dtype_size(dtype);
	info->key_bytes = (uint32_t)kb;
	RSX_TRY(topk_args("rsx_sort_topk", src, n, k, dtype, order, out_keys, out_idx, idx_bytes));
	if (k == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, nullptr);
	const StageRow rows[3] = {{src, n * kb, n * kb, STAGE_RECS0}, {out_keys, 0, k * kb}, {out_idx, 0, k * idx_bytes}};
	return staged_call(*c, "rsx_sort_topk", rows, [&](void *const *d, size_t *back) {
		back[1] = k * kb, back[2] = k * idx_bytes;
		return rsx_sort_topk_device(d[0], n, k, dtype, order, d[1], d[2], idx_bytes, nullptr, info);
	});
}

}  // extern "C"
