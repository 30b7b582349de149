// rsx_nth_api.hpp: rsx_sort_nth[_device] -- the host driver (multi-rank MSD radix select over the kernels of rsx_nth.hpp, or the rank
// sort) and its entry points; part of librsx.so's host side, included by rsx.hip behind the routes and rsx_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_nth_device: the elements at given ranks of the stable sorted order by multi-rank MSD radix select (rsx_nth.hpp) ----
// Default route: select from NTH_MIN_N keys on while there are at most RSX_NTH_MAX_SELECT_RANKS distinct ranks; the
// ordinary rank sort otherwise.  The candidate buffer takes active buckets of together at most n / 8 + 1024 elements (nth_cap);
// larger ones are narrowed by further histograms over the input.
constexpr size_t NTH_MIN_N = (size_t)1 << 18;
inline size_t nth_cap(size_t n) { return n / 8 + 1024; }
static_assert((unsigned)NTH_MAX_RANKS == (unsigned)RSX_NTH_MAX_SELECT_RANKS, "rsx.h and rsx_nth.hpp disagree");

// what the call asks for, prepared by the entry point: the distinct ranks ascending, and the record of each caller position
struct NthAsk {
	const uint64_t *ranks;
	size_t m;
	std::vector<u64> distinct;
	std::vector<u32> map;
	uint64_t *n_less, *n_equal;
};

struct NthIo {
	u64 *ranks, *nless, *nequal;
	u32 *map;
};
inline int nth_io(Ctx &c, size_t m, NthIo *io)
{
	RSX_TRY(c.nthio.ensure(m * (3 * sizeof(u64) + sizeof(u32))));
	io->ranks = (u64 *)c.nthio.p;
	io->nless = io->ranks + m;
	io->nequal = io->nless + m;
	io->map = (u32 *)(io->nequal + m);
	return RSX_OK;
}

// (behind the kernel that wrote them) the two host arrays; the call returns with them complete, and with the caller's rank
// list no longer in use
inline int nth_results_back(Ctx &c, const NthAsk &ask, const NthIo &io)
{
	if (ask.n_less)
		HIP_TRY(hipMemcpyAsync(ask.n_less, io.nless, ask.m * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
	if (ask.n_equal)
		HIP_TRY(hipMemcpyAsync(ask.n_equal, io.nequal, ask.m * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	return RSX_OK;
}

// *done = 0: no room for the buffers, or a wanted key occurs too often for the candidate buffer and indices are wanted (neither
// is an error: the caller takes the sort route)
template <typename KT, typename IT>
int nth_select(Ctx &c, const KT *src, size_t n, const NthAsk &ask, int dtype, int order, KT *out_keys, IT *out_idx, rsx_nth_info *info,
               int *done)
{
	*done = 0;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u64 tile = nth_tile<KT>();
	const u64 tiles = std::max<u64>(1, ((u64)n + tile - 1) / tile);
	const u64 groups = std::min<u64>(NTH_MAX_GROUPS, tiles);
	const u64 chunk = (tiles + groups - 1) / groups * tile;
	const size_t cap = nth_cap(n), cpad = (cap + 15) & ~(size_t)15;   // (every array a multiple of 16 bytes)
	const size_t table_bytes = (size_t)NTH_MAX_RANKS * 256 * sizeof(u64);
	const size_t m = ask.m, nd = ask.distinct.size();
	NthIo io;
	if (c.nthctl.ensure(sizeof(NthCtl) + table_bytes + (size_t)groups * sizeof(u64)) != RSX_OK ||
	    c.nthcand.ensure(2 * cpad * (sizeof(KT) + (out_idx ? sizeof(IT) : 0))) != RSX_OK || nth_io(c, m, &io) != RSX_OK)
		return RSX_OK;
	char *base = (char *)c.nthctl.p;
	NthCtl *ctl = (NthCtl *)base;
	u64 *table = (u64 *)(base + sizeof(NthCtl));
	u64 *goff = table + (size_t)NTH_MAX_RANKS * 256;
	KT *ck = (KT *)c.nthcand.p, *ck2 = ck + cpad;
	IT *ci = out_idx ? (IT *)(ck2 + cpad) : nullptr, *ci2 = out_idx ? ci + cpad : nullptr;
	NthCtl h;
	memset(&h, 0, sizeof h);
	h.nrec = (u32)nd;
	h.nact = 1;
	h.act_size[0] = n;
	for (size_t r = 0; r < nd; ++r)
		h.rec[r].k_rem = ask.distinct[r];
	HIP_TRY(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, c.stream));
	HIP_TRY(hipMemsetAsync(table, 0, table_bytes, c.stream));
	HIP_TRY(hipMemcpyAsync(io.map, ask.map.data(), m * sizeof(u32), hipMemcpyHostToDevice, c.stream));
	const dim3 grid((unsigned)groups), threads(NTH_THREADS);
	const u32 top = 8 * ((u32)sizeof(KT) - 1), want_idx = out_idx ? 1u : 0u;
	// every level's histogram and pick (those behind the switch to the candidates do nothing), then the candidates' two passes
	hipLaunchKernelGGL((rsx_nth_hist_kernel<KT, 1>), grid, threads, 0, c.stream, src, (u64)n, ka, (const NthCtl *)ctl, table, chunk, top);
	hipLaunchKernelGGL((rsx_nth_pick_kernel<KT>), dim3(1), dim3(256), 0, c.stream, ctl, table, top, (u64)cap, want_idx);
	if constexpr (sizeof(KT) > 1) {
		for (u32 shift = top - 8;; shift -= 8) {
			hipLaunchKernelGGL((rsx_nth_hist_kernel<KT, 0>), grid, threads, 0, c.stream, src, (u64)n, ka, (const NthCtl *)ctl, table, chunk,
			                   shift);
			hipLaunchKernelGGL((rsx_nth_pick_kernel<KT>), dim3(1), dim3(256), 0, c.stream, ctl, table, shift, (u64)cap, want_idx);
			if (!shift)
				break;
		}
	}
	hipLaunchKernelGGL((rsx_nth_count_kernel<KT>), grid, threads, 0, c.stream, src, (u64)n, ka, ctl, goff, chunk);
	hipLaunchKernelGGL((rsx_nth_write_kernel<KT, IT>), grid, threads, 0, c.stream, src, (u64)n, ka, ctl, (const u64 *)goff, chunk, ck, ci,
	                   (u64)cap);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(&h, ctl, offsetof(NthCtl, act_prefix), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	if (h.mode == 0 || (h.mode == 1 && (h.cand_n == 0 || h.cand_n > cap)) || (h.mode == 2 && out_idx))
		return RSX_OK;
	// the candidates sorted by the library's stable sorts (their scratch is the context's other buffers)
	const KT *sk = ck;
	const IT *si = ci;
	if (h.mode == 1 && h.cand_n > 1) {
		rsx_info si_info;
		info_clear(&si_info, dtype);
		if (out_idx) {
			RSX_TRY((sort_pairs_device<KT, IT>(c, ck, ck2, ci, ci2, (size_t)h.cand_n, dtype, order, &si_info)));
			if (si_info.result_in_aux) {
				sk = ck2;
				si = ci2;
			}
		} else {
			void *res = nullptr;
			RSX_TRY(sort_keys_device<KT>(c, ck, ck2, (size_t)h.cand_n, dtype, order, &res, &si_info));
			sk = (const KT *)res;
		}
	}
	hipLaunchKernelGGL((rsx_nth_gather_kernel<KT, IT>), dim3((unsigned)std::min<u64>(1024, ((u64)m + 255) / 256)), dim3(256), 0, c.stream,
	                   (const NthCtl *)ctl, sk, si, (const u32 *)io.map, (u64)m, out_keys, out_idx, io.nless, io.nequal, ka);
	HIP_TRY(hipGetLastError());
	RSX_TRY(nth_results_back(c, ask, io));
	info->route = RSX_NTH_SELECT;
	info->input_reads = h.input_reads;
	info->digit_passes = h.digit_passes;
	info->active_buckets = h.nact;
	info->from_prefix = h.mode == 2 ? 1 : 0;
	info->candidates = h.mode == 1 ? h.cand_n : 0;
	*done = 1;
	return RSX_OK;
}

// the sort route: rsx_sort_rank_device's machinery on a workspace copy, the m entries read through the ranks
template <typename KT, typename IT>
int nth_by_sort(Ctx &c, const KT *src, size_t n, const NthAsk &ask, int dtype, int order, KT *out_keys, IT *out_idx, rsx_nth_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const size_t m = ask.m;
	NthIo io;
	RSX_TRY(c.vals[0].ensure(2 * n * sizeof(IT)));
	RSX_TRY(nth_io(c, m, &io));
	void *res = nullptr;
	rsx_info ri;
	info_clear(&ri, dtype);
	RSX_TRY((sort_rank_device<KT, IT>(c, src, (IT *)c.vals[0].p, n, dtype, order, &res, &ri)));
	HIP_TRY(hipMemcpyAsync(io.ranks, ask.ranks, m * sizeof(u64), hipMemcpyHostToDevice, c.stream));
	hipLaunchKernelGGL((rsx_nth_sorted_kernel<KT, IT>), dim3((unsigned)std::min<u64>(1024, ((u64)m + 255) / 256)), dim3(256), 0, c.stream, src,
	                   (const IT *)res, (u64)n, (const u64 *)io.ranks, (u64)m, out_keys, out_idx, io.nless, io.nequal, ka);
	HIP_TRY(hipGetLastError());
	RSX_TRY(nth_results_back(c, ask, io));
	info->route = RSX_NTH_SORT;
	return RSX_OK;
}

template <typename KT, typename IT>
int sort_nth_device(Ctx &c, const KT *src, size_t n, const NthAsk &ask, int dtype, int order, KT *out_keys, IT *out_idx, rsx_nth_info *info)
{
	const unsigned force = env().nth_force;
	const size_t nd = ask.distinct.size();
	if (nd >= 1 && nd <= NTH_MAX_RANKS && (force == 1 || (force == 0 && n >= NTH_MIN_N))) {
		int done = 0;
		RSX_TRY((nth_select<KT, IT>(c, src, n, ask, dtype, order, out_keys, out_idx, info, &done)));
		if (done)
			return RSX_OK;
	}
	return nth_by_sort<KT, IT>(c, src, n, ask, dtype, order, out_keys, out_idx, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_nth: the elements at given ranks of the sorted order (rsx_nth.hpp) ---- */
static int nth_args(const char *who, const void *src, size_t n, const uint64_t *ranks, size_t m, rsx_dtype dtype, rsx_order order,
                    const void *out_keys, const void *out_idx, size_t idx_bytes)
{
	RSX_TRY(select_args(who, src, n, dtype, order, out_keys, out_idx, idx_bytes));
	if (m && !ranks)
		return fail(RSX_EINVAL, "%s: ranks is NULL", who);
	for (size_t j = 0; j < m; ++j)
		if (ranks[j] >= (uint64_t)n)
			return fail(RSX_EINVAL, "%s: rank exceeds n (ranks[%zu] = %llu, n = %zu)", who, j, (unsigned long long)ranks[j], n);
	return RSX_OK;
}

static void nth_fill_trivial(size_t m, uint64_t *n_less, uint64_t *n_equal)
{
	for (size_t j = 0; j < m; ++j) {
		if (n_less)
			n_less[j] = 0;
		if (n_equal)
			n_equal[j] = 1;
	}
}

int rsx_sort_nth_device(const void *d_src, size_t n, const uint64_t *ranks, size_t m, rsx_dtype dtype, rsx_order order, void *d_out_keys,
                        void *d_out_idx, size_t idx_bytes, uint64_t *n_less, uint64_t *n_equal, void *stream, rsx_nth_info *info)
{
	rsx_nth_info local;
	info = info_or(info, &local);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	RSX_TRY(nth_args("rsx_sort_nth_device", d_src, n, ranks, m, dtype, order, d_out_keys, d_out_idx, idx_bytes));
	if (m == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_nth_device", "the call waits for what the selection found"));
	if (n == 1) {
		// (one key: itself, at index 0, for every rank)
		const dim3 grid((unsigned)std::min<u64>(1024, ((u64)m + 255) / 256));
		RSX_DISPATCH_KT_W(dtype, idx_bytes, IT, hipLaunchKernelGGL((rsx_nth_single_kernel<KT, IT>), grid, dim3(256), 0, c->stream,
		                                                           (const KT *)d_src, (u64)m, (KT *)d_out_keys, (IT *)d_out_idx));
		HIP_TRY(hipGetLastError());
		nth_fill_trivial(m, n_less, n_equal);
		return RSX_OK;
	}
	NthAsk ask;
	ask.ranks = ranks;
	ask.m = m;
	ask.n_less = n_less;
	ask.n_equal = n_equal;
	ask.distinct.assign(ranks, ranks + m);
	std::sort(ask.distinct.begin(), ask.distinct.end());
	ask.distinct.erase(std::unique(ask.distinct.begin(), ask.distinct.end()), ask.distinct.end());
	ask.map.resize(m);
	for (size_t j = 0; j < m; ++j)
		ask.map[j] = (u32)std::min<size_t>(std::lower_bound(ask.distinct.begin(), ask.distinct.end(), ranks[j]) - ask.distinct.begin(),
		                                   0xFFFFFFFFu);
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_nth_device<KT, IT>(*c, (const KT *)d_src, n, ask, dtype, order, (KT *)d_out_keys, (IT *)d_out_idx, info)));
	return RSX_OK;
}

int rsx_sort_nth(const void *src, size_t n, const uint64_t *ranks, size_t m, rsx_dtype dtype, rsx_order order, void *out_keys, void *out_idx,
                 size_t idx_bytes, uint64_t *n_less, uint64_t *n_equal, rsx_nth_info *info)
{
	rsx_nth_info local;
	info = info_or(info, &local);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(nth_args("rsx_sort_nth", src, n, ranks, m, dtype, order, out_keys, out_idx, idx_bytes));
	if (m == 0)
		return RSX_OK;
	if (one_on_host(n, src)) {
		// (one key: itself, at index 0, for every rank)
		for (size_t j = 0; j < m; ++j) {
			if (out_keys)
				memcpy((char *)out_keys + j * kb, src, kb);
			if (out_idx)
				memset((char *)out_idx + j * idx_bytes, 0, idx_bytes);
		}
		nth_fill_trivial(m, n_less, n_equal);
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const StageRow rows[3] = {{src, n * kb, n * kb, STAGE_RECS0}, {out_keys, 0, m * kb}, {out_idx, 0, m * idx_bytes}};
	return staged_call(*c, "rsx_sort_nth", rows, [&](void *const *d, size_t *back) {
		back[1] = m * kb, back[2] = m * idx_bytes;
		return rsx_sort_nth_device(d[0], n, ranks, m, dtype, order, d[1], d[2], idx_bytes, n_less, n_equal, nullptr, info);
	});
}

}  // extern "C"
