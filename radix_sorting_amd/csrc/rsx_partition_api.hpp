// rsx_partition_api.hpp: rsx_sort_partition[_device] -- the host driver (count, scan and stable placement by a searched part over the
// kernels of rsx_partition.hpp, or rsx_sort_locate_device's bins, their rank sort and a gather) and its entry points; part of
// librsx.so's host side, included by rsx.hip behind rsx_locate_api.hpp.
#pragma once

namespace {

static_assert((unsigned)PARTITION_MAX_EDGES == (unsigned)RSX_PARTITION_MAX_EDGES, "rsx.h and rsx_partition_shape.hpp disagree");
static_assert((unsigned)PARTITION_MAX_EDGES == (unsigned)PARTITION_MAX_EDGES_COMPILED && PARTITION_MAX_EDGES_DEFAULT <= PARTITION_MAX_EDGES_COMPILED, "rsx_env.hpp and rsx_partition_shape.hpp disagree");
static_assert((unsigned)PARTITION_BALLOT_PARTS_DEFAULT == (unsigned)PARTITION_BALLOT_PARTS_ENV_DEFAULT, "rsx_env.hpp and rsx_partition_shape.hpp disagree");

// ---- rsx_sort_partition_device: the stable multi-way split by given splitters (rsx_partition.hpp) -----------------
// what the call writes: keys or idx may be nullptr (not both), offsets may be
template <typename KT, typename IT> struct PartitionOut {
	KT *keys;      // n entries
	IT *idx;       // n entries
	IT *offsets;   // m + 2 entries
	bool below;    // RSX_PARTITION_BELOW
};

// where the parts of the scatter route's table lie in parttab
struct PartitionTab {
	LocateHdr *hdr;
	u32 *start;
	void *edges;
	u64 *cum, *rows, *starts;
};
inline size_t partition_tab_bytes(u32 wgs) { return 2048 + 2048 + 2048 + 2 * (size_t)wgs * PARTITION_MAX_BINS * sizeof(u64); }
inline PartitionTab partition_tab(void *p, u32 wgs)
{
	PartitionTab t;
	char *b = (char *)p;
	t.hdr = (LocateHdr *)b;
	t.start = (u32 *)(b + 256);
	t.edges = b + 2048;                 // at most 255 keys of 8 bytes
	t.cum = (u64 *)(b + 4096);          // at most 256 entries
	t.rows = (u64 *)(b + 6144);
	t.starts = t.rows + (size_t)wgs * PARTITION_MAX_BINS;
	return t;
}

// route 1.  `sv`: the edges in sorted order.  *done = 0: more than the cut-off distinct edges, or no room.
template <typename KT, typename IT>
int partition_scatter(Ctx &c, const KT *src, size_t n, const KT *sv, size_t m, int dtype, int order, const PartitionOut<KT, IT> &out,
                      rsx_partition_info *info, int *done)
{
	*done = 0;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u32 max_d = env().partition_max_edges;
	const PartitionGrid g = partition_grid((u64)n, partition_head((u64)(uintptr_t)src, (u32)sizeof(KT), (u64)n));
	if (c.parttab.ensure(partition_tab_bytes(g.wgs)) != RSX_OK)
		return RSX_OK;
	const PartitionTab t = partition_tab(c.parttab.p, g.wgs);
	LocateHdr h;
	RSX_TRY(locate_prepared<KT>(c, sv, m, ka, max_d, t.edges, t.cum, t.start, t.hdr, &h));
	info->distinct_edges = h.distinct;
	if (h.distinct == 0 || h.distinct > max_d)
		return RSX_OK;
	const u32 form = partition_rank_form(h.distinct + 1u, env().partition_ballot_parts);
	// (the count writes no index: one instantiation serves both index widths)
#define RSX_PARTITION_LAUNCH(WT, PLACE, FORM, ROWS, KEYS, IDX)                                                                            \
	hipLaunchKernelGGL((rsx_partition_pass_kernel<KT, WT, PLACE, FORM>), dim3(g.wgs), dim3(PARTITION_THREADS), 0, c.stream, src, (u64)n, ka,   \
	                   (const KT *)t.edges, (const u32 *)t.start, h.distinct, h.shift, h.steps, out.below ? 1u : 0u, g, ROWS, KEYS, IDX)
	if (form == 1)
		RSX_PARTITION_LAUNCH(u32, false, 1, t.rows, (KT *)nullptr, (u32 *)nullptr);
	else
		RSX_PARTITION_LAUNCH(u32, false, 2, t.rows, (KT *)nullptr, (u32 *)nullptr);
	hipLaunchKernelGGL((rsx_partition_scan_kernel<IT>), dim3(1), dim3(1024), 0, c.stream, (const u64 *)t.rows, t.starts, g.wgs, h.distinct,
	                   (const u64 *)t.cum, (u64)m, (u64)n, out.offsets);
	if (form == 1)
		RSX_PARTITION_LAUNCH(IT, true, 1, t.starts, out.keys, out.idx);
	else
		RSX_PARTITION_LAUNCH(IT, true, 2, t.starts, out.keys, out.idx);
#undef RSX_PARTITION_LAUNCH
	HIP_TRY(hipGetLastError());
	info->route = RSX_PARTITION_SCATTER;
	info->input_reads = 2;
	info->search_steps = h.steps;
	info->rank_form = form;
	info->shares = g.wgs;
	*done = 1;
	return RSX_OK;
}

inline size_t idx_slot_bytes(size_t n, size_t idx_bytes) { return (n * idx_bytes + 255) & ~(size_t)255; }

// route 2: partidx = [bins n][indices n][indices n][less m][equal m]; rsx_sort_locate_device's bins of the keys and less / equal of
// the sorted edges, the stable rank sort of the bins (their constant bytes cost no pass), keys and indices through it
template <typename KT, typename IT>
int partition_by_sort(Ctx &c, const KT *src, size_t n, const KT *sv, size_t m, int dtype, int order, const PartitionOut<KT, IT> &out,
                      rsx_partition_info *info)
{
	info->route = RSX_PARTITION_SORT;
	info->input_reads = info->search_steps = info->rank_form = info->shares = 0;
	const size_t npad = idx_slot_bytes(n, sizeof(IT)), mpad = idx_slot_bytes(m, sizeof(IT));
	RSX_TRY(c.partidx.ensure(npad + 2 * npad + 2 * mpad));
	char *b = (char *)c.partidx.p;
	IT *bins = (IT *)b, *ib = (IT *)(b + npad), *less = (IT *)(b + 3 * npad), *equal = (IT *)(b + 3 * npad + mpad);
	const LocateOut<IT> lo{out.offsets ? less : nullptr, (out.offsets && out.below) ? equal : nullptr, bins, out.below};
	RSX_TRY((sort_locate_device<KT, IT>(c, src, n, sv, m, dtype, order, lo, &info->locate)));
	if (!info->distinct_edges)
		info->distinct_edges = info->locate.distinct_values;
	void *res = nullptr;
	RSX_TRY((sort_rank_device<IT, IT>(c, bins, ib, n, unsigned_dtype(sizeof(IT)), RSX_ASCENDING, &res, &info->sort)));
	hipLaunchKernelGGL((rsx_partition_gather_kernel<KT, IT>), dim3(small_grid(n, 256, 2048)), dim3(256), 0, c.stream, src, (const IT *)res, (u64)n,
	                   out.keys, out.idx);
	if (out.offsets) {
		HIP_TRY(hipMemcpyAsync(out.offsets + 1, less, m * sizeof(IT), hipMemcpyDeviceToDevice, c.stream));
		hipLaunchKernelGGL((rsx_partition_ends_kernel<IT>), dim3(small_grid(m + 2, 256, 2048)), dim3(256), 0, c.stream, out.offsets,
		                   out.below ? (const IT *)equal : (const IT *)nullptr, (u64)m, (u64)n);
	}
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// n > 0 and m > 0
template <typename KT, typename IT>
int sort_partition_device(Ctx &c, const KT *src, size_t n, const KT *edges, size_t m, int dtype, int order, const PartitionOut<KT, IT> &out,
                          rsx_partition_info *info)
{
	const KT *sv = nullptr;
	RSX_TRY(sorted_copy<KT>(c, c.partvals, edges, m, dtype, order, &sv));   // (sort_locate_device fills locvals while it reads them)
	if (env().partition_force != 2) {
		int done = 0;
		RSX_TRY((partition_scatter<KT, IT>(c, src, n, sv, m, dtype, order, out, info, &done)));
		if (done)
			return RSX_OK;
	}
	return partition_by_sort<KT, IT>(c, src, n, sv, m, dtype, order, out, info);
}

// m == 0: one part
template <typename IT>
int partition_one_part(Ctx &c, const void *src, size_t n, size_t kb, void *out_keys, IT *out_idx, IT *offsets)
{
	if (out_keys)
		HIP_TRY(hipMemcpyAsync(out_keys, src, n * kb, hipMemcpyDeviceToDevice, c.stream));
	if (out_idx)
		hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(small_grid(n, 256, 2048)), dim3(256), 0, c.stream, out_idx, (u64)n);
	if (offsets)
		hipLaunchKernelGGL((rsx_partition_ends_kernel<IT>), dim3(1), dim3(256), 0, c.stream, offsets, (const IT *)nullptr, (u64)0, (u64)n);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

}  // namespace

extern "C" {

/* ---- rsx_sort_partition: the stable multi-way split by given splitters (rsx_partition.hpp) ---- */
static int partition_args(const char *who, const void *src, size_t n, const void *edges, size_t m, rsx_dtype dtype, rsx_order order,
                          const void *out_keys, const void *out_idx, size_t idx_bytes, uint32_t flags)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || (n && !src) || (m && !edges) ||
	    (flags & ~(uint32_t)RSX_PARTITION_BELOW))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!out_keys && !out_idx)
		return fail(RSX_EINVAL, "%s: both of out_keys and out_idx are NULL", who);
	if (n && out_keys == src)
		return fail(RSX_EINVAL, "%s: out_keys is src (the split is not done in place)", who);
	RSX_TRY(idx_args(who, idx_bytes, n, n));   // (an offset may be n itself)
	if (idx_bytes == 4 && (uint64_t)m > 0xFFFFFFFEull)
		return fail(RSX_EINVAL, "%s: m = %zu does not fit a 4-byte index", who, m);
	return RSX_OK;
}

static void partition_info_start(rsx_partition_info *info, rsx_dtype dtype)
{
	info_clear(&info->sort, dtype);
	info_clear(&info->locate.sort, dtype);
	info->key_bytes = info->locate.key_bytes = (uint32_t)dtype_size(dtype);
}

int rsx_sort_partition_device(const void *d_src, size_t n, const void *d_edges, size_t m, rsx_dtype dtype, rsx_order order, void *d_out_keys,
                              void *d_out_idx, void *d_offsets, size_t idx_bytes, uint32_t flags, void *stream, rsx_partition_info *info)
{
	rsx_partition_info local;
	info = info_or(info, &local);
	partition_info_start(info, dtype);
	RSX_TRY(partition_args("rsx_sort_partition_device", d_src, n, d_edges, m, dtype, order, d_out_keys, d_out_idx, idx_bytes, flags));
	if (n == 0 && !d_offsets)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_partition_device", "the call waits for the number of distinct edges"));
	if (n == 0) {
		HIP_TRY(hipMemsetAsync(d_offsets, 0, (m + 2) * idx_bytes, c->stream));
		return RSX_OK;
	}
	if (m == 0) {
		if (idx_bytes == 4)
			return partition_one_part<u32>(*c, d_src, n, dtype_size(dtype), d_out_keys, (u32 *)d_out_idx, (u32 *)d_offsets);
		return partition_one_part<u64>(*c, d_src, n, dtype_size(dtype), d_out_keys, (u64 *)d_out_idx, (u64 *)d_offsets);
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_partition_device<KT, IT>(*c, (const KT *)d_src, n, (const KT *)d_edges, m, dtype, order,
	                                                        PartitionOut<KT, IT>{(KT *)d_out_keys, (IT *)d_out_idx, (IT *)d_offsets,
	                                                                             (flags & RSX_PARTITION_BELOW) != 0},
	                                                        info)));
	return RSX_OK;
}

int rsx_sort_partition(const void *src, size_t n, const void *edges, size_t m, rsx_dtype dtype, rsx_order order, void *out_keys, void *out_idx,
                       void *offsets, size_t idx_bytes, uint32_t flags, rsx_partition_info *info)
{
	rsx_partition_info local;
	info = info_or(info, &local);
	partition_info_start(info, dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(partition_args("rsx_sort_partition", src, n, edges, m, dtype, order, out_keys, out_idx, idx_bytes, flags));
	if (n == 0 && !offsets)
		return RSX_OK;
	if (n == 0 && (rsx_device_count() <= 0 || !is_device_ptr(offsets))) {   // (asked first: then no device call is made)
		memset(offsets, 0, (m + 2) * idx_bytes);
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const size_t ob = (m + 2) * idx_bytes;
	const StageRow rows[5] = {{src, n * kb, n * kb, STAGE_RECS0}, {edges, m * kb, m * kb}, {out_keys, 0, n * kb}, {out_idx, 0, n * idx_bytes},
	                          {offsets, 0, ob}};
	return staged_call(*c, "rsx_sort_partition", rows, [&](void *const *d, size_t *back) {
		back[2] = n * kb, back[3] = n * idx_bytes, back[4] = ob;
		return rsx_sort_partition_device(d[0], n, d[1], m, dtype, order, d[2], d[3], d[4], idx_bytes, flags, nullptr, info);
	});
}

}  // extern "C"
