// rsx_group_api.hpp: rsx_sort_group[_device] -- the host driver (routes by rank cells over the bitmap, count table or sort + heads
// over the kernels of rsx_group.hpp and rsx_unique.hpp) and its entry points; part of librsx.so's host side, included by rsx.hip
// behind the routes, rsx_api.hpp and rsx_keybits_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_group_device: every key's group among the distinct keys in order (rsx_group.hpp) ------------------
// what the call writes: each may be nullptr
template <typename KT, typename IT> struct GroupOut {
	IT *inverse;
	KT *keys;
	IT *counts;
	IT *first;
};

inline GroupCell *group_cells(Ctx &c) { return (GroupCell *)c.gcells.p; }

// the lookup over `ncells` cells made for packed values below 2^vbits
template <typename KT, typename IT>
int group_lookup(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, const BitRuns &runs, u32 vbits, u32 ncells, IT *inverse)
{
	// as the mark kernel: two workgroups of 1024 threads fill a CU (2 x 16 or 2 x 64 KiB of its 160 KiB of LDS), and a
	// workgroup should have a few sweeps of its own to pay for its copy of the cells
	const unsigned grid = sweep_grid(n, sizeof(KT));
	const GroupCell *cells = group_cells(c);
	if (vbits <= 16)
		hipLaunchKernelGGL((rsx_group_lookup_kernel<KT, IT, 16>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, cells, ncells, inverse);
	else if (vbits <= 18)
		hipLaunchKernelGGL((rsx_group_lookup_kernel<KT, IT, 18>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, cells, ncells, inverse);
	else
		hipLaunchKernelGGL((rsx_group_lookup_kernel<KT, IT, 0>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, cells, ncells, inverse);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// route 4: the stable key + index sort of a workspace copy (none where the plan found the input sorted), then the heads
template <typename KT, typename IT>
int group_by_sort(Ctx &c, const KT *src, size_t n, int dtype, int order, bool sorted, const GroupOut<KT, IT> &out, size_t *n_groups,
                  rsx_group_info *info)
{
	info->route = RSX_GROUP_SORT;
	IndexSorted<KT, IT> s;
	RSX_TRY((keybits_index_sort<KT, IT>(c, src, n, dtype, order, sorted, &info->sort, &s)));
	u64 tiles;
	RSX_TRY(keybits_heads<KT>(c, s.in, n, &tiles));
	if (out.inverse || out.keys || out.counts || out.first)
		hipLaunchKernelGGL((rsx_group_heads_kernel<KT, IT>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, s.in, s.perm, (u64)n,
		                   (const UniqueRec *)unique_recs(c), out.inverse, out.keys, out.counts, out.first);
	HIP_TRY(hipGetLastError());
	return unique_total(c, n_groups);
}

template <typename KT, typename IT>
int sort_group_device(Ctx &c, const KT *src, size_t n, int dtype, int order, const GroupOut<KT, IT> &out, size_t *n_groups, rsx_group_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u32 max_bits = env().group_max_bits;
	KeyBits kb;
	// (with counts or first: one kept column at most)
	RSX_TRY(keybits_front<KT>(c, src, n, ka, !max_bits ? 0u : (out.counts || out.first) ? 8u : max_bits, &info->sort, &info->varying_bits, &kb));
	if (kb.planned) {
		const Plan &plan = kb.plan;
		if (kb.vary == 0) {
			// every key equal: one group of n, first seen at 0
			info->route = RSX_GROUP_TRIVIAL;
			*n_groups = 1;
			if (out.inverse)
				HIP_TRY(hipMemsetAsync(out.inverse, 0, n * sizeof(IT), c.stream));
			if (out.keys)
				HIP_TRY(hipMemcpyAsync(out.keys, src, sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
			if (out.first)
				HIP_TRY(hipMemsetAsync(out.first, 0, sizeof(IT), c.stream));
			if (out.counts)
				RSX_TRY(put_index_device(out.counts, sizeof(IT), n, c.stream));
			return RSX_OK;
		}
		if (max_bits && plan.ncols == 1 && !out.first && c.gcells.ensure(UNIQUE_CHUNK_WORDS * sizeof(GroupCell)) == RSX_OK) {
			// one kept column: the plan's 256 scanned counts say which of its values occur and how often -- no mark pass
			const u32 col = plan.cols[0];
			hipLaunchKernelGGL((rsx_group_table_kernel<KT>), dim3(1), dim3(256), 0, c.stream, (const u64 *)(c.ghist() + 256 * col), (u64)n,
			                   8 * col, src, ka, group_cells(c), out.keys, (void *)out.counts, (u32)sizeof(IT), unique_hdr(c));
			HIP_TRY(hipGetLastError());
			if (out.inverse)
				RSX_TRY((group_lookup<KT, IT>(c, src, n, ka, column_runs(col), 8u, 8u, out.inverse)));
			info->route = RSX_GROUP_TABLE;
			info->table_bytes = 256 * sizeof(u64) + 8 * sizeof(GroupCell);
			return unique_total(c, n_groups);
		}
		if constexpr (sizeof(KT) >= 2) {
			// routes 1 and 2: every key sets its bit, the cells are made over the bitmap, every key looks its group up (no room for
			// the cells or the bitmap: the sort)
			BitRuns runs;
			if (!out.counts && !out.first && kb.vbits <= max_bits && bit_runs(kb.vary, &runs)) {
				const BitmapShape s = bitmap_shape(kb.vbits);
				int done = 0;
				if (c.gcells.ensure((size_t)s.words * sizeof(GroupCell)) == RSX_OK)
					RSX_TRY(keybits_bitmap<KT>(c, src, n, ka, kb.vary, runs, s, &done));
				if (done) {
					const u32 *bitmap = (const u32 *)c.ubits.p;
					hipLaunchKernelGGL(rsx_group_cells_kernel, dim3((unsigned)s.chunks), dim3(256), 0, c.stream, bitmap,
					                   (const UniqueRec *)unique_recs(c), group_cells(c));
					if (out.keys)
						hipLaunchKernelGGL((rsx_unique_expand_kernel<KT, 1>), dim3((unsigned)s.chunks), dim3(256), 0, c.stream, bitmap,
						                   unique_recs(c), out.keys, src, ka, runs, (KT)kb.vary);
					HIP_TRY(hipGetLastError());
					if (out.inverse)
						RSX_TRY((group_lookup<KT, IT>(c, src, n, ka, runs, kb.vbits, (u32)s.words, out.inverse)));
					info->route = kb.vbits <= 18 ? RSX_GROUP_RANK_LDS : RSX_GROUP_RANK_GLOBAL;
					info->table_bytes = s.bytes + (u64)s.words * sizeof(GroupCell);
					return unique_total(c, n_groups);
				}
			}
		}
	}
	return group_by_sort<KT, IT>(c, src, n, dtype, order, kb.sorted, out, n_groups, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_group: every key's group among the distinct keys in order (rsx_group.hpp) ---- */
static int group_args(const char *who, const void *src, size_t n, rsx_dtype dtype, rsx_order order, size_t idx_bytes, const size_t *n_groups)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || !n_groups || (n && !src))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	return idx_args(who, idx_bytes, n, n);   // (a count may be n itself)
}

int rsx_sort_group_device(const void *d_src, size_t n, rsx_dtype dtype, rsx_order order, void *d_out_inverse, void *d_out_keys,
                          void *d_out_counts, void *d_out_first, size_t idx_bytes, void *stream, size_t *n_groups, rsx_group_info *info)
{
	rsx_group_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	RSX_TRY(group_args("rsx_sort_group_device", d_src, n, dtype, order, idx_bytes, n_groups));
	if (n == 0) {
		*n_groups = 0;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_group_device", "the call waits for the number of groups"));
	if (n == 1) {
		// (one key: group 0, itself, once, first at 0)
		if (d_out_inverse)
			HIP_TRY(hipMemsetAsync(d_out_inverse, 0, idx_bytes, c->stream));
		if (d_out_keys)
			HIP_TRY(hipMemcpyAsync(d_out_keys, d_src, dtype_size(dtype), hipMemcpyDeviceToDevice, c->stream));
		if (d_out_first)
			HIP_TRY(hipMemsetAsync(d_out_first, 0, idx_bytes, c->stream));
		if (d_out_counts)
			RSX_TRY(put_index_device(d_out_counts, idx_bytes, 1, c->stream));
		*n_groups = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_group_device<KT, IT>(*c, (const KT *)d_src, n, dtype, order,
	                                                    GroupOut<KT, IT>{(IT *)d_out_inverse, (KT *)d_out_keys, (IT *)d_out_counts, (IT *)d_out_first},
	                                                    n_groups, info)));
	return RSX_OK;
}

int rsx_sort_group(const void *src, size_t n, rsx_dtype dtype, rsx_order order, void *out_inverse, void *out_keys, void *out_counts,
                   void *out_first, size_t idx_bytes, size_t *n_groups, rsx_group_info *info)
{
	rsx_group_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(group_args("rsx_sort_group", src, n, dtype, order, idx_bytes, n_groups));
	if (n == 0) {
		*n_groups = 0;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	if (one_on_host(n, src)) {
		if (out_inverse)
			memset(out_inverse, 0, idx_bytes);
		if (out_keys)
			memcpy(out_keys, src, kb);
		if (out_first)
			memset(out_first, 0, idx_bytes);
		if (out_counts)
			put_index(out_counts, idx_bytes, 1);
		*n_groups = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const StageRow rows[5] = {{src, n * kb, n * kb, STAGE_RECS0}, {out_inverse, 0, n * idx_bytes}, {out_keys, 0, n * kb},
	                          {out_counts, 0, n * idx_bytes}, {out_first, 0, n * idx_bytes}};
	return staged_call(*c, "rsx_sort_group", rows, [&](void *const *d, size_t *back) {
		RSX_TRY(rsx_sort_group_device(d[0], n, dtype, order, d[1], d[2], d[3], d[4], idx_bytes, nullptr, n_groups, info));
		back[1] = n * idx_bytes, back[2] = *n_groups * kb, back[3] = back[4] = *n_groups * idx_bytes;
		return (int)RSX_OK;
	});
}

}  // extern "C"
