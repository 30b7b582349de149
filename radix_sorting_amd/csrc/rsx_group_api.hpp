// rsx_group_api.hpp: rsx_sort_group[_device] -- the host driver (routes by rank cells over the bitmap, count table or sort + heads
// over the kernels of rsx_group.hpp and rsx_unique.hpp) and its entry points; part of librsx.so's host side, included by rsx.hip
// behind the routes, rsx_api.hpp and rsx_unique_api.hpp.
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
int group_lookup(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, const BitRuns &runs, u32 vbits, u32 ncells, IT *inverse, rsx_group_info *info)
{
	// as the mark kernel: two workgroups of 1024 threads fill a CU (2 x 16 or 2 x 64 KiB of its 160 KiB of LDS), and a
	// workgroup should have a few sweeps of its own to pay for its copy of the cells
	const u64 nvec = (u64)n * sizeof(KT) / 16;
	const unsigned grid = (unsigned)std::max<u64>(1, std::min<u64>(512, nvec / 16384));
	const GroupCell *cells = group_cells(c);
	if (vbits <= 16)
		hipLaunchKernelGGL((rsx_group_lookup_kernel<KT, IT, 16>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, cells, ncells, inverse);
	else if (vbits <= 18)
		hipLaunchKernelGGL((rsx_group_lookup_kernel<KT, IT, 18>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, cells, ncells, inverse);
	else
		hipLaunchKernelGGL((rsx_group_lookup_kernel<KT, IT, 0>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, cells, ncells, inverse);
	HIP_TRY(hipGetLastError());
	info->route = vbits <= 18 ? RSX_GROUP_RANK_LDS : RSX_GROUP_RANK_GLOBAL;
	return RSX_OK;
}

// routes 1 and 2: every key sets its bit, the cells are made over the bitmap, every key looks its group up.  *done = 0: no room.
template <typename KT, typename IT>
int group_rank(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, u64 vary, u32 vbits, const BitRuns &runs, const GroupOut<KT, IT> &out,
               size_t *n_groups, rsx_group_info *info, int *done)
{
	*done = 0;
	if constexpr (sizeof(KT) >= 2) {
		const u64 words = std::max<u64>(UNIQUE_CHUNK_WORDS, ((u64)1 << vbits) / 32);   // (a multiple of the read-out's chunk)
		const u64 chunks = words / UNIQUE_CHUNK_WORDS;
		if (c.ubits.ensure((size_t)words * sizeof(u32)) != RSX_OK || c.gcells.ensure((size_t)words * sizeof(GroupCell)) != RSX_OK ||
		    c.urecs.ensure(64 + (size_t)chunks * sizeof(UniqueRec)) != RSX_OK)
			return RSX_OK;   // (not an error: the caller takes the sort)
		u32 *bitmap = (u32 *)c.ubits.p;
		HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)words * sizeof(u32), c.stream));
		const u64 nvec = (u64)n * sizeof(KT) / 16;
		const u32 full = vbits > 18 && vbits <= 20 ? 256u : 512u;
		const unsigned grid = (unsigned)std::max<u64>(1, std::min<u64>(full, nvec / 16384));
		if (vbits <= 16)
			hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 16>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
		else if (vbits <= 18)
			hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 18>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
		else if (vbits <= 20)
			hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 20>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
		else
			hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 0>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
		hipLaunchKernelGGL((rsx_unique_expand_kernel<KT, 0>), dim3((unsigned)chunks), dim3(256), 0, c.stream, (const u32 *)bitmap,
		                   unique_recs(c), (KT *)nullptr, src, ka, runs, (KT)vary);
		hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(1024), 0, c.stream, unique_recs(c), chunks, unique_hdr(c));
		hipLaunchKernelGGL(rsx_group_cells_kernel, dim3((unsigned)chunks), dim3(256), 0, c.stream, (const u32 *)bitmap,
		                   (const UniqueRec *)unique_recs(c), group_cells(c));
		if (out.keys)
			hipLaunchKernelGGL((rsx_unique_expand_kernel<KT, 1>), dim3((unsigned)chunks), dim3(256), 0, c.stream, (const u32 *)bitmap,
			                   unique_recs(c), out.keys, src, ka, runs, (KT)vary);
		HIP_TRY(hipGetLastError());
		if (out.inverse)
			RSX_TRY((group_lookup<KT, IT>(c, src, n, ka, runs, vbits, (u32)words, out.inverse, info)));
		info->route = vbits <= 18 ? RSX_GROUP_RANK_LDS : RSX_GROUP_RANK_GLOBAL;
		info->table_bytes = (u64)words * (sizeof(u32) + sizeof(GroupCell));
		*done = 1;
		return unique_total(c, n_groups);
	}
	return RSX_OK;
}

// route 4: the stable key + index sort of a workspace copy (none where the plan found the input sorted), then the heads
template <typename KT, typename IT>
int group_by_sort(Ctx &c, const KT *src, size_t n, int dtype, int order, bool sorted, const GroupOut<KT, IT> &out, size_t *n_groups,
                  rsx_group_info *info)
{
	info->route = RSX_GROUP_SORT;
	const KT *in = src;
	const IT *perm = nullptr;
	if (!sorted) {
		const size_t npad = (n + 63) & ~(size_t)63;   // (the second buffers as well aligned as the first)
		RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
		RSX_TRY(c.keys[1].ensure(n * sizeof(KT)));
		RSX_TRY(c.vals[0].ensure(2 * npad * sizeof(IT)));
		KT *k0 = (KT *)c.keys[0].p, *k1 = (KT *)c.keys[1].p;
		IT *v0 = (IT *)c.vals[0].p, *v1 = v0 + npad;
		HIP_TRY(hipMemcpyAsync(k0, src, n * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
		hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, v0, (u64)n);
		HIP_TRY(hipGetLastError());
		rsx_info si;
		info_clear(&si, dtype);
		RSX_TRY((sort_pairs_device<KT, IT>(c, k0, k1, v0, v1, n, dtype, order, &si)));
		info->sort = si;
		in = si.result_in_aux ? k1 : k0;
		perm = si.result_in_aux ? v1 : v0;
	}
	const u64 tiles = ((u64)n + unique_heads_tile<KT>() - 1) / unique_heads_tile<KT>();
	RSX_TRY(c.urecs.ensure(64 + (size_t)tiles * sizeof(UniqueRec)));
	hipLaunchKernelGGL((rsx_unique_heads_kernel<KT, 0>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, in, (u64)n, unique_recs(c),
	                   (KT *)nullptr, (void *)nullptr, 0u);
	hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(1024), 0, c.stream, unique_recs(c), tiles, unique_hdr(c));
	if (out.inverse || out.keys || out.counts || out.first)
		hipLaunchKernelGGL((rsx_group_heads_kernel<KT, IT>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, in, perm, (u64)n,
		                   (const UniqueRec *)unique_recs(c), out.inverse, out.keys, out.counts, out.first);
	HIP_TRY(hipGetLastError());
	return unique_total(c, n_groups);
}

template <typename KT, typename IT>
int sort_group_device(Ctx &c, const KT *src, size_t n, int dtype, int order, const GroupOut<KT, IT> &out, size_t *n_groups, rsx_group_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u32 max_bits = env().group_max_bits;
	RSX_TRY(c.urecs.ensure(64 + 64 * sizeof(UniqueRec)));
	bool to_sort = false, sorted = false;
	if (unique_sample_wanted<KT>(c, n)) {
		// (as rsx_sort_unique_device: the sample can only PROVE that many bits vary -- more than any table here takes)
		const u64 init[2] = {0, ~0ull};
		u64 got[2];
		HIP_TRY(hipMemcpyAsync(unique_hdr(c), init, sizeof init, hipMemcpyHostToDevice, c.stream));
		hipLaunchKernelGGL((rsx_unique_sample_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, src, (u64)n, ka, unique_hdr(c));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(got, unique_hdr(c), sizeof got, hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
		const u32 limit = !max_bits ? 0u : (out.counts || out.first) ? 8u : max_bits;   // (with counts or first: one kept column at most)
		to_sort = (u32)__builtin_popcountll(got[0] ^ got[1]) > limit;
	}
	if (!to_sort) {
		Plan plan{};
		RSX_TRY(plan_phase<KT>(c, src, n, ka, &plan, 0));
		info_from_plan(&info->sort, plan);
		const u64 vary = ((u64)plan.vary_hi << 32) | plan.vary_lo;
		const u32 vbits = (u32)__builtin_popcountll(vary);
		info->varying_bits = vbits;
		sorted = plan.sorted != 0;
		if (sorted)
			info->sort.early_exit = 2;
		if (vary == 0) {
			// every key equal: one group of n, first seen at 0
			info->route = RSX_GROUP_TRIVIAL;
			*n_groups = 1;
			const IT cnt = (IT)n;
			if (out.inverse)
				HIP_TRY(hipMemsetAsync(out.inverse, 0, n * sizeof(IT), c.stream));
			if (out.keys)
				HIP_TRY(hipMemcpyAsync(out.keys, src, sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
			if (out.first)
				HIP_TRY(hipMemsetAsync(out.first, 0, sizeof(IT), c.stream));
			if (out.counts) {
				HIP_TRY(hipMemcpyAsync(out.counts, &cnt, sizeof(IT), hipMemcpyHostToDevice, c.stream));
				HIP_TRY(hipStreamSynchronize(c.stream));   // (cnt goes out of scope)
			}
			return RSX_OK;
		}
		if (max_bits && plan.ncols == 1 && !out.first && c.gcells.ensure(UNIQUE_CHUNK_WORDS * sizeof(GroupCell)) == RSX_OK) {
			// one kept column: the plan's 256 scanned counts say which of its values occur and how often -- no mark pass
			const u32 col = plan.cols[0];
			hipLaunchKernelGGL((rsx_group_table_kernel<KT>), dim3(1), dim3(256), 0, c.stream, (const u64 *)(c.ghist() + 256 * col), (u64)n,
			                   8 * col, src, ka, group_cells(c), out.keys, (void *)out.counts, (u32)sizeof(IT), unique_hdr(c));
			HIP_TRY(hipGetLastError());
			BitRuns runs{};
			runs.n = 1;
			runs.src[0] = (uint8_t)(8 * col);
			runs.len[0] = 8;
			runs.dst[0] = 0;
			if (out.inverse)
				RSX_TRY((group_lookup<KT, IT>(c, src, n, ka, runs, 8u, 8u, out.inverse, info)));
			info->route = RSX_GROUP_TABLE;
			info->table_bytes = 256 * sizeof(u64) + 8 * sizeof(GroupCell);
			return unique_total(c, n_groups);
		}
		BitRuns runs;
		if (!out.counts && !out.first && vbits <= max_bits && bit_runs(vary, &runs)) {
			int done = 0;
			RSX_TRY((group_rank<KT, IT>(c, src, n, ka, vary, vbits, runs, out, n_groups, info, &done)));
			if (done)
				return RSX_OK;
		}
	}
	return group_by_sort<KT, IT>(c, src, n, dtype, order, sorted, out, n_groups, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_group: every key's group among the distinct keys in order (rsx_group.hpp) ---- */
static int group_args(const char *who, const void *src, size_t n, rsx_dtype dtype, rsx_order order, size_t idx_bytes, const size_t *n_groups)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || !n_groups || (n && !src))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (idx_bytes != 4 && idx_bytes != 8)
		return fail(RSX_EINVAL, "%s: idx_bytes = %zu (4 or 8)", who, idx_bytes);
	if (idx_bytes == 4 && (uint64_t)n > 0xFFFFFFFFull)   // (a count may be n itself)
		return fail(RSX_EINVAL, "%s: n = %zu does not fit a 4-byte index", who, n);
	return RSX_OK;
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
		const u64 one64 = 1;
		const u32 one32 = 1;
		if (d_out_inverse)
			HIP_TRY(hipMemsetAsync(d_out_inverse, 0, idx_bytes, c->stream));
		if (d_out_keys)
			HIP_TRY(hipMemcpyAsync(d_out_keys, d_src, dtype_size(dtype), hipMemcpyDeviceToDevice, c->stream));
		if (d_out_first)
			HIP_TRY(hipMemsetAsync(d_out_first, 0, idx_bytes, c->stream));
		if (d_out_counts) {
			HIP_TRY(hipMemcpyAsync(d_out_counts, idx_bytes == 4 ? (const void *)&one32 : (const void *)&one64, idx_bytes, hipMemcpyHostToDevice,
			                       c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
		}
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
		if (out_counts) {
			if (idx_bytes == 4)
				*(uint32_t *)out_counts = 1;
			else
				*(uint64_t *)out_counts = 1;
		}
		*n_groups = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	void *const outs[4] = {out_inverse, out_counts, out_first, out_keys};
	if (is_device_ptr(src)) {
		for (void *o : outs)
			if (o && !is_device_ptr(o))
				return fail(RSX_EINVAL, "rsx_sort_group: src is a device pointer but an output is not");
		RSX_TRY(rsx_sort_group_device(src, n, dtype, order, out_inverse, out_keys, out_counts, out_first, idx_bytes, nullptr, n_groups, info));
		HIP_TRY(hipStreamSynchronize(c->stream));
		return RSX_OK;
	}
	// host buffers: the keys staged in recs[0] as rsx_sort_rank stages them, the outputs in [inverse][counts][first][keys]
	const size_t ipad = (n * idx_bytes + 255) & ~(size_t)255;
	RSX_TRY(c->recs[0].ensure(n * kb));
	RSX_TRY(c->gout.ensure(3 * ipad + n * kb));
	HIP_TRY(hipMemcpyAsync(c->recs[0].p, src, n * kb, hipMemcpyHostToDevice, c->stream));
	char *dout[4];
	for (int i = 0; i < 4; ++i)
		dout[i] = outs[i] ? (char *)c->gout.p + (size_t)i * ipad : nullptr;
	RSX_TRY(rsx_sort_group_device(c->recs[0].p, n, dtype, order, dout[0], dout[3], dout[1], dout[2], idx_bytes, nullptr, n_groups, info));
	const size_t g = *n_groups;
	if (out_inverse)
		HIP_TRY(hipMemcpyAsync(out_inverse, dout[0], n * idx_bytes, hipMemcpyDeviceToHost, c->stream));
	if (out_counts)
		HIP_TRY(hipMemcpyAsync(out_counts, dout[1], g * idx_bytes, hipMemcpyDeviceToHost, c->stream));
	if (out_first)
		HIP_TRY(hipMemcpyAsync(out_first, dout[2], g * idx_bytes, hipMemcpyDeviceToHost, c->stream));
	if (out_keys)
		HIP_TRY(hipMemcpyAsync(out_keys, dout[3], g * kb, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return RSX_OK;
}

}  // extern "C"
