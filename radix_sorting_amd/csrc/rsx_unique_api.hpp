// rsx_unique_api.hpp: rsx_sort_unique[_device] -- the host driver (routes by bitmap, count table or sort + compaction over the kernels
// of rsx_unique.hpp) and its entry points; part of librsx.so's host side, included by rsx.hip behind the routes, rsx_api.hpp and
// rsx_keybits_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_unique_device: the distinct keys in order, by bitmap or count table where they fit (rsx_unique.hpp) ------
template <typename KT>
int sort_unique_device(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void *counts, size_t count_bytes, void **result,
                       size_t *n_unique, rsx_unique_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u32 max_bits = env().unique_max_bits;
	KeyBits kb;
	// (with counts: one kept column at most)
	RSX_TRY(keybits_front<KT>(c, src, n, ka, !max_bits ? 0u : counts ? 8u : max_bits, &info->sort, &info->varying_bits, &kb));
	const Plan &plan = kb.plan;
	// a bitmap or table was read out into aux: how many keys that were
	auto read_out = [&](uint32_t route, u64 table_bytes) {
		info->route = route;
		info->table_bytes = table_bytes;
		*result = aux;
		info->sort.result_in_aux = 1;
		return unique_total(c, n_unique);
	};
	if (kb.planned) {
		if (kb.vary == 0) {
			// every key equal: the first one, n times
			info->route = RSX_UNIQUE_TRIVIAL;
			*result = src;
			*n_unique = 1;
			if (counts)
				RSX_TRY(put_index_device(counts, count_bytes, n, c.stream));
			return RSX_OK;
		}
		if (max_bits && plan.ncols == 1) {
			// one kept column: its 256 counts are the answer (the scanned histogram the plan left), no key is read again
			const u32 col = plan.cols[0];
			hipLaunchKernelGGL((rsx_unique_table_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, (const u64 *)(c.ghist() + 256 * col),
			                   (const u32 *)nullptr, 256u, (u64)n, 8 * col, (const KT *)src, ka, aux, counts, (u32)count_bytes, unique_hdr(c));
			HIP_TRY(hipGetLastError());
			return read_out(RSX_UNIQUE_TABLE, 256 * sizeof(u64));
		}
		if constexpr (sizeof(KT) == 2) {
			// 2-byte keys with counts: the joint table of both bytes (32-bit counters: below 2^32 keys; the kernel leaves sorted
			// input alone, which the compaction below takes without a sort)
			if (max_bits && counts && plan.ncols == 2 && !plan.sorted && n < ((size_t)1 << 32) &&
			    c.joint.ensure(65536 * sizeof(u32) + 65537 * sizeof(u64) + 8) == RSX_OK) {
				u32 *jt = (u32 *)c.joint.p;
				HIP_TRY(hipMemsetAsync(jt, 0, 65536 * sizeof(u32), c.stream));
				hipLaunchKernelGGL(rsx_joint16_kernel, dim3(512), dim3(1024), 0, c.stream, (const uint16_t *)src, (u64)n, ka, jt,
				                   (const Plan *)c.plan());
				hipLaunchKernelGGL((rsx_unique_table_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, (const u64 *)nullptr, (const u32 *)jt,
				                   65536u, (u64)n, 0u, (const KT *)src, ka, aux, counts, (u32)count_bytes, unique_hdr(c));
				HIP_TRY(hipGetLastError());
				return read_out(RSX_UNIQUE_TABLE, 65536 * sizeof(u32));
			}
		}
		if constexpr (sizeof(KT) >= 2) {
			// routes 1 and 2: every key sets its bit, the bitmap is read out in order (no room for it: the sort)
			BitRuns runs;
			if (!counts && kb.vbits <= max_bits && bit_runs(kb.vary, &runs)) {
				const BitmapShape s = bitmap_shape(kb.vbits);
				int done = 0;
				RSX_TRY(keybits_bitmap<KT>(c, src, n, ka, kb.vary, runs, s, &done));
				if (done) {
					hipLaunchKernelGGL((rsx_unique_expand_kernel<KT, 1>), dim3((unsigned)s.chunks), dim3(256), 0, c.stream, (const u32 *)c.ubits.p,
					                   unique_recs(c), aux, (const KT *)src, ka, runs, (KT)kb.vary);
					HIP_TRY(hipGetLastError());
					return read_out(kb.vbits <= 20 ? RSX_UNIQUE_BITMAP_LDS : RSX_UNIQUE_BITMAP_GLOBAL, s.bytes);
				}
			}
		}
	}
	// the ordinary sort (any route; every early exit), then one compaction of the sorted buffer into the other one
	info->route = RSX_UNIQUE_SORT;
	KT *in = src;
	if (!kb.sorted) {
		void *res = nullptr;
		rsx_info si;
		info_clear(&si, dtype);
		RSX_TRY(sort_keys_device<KT>(c, src, aux, n, dtype, order, &res, &si));
		info->sort = si;
		in = (KT *)res;
	}
	// the sorted array `in` compacted into `out`: count the heads per tile, scan, write (12 bytes per 4-byte key)
	KT *out = in == src ? aux : src;
	u64 tiles;
	RSX_TRY(keybits_heads<KT>(c, (const KT *)in, n, &tiles));
	hipLaunchKernelGGL((rsx_unique_heads_kernel<KT, 1>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, (const KT *)in, (u64)n,
	                   unique_recs(c), out, counts, (u32)count_bytes);
	HIP_TRY(hipGetLastError());
	*result = out;
	info->sort.result_in_aux = out == aux;
	return unique_total(c, n_unique);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_unique: the distinct keys in order (rsx_unique.hpp) ---- */
static int unique_args(const char *who, size_t n, rsx_dtype dtype, rsx_order order, const void *src, const void *aux, const void *counts,
                       size_t count_bytes, void **result, size_t *n_unique)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || !result || !n_unique || (n && (!src || !aux)))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (counts ? (count_bytes != 4 && count_bytes != 8) : (count_bytes != 0 && count_bytes != 4 && count_bytes != 8))
		return fail(RSX_EINVAL, "%s: count_bytes = %zu (4 or 8)", who, count_bytes);
	if (counts && count_bytes == 4 && (uint64_t)n > 0xFFFFFFFFull)
		return fail(RSX_EINVAL, "%s: n = %zu does not fit a 4-byte count", who, n);
	return RSX_OK;
}

int rsx_sort_unique_device(void *d_src, void *d_aux, size_t n, rsx_dtype dtype, rsx_order order, void *d_counts, size_t count_bytes,
                           void *stream, void **result, size_t *n_unique, rsx_unique_info *info)
{
	rsx_unique_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	RSX_TRY(unique_args("rsx_sort_unique_device", n, dtype, order, d_src, d_aux, d_counts, count_bytes, result, n_unique));
	if (n < 2 && !(n == 1 && d_counts)) {
		*result = d_src;
		*n_unique = n;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_unique_device", "the call waits for the number of distinct keys"));
	if (n == 1) {
		// (one key, once: the only small case that has to write device memory)
		RSX_TRY(put_index_device(d_counts, count_bytes, 1, (hipStream_t)stream));
		*result = d_src;
		*n_unique = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_DISPATCH_KT(dtype, return sort_unique_device<KT>(*c, (KT *)d_src, (KT *)d_aux, n, dtype, order, d_counts, count_bytes, result,
	                                                     n_unique, info));
	return RSX_OK;
}

int rsx_sort_unique(void *src, void *aux, size_t n, rsx_dtype dtype, rsx_order order, void *counts, size_t count_bytes, void **result,
                    size_t *n_unique, rsx_unique_info *info)
{
	rsx_unique_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(unique_args("rsx_sort_unique", n, dtype, order, src, aux, counts, count_bytes, result, n_unique));
	if (n < 2 && !(n == 1 && counts)) {
		*result = src;
		*n_unique = n;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	if (one_on_host(n, src)) {
		put_index(counts, count_bytes, 1);
		*result = src;
		*n_unique = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const void *const ps[3] = {src, aux, counts};
	const PtrKind kind = pointer_kind(ps, 3);
	if (kind == PTR_MIXED)
		return mixed_pointers("rsx_sort_unique");
	if (kind == PTR_DEVICE)
		return rsx_sort_unique_device(src, aux, n, dtype, order, counts, count_bytes, nullptr, result, n_unique, info);
	// host buffers: staged as rsx_sort stages them; the distinct keys (and counts) come back into the buffer that
	// corresponds to the device buffer they ended in, the other one is left as it was
	RSX_TRY(c->keys[0].ensure(n * kb));
	RSX_TRY(c->keys[1].ensure(n * kb));
	if (counts)
		RSX_TRY(c->vals[0].ensure(n * count_bytes));
	HIP_TRY(hipMemcpyAsync(c->keys[0].p, src, n * kb, hipMemcpyHostToDevice, c->stream));
	void *dres = nullptr;
	RSX_TRY(rsx_sort_unique_device(c->keys[0].p, c->keys[1].p, n, dtype, order, counts ? c->vals[0].p : nullptr, count_bytes, nullptr, &dres,
	                               n_unique, info));
	void *hres = dres == c->keys[1].p ? aux : src;
	if (dres == c->keys[1].p || info->route != RSX_UNIQUE_TRIVIAL)
		HIP_TRY(hipMemcpyAsync(hres, dres, *n_unique * kb, hipMemcpyDeviceToHost, c->stream));
	if (counts)
		HIP_TRY(hipMemcpyAsync(counts, c->vals[0].p, *n_unique * count_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	*result = hres;
	return RSX_OK;
}

}  // extern "C"
