// rsx_unique_api.hpp: rsx_sort_unique[_device] -- the host driver (routes by bitmap, count table or sort + compaction over the kernels
// of rsx_unique.hpp) and its entry points; part of librsx.so's host side, included by rsx.hip behind the routes and rsx_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_unique_device: the distinct keys in order, by bitmap or count table where they fit (rsx_unique.hpp) ------
// The sizes at which the ordinary sort would go without a histogram (blind_wanted's, without spending its back-off): there
// a sample of the keys is looked at first, so that evenly spread keys never pay a histogram the sort would not have paid.
template <typename KT> bool unique_sample_wanted(const Ctx &c, size_t n)
{
	if constexpr (sizeof(KT) < 4)
		return false;
	if (!blind_gate(c))
		return false;
	if (n < ((size_t)1 << 22) || n >= blind_keys_end<KT>())
		return false;
	size_t floor_keys = sizeof(KT) == 8 ? (size_t)9 << 19 : (size_t)15 << 19;
	if (env().blind_min_log2)
		floor_keys = (size_t)1 << env().blind_min_log2;
	floor_keys = std::min(floor_keys, (size_t)1 << env().two_level_min_log2);
	return n >= floor_keys;
}

inline u64 *unique_hdr(Ctx &c) { return (u64 *)c.urecs.p; }
inline UniqueRec *unique_recs(Ctx &c) { return (UniqueRec *)((u64 *)c.urecs.p + 8); }

// the number of distinct keys a read-out left in the header, once the stream is through
inline int unique_total(Ctx &c, size_t *n_unique)
{
	u64 total = 0;
	HIP_TRY(hipMemcpyAsync(&total, unique_hdr(c), sizeof total, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	*n_unique = (size_t)total;
	return RSX_OK;
}

// the sorted array `in` compacted into `out`: count the heads per tile, scan, write (12 bytes per 4-byte key)
template <typename KT>
int unique_compact(Ctx &c, const KT *in, KT *out, size_t n, void *counts, size_t count_bytes, size_t *n_unique)
{
	const u64 tiles = ((u64)n + unique_heads_tile<KT>() - 1) / unique_heads_tile<KT>();
	RSX_TRY(c.urecs.ensure(64 + (size_t)tiles * sizeof(UniqueRec)));
	hipLaunchKernelGGL((rsx_unique_heads_kernel<KT, 0>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, in, (u64)n, unique_recs(c),
	                   (KT *)nullptr, (void *)nullptr, 0u);
	hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(1024), 0, c.stream, unique_recs(c), tiles, unique_hdr(c));
	hipLaunchKernelGGL((rsx_unique_heads_kernel<KT, 1>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, in, (u64)n, unique_recs(c), out,
	                   counts, (u32)count_bytes);
	HIP_TRY(hipGetLastError());
	return unique_total(c, n_unique);
}

// routes 1 and 2: every key sets its bit, the bitmap is read out in order.  *done = 0: no room for the bitmap.
template <typename KT>
int unique_bitmap(Ctx &c, const KT *src, KT *out, size_t n, KdfArgs<KT> ka, u64 vary, u32 vbits, const BitRuns &runs, size_t *n_unique,
                  rsx_unique_info *info, int *done)
{
	*done = 0;
	if constexpr (sizeof(KT) >= 2) {
		const u64 words = std::max<u64>(UNIQUE_CHUNK_WORDS, ((u64)1 << vbits) / 32);   // (a multiple of the read-out's chunk)
		const u64 chunks = words / UNIQUE_CHUNK_WORDS;
		if (c.ubits.ensure((size_t)words * sizeof(u32)) != RSX_OK || c.urecs.ensure(64 + (size_t)chunks * sizeof(UniqueRec)) != RSX_OK)
			return RSX_OK;   // (not an error: the caller takes the sort)
		u32 *bitmap = (u32 *)c.ubits.p;
		HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)words * sizeof(u32), c.stream));
		// Two workgroups of 1024 threads fill a CU (2048 threads; 2 x 8 or 2 x 32 KiB of its 160 KiB of LDS); the 128 KiB form
		// leaves room for one.  A workgroup should have at least four sweeps of its own to pay for zeroing and merging its bitmap.
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
		hipLaunchKernelGGL((rsx_unique_expand_kernel<KT, 1>), dim3((unsigned)chunks), dim3(256), 0, c.stream, (const u32 *)bitmap,
		                   unique_recs(c), out, src, ka, runs, (KT)vary);
		HIP_TRY(hipGetLastError());
		info->route = vbits <= 20 ? RSX_UNIQUE_BITMAP_LDS : RSX_UNIQUE_BITMAP_GLOBAL;
		info->table_bytes = (u64)words * sizeof(u32);
		*done = 1;
		return unique_total(c, n_unique);
	}
	return RSX_OK;
}

template <typename KT>
int sort_unique_device(Ctx &c, KT *src, KT *aux, size_t n, int dtype, int order, void *counts, size_t count_bytes, void **result,
                       size_t *n_unique, rsx_unique_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const u32 max_bits = env().unique_max_bits;
	RSX_TRY(c.urecs.ensure(64 + 64 * sizeof(UniqueRec)));
	bool have_plan = false, to_sort = false;
	Plan plan{};
	if (unique_sample_wanted<KT>(c, n)) {
		// The sample can only PROVE that many bits vary (a bit that differs between two sampled keys differs among the keys):
		// more than any bitmap or table here takes, and the keys go to the sort as if this entry point were rsx_sort_device.
		const u64 init[2] = {0, ~0ull};
		u64 got[2];
		HIP_TRY(hipMemcpyAsync(unique_hdr(c), init, sizeof init, hipMemcpyHostToDevice, c.stream));
		hipLaunchKernelGGL((rsx_unique_sample_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, (const KT *)src, (u64)n, ka, unique_hdr(c));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(got, unique_hdr(c), sizeof got, hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
		const u32 limit = !max_bits ? 0u : counts ? 8u : max_bits;   // (with counts: one kept column at most)
		to_sort = (u32)__builtin_popcountll(got[0] ^ got[1]) > limit;
	}
	u64 vary = 0;
	u32 vbits = 0;
	if (!to_sort) {
		RSX_TRY(plan_phase<KT>(c, src, n, ka, &plan, 0));
		have_plan = true;
		info_from_plan(&info->sort, plan);
		vary = ((u64)plan.vary_hi << 32) | plan.vary_lo;
		vbits = (u32)__builtin_popcountll(vary);
		info->varying_bits = vbits;
		if (plan.sorted)
			info->sort.early_exit = 2;
		if (vary == 0) {
			// every key equal: the first one, n times
			info->route = RSX_UNIQUE_TRIVIAL;
			*result = src;
			*n_unique = 1;
			if (counts) {
				const u64 c64 = n;
				const u32 c32 = (u32)n;
				HIP_TRY(hipMemcpyAsync(counts, count_bytes == 4 ? (const void *)&c32 : (const void *)&c64, count_bytes, hipMemcpyHostToDevice,
				                       c.stream));
				HIP_TRY(hipStreamSynchronize(c.stream));
			}
			return RSX_OK;
		}
		if (max_bits && plan.ncols == 1) {
			// one kept column: its 256 counts are the answer (the scanned histogram the plan left), no key is read again
			const u32 col = plan.cols[0];
			hipLaunchKernelGGL((rsx_unique_table_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, (const u64 *)(c.ghist() + 256 * col),
			                   (const u32 *)nullptr, 256u, (u64)n, 8 * col, (const KT *)src, ka, aux, counts, (u32)count_bytes, unique_hdr(c));
			HIP_TRY(hipGetLastError());
			info->route = RSX_UNIQUE_TABLE;
			info->table_bytes = 256 * sizeof(u64);
			*result = aux;
			info->sort.result_in_aux = 1;
			return unique_total(c, n_unique);
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
				info->route = RSX_UNIQUE_TABLE;
				info->table_bytes = 65536 * sizeof(u32);
				*result = aux;
				info->sort.result_in_aux = 1;
				return unique_total(c, n_unique);
			}
		}
		BitRuns runs;
		if (!counts && vbits <= max_bits && bit_runs(vary, &runs)) {
			int done = 0;
			RSX_TRY(unique_bitmap<KT>(c, src, aux, n, ka, vary, vbits, runs, n_unique, info, &done));
			if (done) {
				*result = aux;
				info->sort.result_in_aux = 1;
				return RSX_OK;
			}
		}
	}
	// the ordinary sort (any route; every early exit), then one compaction of the sorted buffer into the other one
	info->route = RSX_UNIQUE_SORT;
	KT *in = src;
	if (!(have_plan && plan.sorted)) {
		void *res = nullptr;
		rsx_info si;
		info_clear(&si, dtype);
		RSX_TRY(sort_keys_device<KT>(c, src, aux, n, dtype, order, &res, &si));
		info->sort = si;
		in = (KT *)res;
	}
	KT *out = in == src ? aux : src;
	RSX_TRY(unique_compact<KT>(c, in, out, n, counts, count_bytes, n_unique));
	*result = out;
	info->sort.result_in_aux = out == aux;
	return RSX_OK;
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
		const u64 one64 = 1;
		const u32 one32 = 1;
		HIP_TRY(hipMemcpyAsync(d_counts, count_bytes == 4 ? (const void *)&one32 : (const void *)&one64, count_bytes, hipMemcpyHostToDevice,
		                       (hipStream_t)stream));
		HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
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
		if (count_bytes == 4)
			*(uint32_t *)counts = 1;
		else
			*(uint64_t *)counts = 1;
		*result = src;
		*n_unique = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	if (is_device_ptr(src)) {
		if (!is_device_ptr(aux) || (counts && !is_device_ptr(counts)))
			return fail(RSX_EINVAL, "rsx_sort_unique: src is a device pointer but aux or counts is not");
		return rsx_sort_unique_device(src, aux, n, dtype, order, counts, count_bytes, nullptr, result, n_unique, info);
	}
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
