// rsx_reduce_api.hpp: rsx_sort_reduce[_device] -- the host driver (routes by cells in LDS, cells in device memory or sort + runs over
// the kernels of rsx_reduce.hpp; the arithmetic: rsx_reduce_shape.hpp) and its entry points; part of librsx.so's host side, included
// by rsx.hip behind the routes, rsx_api.hpp and rsx_keybits_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_reduce_device: count, sum, min and max of a second column per group of equal keys -----------------
// what the call writes: each may be nullptr
struct ReduceOut {
	void *keys, *counts;
	size_t idx_bytes;
	void *sum, *mn, *mx;
};

// below this many elements the plan is made at once: a sample and its wait cost more than the histogram it could save
constexpr size_t REDUCE_SAMPLE_MIN = (size_t)1 << 16;

inline bool reduce_val_dtype_ok(int d) { return d == RSX_U32 || d == RSX_I32 || d == RSX_F32 || d == RSX_U64 || d == RSX_I64 || d == RSX_F64; }
inline bool reduce_val_is_float(int d) { return d == RSX_F32 || d == RSX_F64; }

// one value's sum on the host: the bits of the 64-bit sum of a group of one
inline u64 reduce_one_sum(const void *val, int val_dtype)
{
	u64 out = 0;
	switch (val_dtype) {
	case RSX_U32: { uint32_t v; memcpy(&v, val, 4); out = v; } break;
	case RSX_I32: { int32_t v; memcpy(&v, val, 4); out = (u64)(long long)v; } break;
	case RSX_F32: { float v; memcpy(&v, val, 4); const double d = 0.0 + (double)v; memcpy(&out, &d, 8); } break;
	case RSX_F64: { double v; memcpy(&v, val, 8); const double d = 0.0 + v; memcpy(&out, &d, 8); } break;
	default: memcpy(&out, val, 8); break;
	}
	return out;
}

template <typename VT> ReduceOutPtrs<VT> reduce_out_ptrs(const ReduceOut &out)
{
	return ReduceOutPtrs<VT>{out.counts, (u32)out.idx_bytes, (u64 *)out.sum, (VT *)out.mn, (VT *)out.mx};
}

// routes 1 and 2: the table set to the identities, one sweep over keys and values, the read-out.  *done = 0: no room (not an
// error: the caller takes the sort)
template <typename KT, typename VT, bool FLT>
int reduce_by_cells(Ctx &c, const KT *keys, const VT *vals, size_t n, KdfArgs<KT> ka, KdfArgs<VT> kv, u64 vary, u32 vbits, u32 flags,
                    const ReduceOut &out, rsx_reduce_info *info, int *done)
{
	constexpr u32 VB = sizeof(VT);
	*done = 0;
	BitRuns runs;
	if (!vbits || !bit_runs(vary, &runs))
		return RSX_OK;
	const bool in_lds = vbits <= env().reduce_lds_bits && vbits <= REDUCE_LDS_MAX_BITS;
	ReduceLds lds{};
	if (in_lds) {
		lds = reduce_lds(vbits, flags & REDUCE_OPS, VB, env().reduce_replicas);
		if (!lds.sets)
			return RSX_OK;
	} else if (sizeof(KT) < 2 || vbits > REDUCE_GLOBAL_MAX_BITS) {
		return RSX_OK;
	}
	const u32 grid = reduce_grid(n, reduce_step_elems(sizeof(KT), VB));
	if (!reduce_share_fits(n, grid))
		return RSX_OK;
	const u64 table_bytes = reduce_table_bytes(vbits, VB);
	if (c.rcells.ensure((size_t)table_bytes) != RSX_OK)
		return RSX_OK;
	u64 *table = (u64 *)c.rcells.p;
	const u64 C = (u64)1 << vbits;
	hipLaunchKernelGGL(rsx_reduce_init_kernel, dim3((unsigned)std::min<u64>((table_bytes / 4 + 255) / 256, 1024)), dim3(256), 0, c.stream, (u32 *)table,
	                   table_bytes / 4, 4 * C, 4 * C + C * VB / 4);
	if (in_lds) {
		auto kernel = rsx_reduce_cells_kernel<KT, VB, FLT, true>;
		static std::atomic<int> raised_on{-1};   // (per instantiation: the device whose limit of dynamic LDS was raised last)
		if (raised_on.load() != c.device) {
			if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REDUCE_LDS_BUDGET) != hipSuccess)
				(void)hipGetLastError();   // (a runtime that has no such limit to raise)
			raised_on.store(c.device);
		}
		hipLaunchKernelGGL(kernel, dim3(grid), dim3(REDUCE_THREADS), lds.bytes, c.stream, keys, vals, (u64)n, ka, kv, runs, vbits, flags, lds, table);
	} else {
		if constexpr (sizeof(KT) >= 2)
			hipLaunchKernelGGL((rsx_reduce_cells_kernel<KT, VB, FLT, false>), dim3(grid), dim3(REDUCE_THREADS), 0, c.stream, keys, vals, (u64)n, ka, kv,
			                   runs, vbits, flags, lds, table);
	}
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL((rsx_reduce_readout_kernel<KT, VB>), dim3(1), dim3(1024), 0, c.stream, (const u64 *)table, vbits, keys, ka, kv, runs, (KT)vary,
	                   (KT *)out.keys, reduce_out_ptrs<VT>(out), unique_hdr(c));
	HIP_TRY(hipGetLastError());
	info->route = in_lds ? RSX_REDUCE_CELLS_LDS : RSX_REDUCE_CELLS_GLOBAL;
	info->table_bytes = table_bytes;
	*done = 1;
	return RSX_OK;
}

// route 3: the stable key + value sort of workspace copies (none where the input is `sorted`), the heads, the runs, the seams
template <typename KT, typename VT, bool FLT>
int reduce_by_sort(Ctx &c, const KT *keys, const VT *vals, size_t n, int dtype, int order, bool sorted, KdfArgs<VT> kv, u32 flags,
                   const ReduceOut &out, rsx_reduce_info *info)
{
	constexpr u32 VB = sizeof(VT);
	const KT *in = keys;
	const VT *vin = vals;
	if (!sorted) {
		const size_t npad = (n + 63) & ~(size_t)63;   // (the second buffers as well aligned as the first)
		RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
		RSX_TRY(c.keys[1].ensure(n * sizeof(KT)));
		RSX_TRY(c.vals[0].ensure(2 * npad * sizeof(VT)));
		KT *k0 = (KT *)c.keys[0].p, *k1 = (KT *)c.keys[1].p;
		VT *v0 = (VT *)c.vals[0].p, *v1 = v0 + npad;
		HIP_TRY(hipMemcpyAsync(k0, keys, n * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
		HIP_TRY(hipMemcpyAsync(v0, vals, n * sizeof(VT), hipMemcpyDeviceToDevice, c.stream));
		rsx_info si;
		info_clear(&si, dtype);
		RSX_TRY((sort_pairs_device<KT, VT>(c, k0, k1, v0, v1, n, dtype, order, &si)));
		info->sort = si;
		in = si.result_in_aux ? k1 : k0;
		vin = si.result_in_aux ? v1 : v0;
	}
	u64 tiles;
	RSX_TRY(keybits_heads<KT>(c, in, n, &tiles));
	RSX_TRY(c.rcells.ensure((size_t)tiles * sizeof(ReducePart)));
	ReducePart *parts = (ReducePart *)c.rcells.p;
	hipLaunchKernelGGL((rsx_reduce_runs_kernel<KT, VB, FLT>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, in, vin, (u64)n,
	                   (const UniqueRec *)unique_recs(c), kv, flags, (KT *)out.keys, reduce_out_ptrs<VT>(out), parts);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL((rsx_reduce_seams_kernel<VB, FLT>), dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, c.stream, (const ReducePart *)parts,
	                   (const UniqueRec *)unique_recs(c), tiles, kv, flags, reduce_out_ptrs<VT>(out));
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

template <typename KT, typename VT, bool FLT>
int sort_reduce_typed(Ctx &c, const KT *keys, const VT *vals, size_t n, int dtype, int order, int val_dtype, unsigned ops, const ReduceOut &out,
                      size_t *n_groups, rsx_reduce_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const KdfArgs<VT> kv = make_kdf<VT>(val_dtype, RSX_ASCENDING);
	const u32 flags = ops | (val_dtype == RSX_I32 ? (u32)REDUCE_SIGNED : 0u);
	const u32 max_bits = env().reduce_force == 2 ? 0u : env().reduce_max_bits;
	KeyBits kb;
	// Keys that end on the sort route should not pay for a plan the sort makes again: from REDUCE_SAMPLE_MIN elements on a sample of
	// the keys is looked at first (rsx_unique_sample_kernel: OR and AND of 4096 derived keys, a lower bound of the varying bits), and
	// more proven bits than any table takes send the keys to the sort as RSX_REDUCE_FORCE=2 does -- no plan, varying_bits = 0
	bool rejected = max_bits == 0;
	if (!rejected && n >= REDUCE_SAMPLE_MIN) {
		RSX_TRY(c.urecs.ensure(64 + 64 * sizeof(UniqueRec)));
		const u64 init[2] = {0, ~0ull};
		u64 got[2];
		HIP_TRY(hipMemcpyAsync(unique_hdr(c), init, sizeof init, hipMemcpyHostToDevice, c.stream));
		hipLaunchKernelGGL((rsx_unique_sample_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, keys, (u64)n, ka, unique_hdr(c));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(got, unique_hdr(c), sizeof got, hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
		rejected = (u32)__builtin_popcountll(got[0] ^ got[1]) > max_bits;
	}
	if (!rejected)
		RSX_TRY(keybits_front<KT>(c, keys, n, ka, max_bits, &info->sort, &info->varying_bits, &kb));
	else
		RSX_TRY(c.urecs.ensure(64 + 64 * sizeof(UniqueRec)));
	bool sorted = kb.sorted;
	info->route = RSX_REDUCE_SORT;
	if (kb.planned && kb.vary == 0) {
		// every key equal: the sorted case of the sort route -- one run over all tiles
		info->route = RSX_REDUCE_TRIVIAL;
		sorted = true;
	} else if (kb.planned && max_bits && kb.vbits <= max_bits) {
		int done = 0;
		RSX_TRY((reduce_by_cells<KT, VT, FLT>(c, keys, vals, n, ka, kv, kb.vary, kb.vbits, flags, out, info, &done)));
		if (done)
			return unique_total(c, n_groups);
	}
	RSX_TRY((reduce_by_sort<KT, VT, FLT>(c, keys, vals, n, dtype, order, sorted, kv, flags, out, info)));
	return unique_total(c, n_groups);
}

template <typename KT, typename VT>
int sort_reduce_device(Ctx &c, const KT *keys, const VT *vals, size_t n, int dtype, int order, int val_dtype, unsigned ops, const ReduceOut &out,
                       size_t *n_groups, rsx_reduce_info *info)
{
	if (reduce_val_is_float(val_dtype))
		return sort_reduce_typed<KT, VT, true>(c, keys, vals, n, dtype, order, val_dtype, ops, out, n_groups, info);
	return sort_reduce_typed<KT, VT, false>(c, keys, vals, n, dtype, order, val_dtype, ops, out, n_groups, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_reduce: per-group count, sum, min and max of values (rsx_reduce.hpp) ---- */
static int reduce_args(const char *who, const void *keys, const void *vals, size_t n, rsx_dtype dtype, rsx_order order, rsx_dtype val_dtype,
                       unsigned ops, size_t idx_bytes, const void *out_sum, const void *out_min, const void *out_max, const size_t *n_groups)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || !n_groups || (n && (!keys || !vals)))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!reduce_val_dtype_ok(val_dtype))
		return fail(RSX_EINVAL, "%s: val_dtype %d (values are 4 or 8 bytes wide)", who, (int)val_dtype);
	if (ops & ~(unsigned)REDUCE_OPS)
		return fail(RSX_EINVAL, "%s: ops = %u (bits of RSX_REDUCE_SUM | MIN | MAX)", who, ops);
	if (!(ops & RSX_REDUCE_SUM) != !out_sum || !(ops & RSX_REDUCE_MIN) != !out_min || !(ops & RSX_REDUCE_MAX) != !out_max)
		return fail(RSX_EINVAL, "%s: an output and its bit of ops do not agree", who);
	return idx_args(who, idx_bytes, n, n);   // (a count may be n itself)
}

int rsx_sort_reduce_device(const void *d_keys, const void *d_vals, size_t n, rsx_dtype dtype, rsx_order order, rsx_dtype val_dtype, unsigned ops,
                           void *d_out_keys, void *d_out_counts, size_t idx_bytes, void *d_out_sum, void *d_out_min, void *d_out_max,
                           void *stream, size_t *n_groups, rsx_reduce_info *info)
{
	rsx_reduce_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	RSX_TRY(reduce_args("rsx_sort_reduce_device", d_keys, d_vals, n, dtype, order, val_dtype, ops, idx_bytes, d_out_sum, d_out_min, d_out_max, n_groups));
	if (n == 0) {
		*n_groups = 0;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_reduce_device", "the call waits for the number of groups"));
	const size_t vb = dtype_size(val_dtype);
	if (n == 1) {
		// (one element: its key, once, and its value three times over)
		if (d_out_keys)
			HIP_TRY(hipMemcpyAsync(d_out_keys, d_keys, dtype_size(dtype), hipMemcpyDeviceToDevice, c->stream));
		if (d_out_min)
			HIP_TRY(hipMemcpyAsync(d_out_min, d_vals, vb, hipMemcpyDeviceToDevice, c->stream));
		if (d_out_max)
			HIP_TRY(hipMemcpyAsync(d_out_max, d_vals, vb, hipMemcpyDeviceToDevice, c->stream));
		if (d_out_sum) {
			u64 v = 0;
			HIP_TRY(hipMemcpyAsync(&v, d_vals, vb, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			RSX_TRY(put_index_device(d_out_sum, 8, reduce_one_sum(&v, val_dtype), c->stream));
		}
		if (d_out_counts)
			RSX_TRY(put_index_device(d_out_counts, idx_bytes, 1, c->stream));
		*n_groups = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	const ReduceOut out{d_out_keys, d_out_counts, idx_bytes, d_out_sum, d_out_min, d_out_max};
	RSX_DISPATCH_KT_W(dtype, vb, VT,
	                  return (sort_reduce_device<KT, VT>(*c, (const KT *)d_keys, (const VT *)d_vals, n, dtype, order, val_dtype, ops, out, n_groups, info)));
	return RSX_OK;
}

int rsx_sort_reduce(const void *keys, const void *vals, size_t n, rsx_dtype dtype, rsx_order order, rsx_dtype val_dtype, unsigned ops,
                    void *out_keys, void *out_counts, size_t idx_bytes, void *out_sum, void *out_min, void *out_max, size_t *n_groups,
                    rsx_reduce_info *info)
{
	rsx_reduce_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	RSX_TRY(reduce_args("rsx_sort_reduce", keys, vals, n, dtype, order, val_dtype, ops, idx_bytes, out_sum, out_min, out_max, n_groups));
	const size_t kb = dtype_size(dtype), vb = dtype_size(val_dtype);
	if (n == 0) {
		*n_groups = 0;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	if (one_on_host(n, keys)) {
		if (out_keys)
			memcpy(out_keys, keys, kb);
		if (out_counts)
			put_index(out_counts, idx_bytes, 1);
		if (out_sum)
			put_index(out_sum, 8, reduce_one_sum(vals, val_dtype));
		if (out_min)
			memcpy(out_min, vals, vb);
		if (out_max)
			memcpy(out_max, vals, vb);
		*n_groups = 1;
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	// (a sum is 8 bytes wide whatever the values are)
	const StageRow rows[7] = {{keys, n * kb, n * kb, STAGE_RECS0}, {vals, n * vb, n * vb, STAGE_RECS1}, {out_keys, 0, n * kb},
	                          {out_counts, 0, n * idx_bytes}, {out_sum, 0, n * 8}, {out_min, 0, n * vb}, {out_max, 0, n * vb}};
	return staged_call(*c, "rsx_sort_reduce", rows, [&](void *const *d, size_t *back) {
		RSX_TRY(rsx_sort_reduce_device(d[0], d[1], n, dtype, order, val_dtype, ops, d[2], d[3], idx_bytes, d[4], d[5], d[6], nullptr, n_groups, info));
		back[2] = *n_groups * kb, back[3] = *n_groups * idx_bytes, back[4] = *n_groups * 8, back[5] = back[6] = *n_groups * vb;
		return (int)RSX_OK;
	});
}

}  // extern "C"
