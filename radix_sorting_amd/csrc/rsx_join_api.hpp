// rsx_join_api.hpp: rsx_sort_join[_device] and rsx_join_pairs[_device] -- the host driver of the equi-join of two key columns
// (phase 1: one range into the sorted right side per left row, by direct addressing into the count table of the right keys' varying
// bits or by sorting the right side and searching it; phase 2: the ranges expanded into the lists of pairs) over the kernels of
// rsx_join.hpp, rsx_rankdata.hpp and rsx_locate.hpp, and its entry points; part of librsx.so's host side, included by rsx.hip
// behind rsx_reduce_api.hpp.
#pragma once

namespace {

static_assert((unsigned)JOIN_TRIVIAL == (unsigned)RSX_JOIN_TRIVIAL && (unsigned)JOIN_TABLE == (unsigned)RSX_JOIN_TABLE &&
                  (unsigned)JOIN_SEARCH == (unsigned)RSX_JOIN_SEARCH && (unsigned)JOIN_MERGE == (unsigned)RSX_JOIN_MERGE &&
                  (unsigned)JOIN_LEFT == (unsigned)RSX_JOIN_LEFT && (unsigned)JOIN_ROW_TILE == (unsigned)RSX_JOIN_ROW_TILE &&
                  (unsigned)JOIN_EXPAND_TILE == (unsigned)RSX_JOIN_EXPAND_TILE,
              "rsx.h and rsx_join_shape.hpp disagree");

// ---- rsx_sort_join_device: one range into the sorted right side per left row (rsx_join.hpp) ------------------------
// what the call writes: each may be nullptr
template <typename IT> struct JoinOut {
	IT *start;        // n entries
	IT *count;        // n entries
	IT *right_perm;   // m entries
	bool left;        // RSX_JOIN_LEFT
};

// jointiles = the pairs of every tile of rows, scanned (what the expansion reads); *n_pairs = their total, once the stream is through
template <typename IT> int join_scan_rows(Ctx &c, const IT *count, size_t n, bool left, u64 *n_pairs)
{
	const u64 T = join_tiles(n, JOIN_ROW_TILE);
	RSX_TRY(c.jointiles.ensure((size_t)(T + 1) * sizeof(u64)));
	u64 *excl = (u64 *)c.jointiles.p;
	hipLaunchKernelGGL((rsx_join_rowsums_kernel<IT>), dim3(small_grid(T, 1, 65536)), dim3(JOIN_THREADS), 0, c.stream, count, (u64)n, left ? 1u : 0u, excl);
	hipLaunchKernelGGL(rsx_join_scan_kernel, dim3(1), dim3(1024), 0, c.stream, excl, T);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(n_pairs, excl + T, sizeof(u64), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	return RSX_OK;
}

// what is known of the right keys before a route is taken
struct JoinRight {
	KeyBits kb;
	bool sorted = false;   // in order as they are: nothing is copied or sorted
};

// the right side in order: the keys (*sk) and, where right_perm is wanted, the stable permutation, written there.  Nothing is
// copied or sorted where the plan found the keys in order.
template <typename KT, typename IT>
int join_sort_right(Ctx &c, const KT *right, size_t m, int dtype, int order, const JoinRight &r, IT *right_perm, rsx_join_info *info, const KT **sk)
{
	*sk = right;
	if (right_perm) {
		IndexSorted<KT, IT> s{right, nullptr, nullptr};
		if (m >= 2)
			RSX_TRY((keybits_index_sort<KT, IT>(c, right, m, dtype, order, r.sorted, &info->sort, &s)));
		if (s.perm)
			HIP_TRY(hipMemcpyAsync(right_perm, s.perm, m * sizeof(IT), hipMemcpyDeviceToDevice, c.stream));
		else
			hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(small_grid(m, 256, 1024)), dim3(256), 0, c.stream, right_perm, (u64)m);
		HIP_TRY(hipGetLastError());
		if (!s.perm)
			info->sort.early_exit = m < 2 ? 1 : 2;
		*sk = s.in;
		return RSX_OK;
	}
	if (r.sorted || m < 2) {
		info->sort.early_exit = m < 2 ? 1 : 2;
		return RSX_OK;
	}
	return keybits_keys_sort<KT>(c, right, m, dtype, order, &info->sort, sk);
}

// route 1: the counts of the right keys' packed varying bits (one-byte keys: of the byte), scanned, and one read of the left keys
// against them.  Where right_perm is wanted the right side is sorted with an iota all the same.  *done = 0: no room for the table
// (not an error: the caller takes the general route).
template <typename KT, typename IT>
int join_table(Ctx &c, const KT *left, size_t n, const KT *right, size_t m, int dtype, int order, const JoinRight &r, const JoinOut<IT> &out,
               rsx_join_info *info, u64 *n_pairs, int *done)
{
	*done = 0;
	constexpr bool ONE = sizeof(KT) == 1;
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const unsigned grid = sweep_grid(n, sizeof(KT));
	const size_t parts_off = ((size_t)join_table_bytes((u32)sizeof(KT)) + 255) & ~(size_t)255;
	if (c.jointab.ensure(parts_off + (size_t)grid * 2 * sizeof(u64)) != RSX_OK)
		return RSX_OK;
	char *base = (char *)c.jointab.p;
	u64 *parts = (u64 *)(base + parts_off);
	if constexpr (ONE) {
		// (all eight bits count as varying: every key passes the test of the fixed bits)
		constexpr size_t CNT_BYTES = 256 * sizeof(u64) + 256;
		u64 *offs = (u64 *)(base + CNT_BYTES);
		HIP_TRY(hipMemsetAsync(base, 0, CNT_BYTES, c.stream));
		RSX_TRY(launch_hist<KT>(c, right, m, ka, (u64 *)base, (u32 *)(base + 256 * sizeof(u64))));
		hipLaunchKernelGGL(rsx_locate_scan256_kernel, dim3(1), dim3(256), 0, c.stream, (const u64 *)base, offs, (u64)m);
		hipLaunchKernelGGL((rsx_join_probe_kernel<KT, IT, true>), dim3(grid), dim3(1024), 0, c.stream, left, (u64)n, ka, column_runs(0), (KT)0xFF, right,
		                   (const u64 *)offs, out.start, out.count, parts);
	} else {
		BitRuns runs;
		if (!bit_runs(r.kb.vary, &runs))
			return RSX_OK;
		u32 *jt = (u32 *)base;
		u64 *offs = (u64 *)(base + 65536 * sizeof(u32));
		HIP_TRY(hipMemsetAsync(jt, 0, 65536 * sizeof(u32), c.stream));
		hipLaunchKernelGGL((rsx_rankdata_count16_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, right, (u64)m, ka, runs, jt);
		hipLaunchKernelGGL(rsx_rankdata_scan16_kernel, dim3(1), dim3(1024), 0, c.stream, (const u32 *)jt, offs, (u64)m);
		hipLaunchKernelGGL((rsx_join_probe_kernel<KT, IT, false>), dim3(grid), dim3(1024), 0, c.stream, left, (u64)n, ka, runs, (KT)r.kb.vary, right,
		                   (const u64 *)offs, out.start, out.count, parts);
	}
	HIP_TRY(hipGetLastError());
	std::vector<u64> host((size_t)grid * 2);
	HIP_TRY(hipMemcpyAsync(host.data(), parts, host.size() * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	u64 pairs = 0;
	for (unsigned b = 0; b < grid; ++b)
		pairs += host[2 * b] + (out.left ? host[2 * b + 1] : 0);
	*n_pairs = pairs;
	if (out.right_perm) {
		const KT *sk;
		RSX_TRY((join_sort_right<KT, IT>(c, right, m, dtype, order, r, out.right_perm, info, &sk)));
	}
	info->route = RSX_JOIN_TABLE;
	info->table_bytes = join_table_read_bytes((u32)sizeof(KT));
	*done = 1;
	return RSX_OK;
}

// routes 2 and 3: the right side sorted, and two binary searches per left key over it -- of the left keys as they come, or
// (merge) of the left keys sorted with an iota, so that neighbouring lanes search neighbouring places, and start / count
// scattered back through the left permutation
template <typename KT, typename IT>
int join_by_search(Ctx &c, const KT *left, size_t n, const KT *right, size_t m, int dtype, int order, const JoinRight &r, bool merge,
                   const JoinOut<IT> &out, rsx_join_info *info, u64 *n_pairs)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const size_t npad = (n + 63) & ~(size_t)63;
	const KT *sl = left;
	const IT *pl = nullptr;
	if (merge && n >= 2) {
		// (the left side first: the right side's sort then leaves its result in the buffers of the context)
		RSX_TRY(c.joinkeys.ensure(2 * npad * sizeof(KT)));
		RSX_TRY(c.joinidx.ensure(4 * npad * sizeof(IT)));
		KT *k0 = (KT *)c.joinkeys.p, *k1 = k0 + npad;
		IT *v0 = (IT *)c.joinidx.p, *v1 = v0 + npad;
		HIP_TRY(hipMemcpyAsync(k0, left, n * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
		hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, v0, (u64)n);
		HIP_TRY(hipGetLastError());
		rsx_info si;
		info_clear(&si, dtype);
		RSX_TRY((sort_pairs_device<KT, IT>(c, k0, k1, v0, v1, n, dtype, order, &si)));
		sl = si.result_in_aux ? k1 : k0;
		pl = si.result_in_aux ? v1 : v0;
		info->left_sorted = 1;
	} else if (!out.count) {
		RSX_TRY(c.joinidx.ensure(npad * sizeof(IT)));
	}
	const KT *sk;
	RSX_TRY((join_sort_right<KT, IT>(c, right, m, dtype, order, r, out.right_perm, info, &sk)));
	IT *const ts = pl ? (IT *)c.joinidx.p + 2 * npad : out.start;
	IT *const tc = pl ? (IT *)c.joinidx.p + 3 * npad : out.count ? out.count : (IT *)c.joinidx.p;
	hipLaunchKernelGGL((rsx_locate_sorted_values_kernel<KT, IT>), dim3(join_search_grid(n)), dim3(256), 0, c.stream, sk, (u64)m, sl, (u64)n, ka,
	                   pl && !out.start ? (IT *)nullptr : ts, tc);
	if (pl && (out.start || out.count))
		hipLaunchKernelGGL((rsx_join_scatter_kernel<IT>), dim3(join_search_grid(n)), dim3(256), 0, c.stream, pl, (u64)n, (const IT *)ts, (const IT *)tc,
		                   out.start, out.count);
	HIP_TRY(hipGetLastError());
	info->route = merge ? RSX_JOIN_MERGE : RSX_JOIN_SEARCH;
	return join_scan_rows<IT>(c, tc, n, out.left, n_pairs);
}

template <typename KT, typename IT>
int sort_join_device(Ctx &c, const KT *left, size_t n, const KT *right, size_t m, int dtype, int order, const JoinOut<IT> &out,
                     rsx_join_info *info, u64 *n_pairs)
{
	const u32 force = env().join_force;
	const bool tables = !env().join_no_table && force == 0;
	JoinRight r;
	if (sizeof(KT) == 1 && tables) {
		int done = 0;
		RSX_TRY((join_table<KT, IT>(c, left, n, right, m, dtype, order, r, out, info, n_pairs, &done)));
		if (done)
			return RSX_OK;
	}
	if (m < 2) {
		// (one right key: nothing varies, and it is in order)
		r.kb.planned = true;
		r.sorted = true;
	} else {
		RSX_TRY(keybits_front<KT>(c, right, m, make_kdf<KT>(dtype, order), tables ? (u32)JOIN_TABLE_MAX_BITS : 0u, &info->sort, &info->varying_bits, &r.kb));
		r.sorted = r.kb.sorted;
	}
	if (sizeof(KT) >= 2 && tables && r.kb.planned && join_table_ok(r.kb.vary, (u64)m)) {
		int done = 0;
		RSX_TRY((join_table<KT, IT>(c, left, n, right, m, dtype, order, r, out, info, n_pairs, &done)));
		if (done)
			return RSX_OK;
	}
	const bool merge = join_route(false, force, (u64)n, (u64)m, (u32)sizeof(KT)) == JOIN_MERGE;
	return join_by_search<KT, IT>(c, left, n, right, m, dtype, order, r, merge, out, info, n_pairs);
}

// ---- rsx_join_pairs_device: the ranges expanded into the lists of pairs ------------------------------------------------------------
template <typename IT>
int join_pairs_device(Ctx &c, const IT *start, const IT *count, const IT *perm, size_t n, size_t m, bool left, IT *out_left, IT *out_right,
                      u64 capacity, u64 *n_pairs)
{
	RSX_TRY(join_scan_rows<IT>(c, count, n, left, n_pairs));
	if (*n_pairs > capacity)
		return fail(RSX_EINVAL, "rsx_join_pairs_device: %llu pairs: the result does not fit a capacity of %llu", (unsigned long long)*n_pairs,
		            (unsigned long long)capacity);
	if (*n_pairs == 0)
		return RSX_OK;
	const u32 grid = join_expand_grid(join_tiles(*n_pairs, JOIN_EXPAND_TILE));
	hipLaunchKernelGGL((rsx_join_expand_kernel<IT>), dim3(grid), dim3(JOIN_THREADS), 0, c.stream, start, count, perm, (u64)n, (u64)m, left ? 1u : 0u,
	                   (const u64 *)c.jointiles.p, *n_pairs, out_left, out_right);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c.stream));
	return RSX_OK;
}

}  // namespace

extern "C" {

/* ---- rsx_sort_join: matching rows of two key columns, phase 1 (rsx_join.hpp) ---- */
static int join_args(const char *who, const void *left, size_t n, const void *right, size_t m, rsx_dtype dtype, rsx_order order, size_t idx_bytes,
                     uint32_t flags, const uint64_t *n_pairs)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || (n && !left) || (m && !right) || (flags & ~(uint32_t)RSX_JOIN_LEFT) ||
	    !n_pairs)
		return fail(RSX_EINVAL, "%s: bad argument", who);
	RSX_TRY(idx_args(who, idx_bytes, n, n));
	return idx_args(who, idx_bytes, m, m);   // (start and count may be m itself)
}

int rsx_sort_join_device(const void *d_left, size_t n, const void *d_right, size_t m, rsx_dtype dtype, rsx_order order, void *d_start,
                         void *d_count, void *d_right_perm, size_t idx_bytes, uint32_t flags, void *stream, uint64_t *n_pairs,
                         rsx_join_info *info)
{
	rsx_join_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	RSX_TRY(join_args("rsx_sort_join_device", d_left, n, d_right, m, dtype, order, idx_bytes, flags, n_pairs));
	const bool left = (flags & RSX_JOIN_LEFT) != 0;
	if (n == 0 || m == 0) {
		// (no row matches anything: count is zeros, and the order of no right rows, or of right rows nobody asks for, is an iota)
		info->route = RSX_JOIN_TRIVIAL;
		*n_pairs = left ? (uint64_t)n : 0;
		if (!(n && (d_start || d_count)) && !(m && d_right_perm))
			return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_join_device", "the call waits for the number of pairs"));
	if (n == 0 || m == 0) {
		if (n && d_start)
			HIP_TRY(hipMemsetAsync(d_start, 0, n * idx_bytes, c->stream));
		if (n && d_count)
			HIP_TRY(hipMemsetAsync(d_count, 0, n * idx_bytes, c->stream));
		if (m && d_right_perm) {
			if (idx_bytes == 4)
				hipLaunchKernelGGL((rsx_iota_kernel<u32>), dim3(small_grid(m, 256, 1024)), dim3(256), 0, c->stream, (u32 *)d_right_perm, (u64)m);
			else
				hipLaunchKernelGGL((rsx_iota_kernel<u64>), dim3(small_grid(m, 256, 1024)), dim3(256), 0, c->stream, (u64 *)d_right_perm, (u64)m);
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(hipStreamSynchronize(c->stream));
		return RSX_OK;
	}
	u64 pairs = 0;
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  RSX_TRY((sort_join_device<KT, IT>(*c, (const KT *)d_left, n, (const KT *)d_right, m, dtype, order,
	                                                    JoinOut<IT>{(IT *)d_start, (IT *)d_count, (IT *)d_right_perm, left}, info, &pairs))));
	HIP_TRY(hipStreamSynchronize(c->stream));
	*n_pairs = pairs;
	return RSX_OK;
}

int rsx_sort_join(const void *left, size_t n, const void *right, size_t m, rsx_dtype dtype, rsx_order order, void *start, void *count,
                  void *right_perm, size_t idx_bytes, uint32_t flags, uint64_t *n_pairs, rsx_join_info *info)
{
	rsx_join_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(join_args("rsx_sort_join", left, n, right, m, dtype, order, idx_bytes, flags, n_pairs));
	const void *const ps[5] = {n ? left : nullptr, m ? right : nullptr, n ? start : nullptr, n ? count : nullptr, m ? right_perm : nullptr};
	if ((n == 0 || m == 0) && (rsx_device_count() <= 0 || pointer_kind(ps, 5) == PTR_HOST)) {
		// nothing matches: answered on the host where the buffers are the host's
		info->route = RSX_JOIN_TRIVIAL;
		*n_pairs = (flags & RSX_JOIN_LEFT) ? (uint64_t)n : 0;
		if (n && start)
			memset(start, 0, n * idx_bytes);
		if (n && count)
			memset(count, 0, n * idx_bytes);
		if (right_perm)
			for (size_t j = 0; j < m; ++j)
				put_index((char *)right_perm + j * idx_bytes, idx_bytes, j);
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const size_t nb = n * idx_bytes, mb = m * idx_bytes;
	const StageRow rows[5] = {{left, n * kb, n * kb, STAGE_RECS0}, {right, m * kb, m * kb, STAGE_RECS1}, {start, 0, nb}, {count, 0, nb},
	                          {right_perm, 0, mb}};
	return staged_call(*c, "rsx_sort_join", rows, [&](void *const *d, size_t *back) {
		back[2] = back[3] = nb, back[4] = mb;
		return rsx_sort_join_device(d[0], n, d[1], m, dtype, order, d[2], d[3], d[4], idx_bytes, flags, nullptr, n_pairs, info);
	});
}

/* ---- rsx_join_pairs: matching rows of two key columns, phase 2 (rsx_join.hpp) ---- */
static int join_pairs_args(const char *who, const void *start, const void *count, const void *right_perm, size_t n, size_t m, size_t idx_bytes,
                           uint32_t flags, const void *out_left, const void *out_right, const uint64_t *n_pairs)
{
	if ((flags & ~(uint32_t)RSX_JOIN_LEFT) || !n_pairs || (n && !count) || (n && out_right && !start) || (n && m && out_right && !right_perm))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!out_left && !out_right)
		return fail(RSX_EINVAL, "%s: both outputs are NULL", who);
	RSX_TRY(idx_args(who, idx_bytes, n, n));
	return idx_args(who, idx_bytes, m, m);
}

int rsx_join_pairs_device(const void *d_start, const void *d_count, const void *d_right_perm, size_t n, size_t m, size_t idx_bytes,
                          uint32_t flags, void *d_out_left, void *d_out_right, uint64_t capacity, void *stream, uint64_t *n_pairs)
{
	if (n_pairs)
		*n_pairs = 0;
	RSX_TRY(join_pairs_args("rsx_join_pairs_device", d_start, d_count, d_right_perm, n, m, idx_bytes, flags, d_out_left, d_out_right, n_pairs));
	if (n == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_join_pairs_device", "the call waits for the number of pairs"));
	const bool left = (flags & RSX_JOIN_LEFT) != 0;
	u64 pairs = 0;
	int rc;
	if (idx_bytes == 4)
		rc = join_pairs_device<u32>(*c, (const u32 *)d_start, (const u32 *)d_count, (const u32 *)d_right_perm, n, m, left, (u32 *)d_out_left,
		                            (u32 *)d_out_right, capacity, &pairs);
	else
		rc = join_pairs_device<u64>(*c, (const u64 *)d_start, (const u64 *)d_count, (const u64 *)d_right_perm, n, m, left, (u64 *)d_out_left,
		                            (u64 *)d_out_right, capacity, &pairs);
	*n_pairs = pairs;
	return rc;
}

int rsx_join_pairs(const void *start, const void *count, const void *right_perm, size_t n, size_t m, size_t idx_bytes, uint32_t flags,
                   void *out_left, void *out_right, uint64_t capacity, uint64_t *n_pairs)
{
	if (n_pairs)
		*n_pairs = 0;
	RSX_TRY(join_pairs_args("rsx_join_pairs", start, count, right_perm, n, m, idx_bytes, flags, out_left, out_right, n_pairs));
	if (n == 0)
		return RSX_OK;
	const void *const ps[5] = {start, count, m ? right_perm : nullptr, out_left, out_right};
	const PtrKind kind = rsx_device_count() <= 0 ? PTR_HOST : pointer_kind(ps, 5);
	if (kind == PTR_MIXED)
		return mixed_pointers("rsx_join_pairs");
	u64 pairs = capacity;   // (device buffers: what the caller set aside)
	if (kind == PTR_HOST) {
		// the number of pairs is a sum over the caller's own counts
		const bool left = (flags & RSX_JOIN_LEFT) != 0;
		pairs = 0;
		for (size_t i = 0; i < n; ++i)
			pairs += join_row_pairs(idx_bytes == 4 ? (u64)((const uint32_t *)count)[i] : (u64)((const uint64_t *)count)[i], left);
		*n_pairs = pairs;
		if (pairs > capacity)
			return fail(RSX_EINVAL, "rsx_join_pairs: %llu pairs: the result does not fit a capacity of %llu", (unsigned long long)pairs,
			            (unsigned long long)capacity);
		if (pairs == 0)
			return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const size_t nb = n * idx_bytes, mb = m * idx_bytes, pb = (size_t)std::min<u64>(pairs, SIZE_MAX / 8) * idx_bytes;
	const StageRow rows[5] = {{start, nb, nb}, {count, nb, nb}, {m ? right_perm : nullptr, mb, mb}, {out_left, 0, pb}, {out_right, 0, pb}};
	return staged_call(*c, "rsx_join_pairs", rows, [&](void *const *d, size_t *back) {
		back[3] = back[4] = pb;
		return rsx_join_pairs_device(d[0], d[1], d[2], n, m, idx_bytes, flags, d[3], d[4], capacity, nullptr, n_pairs);
	});
}

}  // extern "C"
