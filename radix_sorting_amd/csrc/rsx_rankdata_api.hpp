// rsx_rankdata_api.hpp: rsx_sort_rankdata[_device] -- the host driver (routes by one column's offsets, the count table of the packed
// varying bits or sort + runs over the kernels of rsx_rankdata.hpp, rsx_group.hpp and rsx_unique.hpp) and its entry points; part of
// librsx.so's host side, included by rsx.hip behind rsx_group_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_rankdata_device: every element's place in the sorted order (rsx_rankdata.hpp) ---------------------
// what the call writes: each may be nullptr
template <typename IT> struct RankdataOut {
	IT *place;
	IT *less;
	IT *equal;
};

enum : size_t { RANKDATA_TAB16_BYTES = 65536 * sizeof(u32) + 65537 * sizeof(u64) };

// route 1, the place: three ordinary launches over one kept column.  *done = 0: no room for the table.
template <typename KT, typename IT>
int rankdata_place(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, u32 col, IT *place, rsx_rankdata_info *info, int *done)
{
	*done = 0;
	const u64 per = ((u64)n + RANKDATA_PLACE_MAX_WGS - 1) / RANKDATA_PLACE_MAX_WGS;
	const u64 share = (per + RANKDATA_PLACE_TILE - 1) / RANKDATA_PLACE_TILE * RANKDATA_PLACE_TILE;
	const u32 wgs = (u32)(((u64)n + share - 1) / share);
	const size_t bytes = (size_t)wgs * 256 * sizeof(u64);
	if (c.rdtab.ensure(bytes) != RSX_OK)
		return RSX_OK;   // (not an error: the caller takes the sort)
	u64 *tab = (u64 *)c.rdtab.p;
	const u64 *offs = (const u64 *)(c.ghist() + 256 * col);
	hipLaunchKernelGGL((rsx_rankdata_digits_kernel<KT>), dim3(wgs), dim3(RANKDATA_PLACE_THREADS), 0, c.stream, src, (u64)n, share, 8 * col, ka, tab);
	hipLaunchKernelGGL(rsx_rankdata_bases_kernel, dim3(1), dim3(1024), 0, c.stream, tab, wgs, offs);
	hipLaunchKernelGGL((rsx_rankdata_place_kernel<KT, IT>), dim3(wgs), dim3(RANKDATA_PLACE_THREADS), 0, c.stream, src, (u64)n, share, 8 * col, ka,
	                   (const u64 *)tab, place);
	HIP_TRY(hipGetLastError());
	info->table_bytes += bytes;
	*done = 1;
	return RSX_OK;
}

// less and equal of every key from the exclusive offsets of its packed value (in_lds: one column's 256, else 65537)
template <typename KT, typename IT>
int rankdata_lookup(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, const BitRuns &runs, const u64 *offs, bool in_lds, IT *less, IT *equal)
{
	// (as group_lookup: two workgroups of 1024 threads fill a CU, each with a few sweeps of its own)
	const unsigned grid = sweep_grid(n, sizeof(KT));
	if (in_lds)
		hipLaunchKernelGGL((rsx_rankdata_lookup_kernel<KT, IT, true>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, offs, less, equal);
	else
		hipLaunchKernelGGL((rsx_rankdata_lookup_kernel<KT, IT, false>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, offs, less, equal);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// route 2: the counts of the packed varying bits (at most 16 of them), their scan, the lookup.  *done = 0: no room.
template <typename KT, typename IT>
int rankdata_count16(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, const BitRuns &runs, IT *less, IT *equal, rsx_rankdata_info *info, int *done)
{
	*done = 0;
	if constexpr (sizeof(KT) >= 2) {
		if (c.rdtab.ensure(RANKDATA_TAB16_BYTES) != RSX_OK)
			return RSX_OK;
		u32 *jt = (u32 *)c.rdtab.p;
		u64 *offs = (u64 *)((char *)c.rdtab.p + 65536 * sizeof(u32));
		HIP_TRY(hipMemsetAsync(jt, 0, 65536 * sizeof(u32), c.stream));
		hipLaunchKernelGGL((rsx_rankdata_count16_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, jt);
		hipLaunchKernelGGL(rsx_rankdata_scan16_kernel, dim3(1), dim3(1024), 0, c.stream, (const u32 *)jt, offs, (u64)n);
		HIP_TRY(hipGetLastError());
		RSX_TRY((rankdata_lookup<KT, IT>(c, src, n, ka, runs, offs, false, less, equal)));
		info->route = RSX_RANKDATA_COUNT16;
		info->table_bytes = RANKDATA_TAB16_BYTES;
		*done = 1;
	}
	return RSX_OK;
}

// route 3: the stable key + index sort of a workspace copy as group_by_sort sets it up (none where the plan found the input
// sorted), then the permutation inverted, or -- for less and equal -- the heads, their positions and the runs pass
template <typename KT, typename IT>
int rankdata_by_sort(Ctx &c, const KT *src, size_t n, int dtype, int order, bool sorted, const RankdataOut<IT> &out, rsx_rankdata_info *info)
{
	info->route = RSX_RANKDATA_SORT;
	IndexSorted<KT, IT> s;
	RSX_TRY((keybits_index_sort<KT, IT>(c, src, n, dtype, order, sorted, &info->sort, &s)));
	if (!out.less && !out.equal) {
		if (s.perm)
			hipLaunchKernelGGL((rsx_rankdata_inverse_kernel<IT>), dim3(2048), dim3(256), 0, c.stream, s.perm, (u64)n, out.place);
		else
			hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, out.place, (u64)n);
		HIP_TRY(hipGetLastError());
		return RSX_OK;
	}
	if (!s.spare) {
		RSX_TRY(c.vals[0].ensure(((n + 63) & ~(size_t)63) * sizeof(IT)));
		s.spare = (IT *)c.vals[0].p;
	}
	u64 tiles;
	RSX_TRY(keybits_heads<KT>(c, s.in, n, &tiles));
	// (the positions of the heads: what rsx_group_heads_kernel calls `first` over the identity permutation)
	hipLaunchKernelGGL((rsx_group_heads_kernel<KT, IT>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, s.in, (const IT *)nullptr, (u64)n,
	                   (const UniqueRec *)unique_recs(c), (IT *)nullptr, (KT *)nullptr, (IT *)nullptr, s.spare);
	hipLaunchKernelGGL((rsx_rankdata_runs_kernel<KT, IT>), dim3((unsigned)tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, s.in, s.perm, (u64)n,
	                   (const UniqueRec *)unique_recs(c), (const IT *)s.spare, (const u64 *)unique_hdr(c), out.place, out.less, out.equal);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

template <typename KT, typename IT>
int sort_rankdata_device(Ctx &c, const KT *src, size_t n, int dtype, int order, const RankdataOut<IT> &out, rsx_rankdata_info *info)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	const bool tables = !env().rankdata_no_tables;
	KeyBits kb;
	// (the place: one kept column at most)
	RSX_TRY(keybits_front<KT>(c, src, n, ka, !tables ? 0u : out.place ? 8u : 16u, &info->sort, &info->varying_bits, &kb));
	if (kb.planned) {
		const Plan &plan = kb.plan;
		if (kb.vary == 0) {
			// every key equal: the input order is the sorted order, nothing is smaller, all n are equal
			info->route = RSX_RANKDATA_TRIVIAL;
			if (out.place)
				hipLaunchKernelGGL((rsx_iota_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, out.place, (u64)n);
			if (out.less)
				HIP_TRY(hipMemsetAsync(out.less, 0, n * sizeof(IT), c.stream));
			if (out.equal)
				hipLaunchKernelGGL((rsx_rankdata_fill_kernel<IT>), dim3(1024), dim3(256), 0, c.stream, out.equal, (u64)n, (IT)n);
			HIP_TRY(hipGetLastError());
			return RSX_OK;
		}
		if (tables && plan.ncols == 1) {
			// one kept column: its 256 exclusive offsets lie in the plan's histogram -- less and equal are lookups, the place is
			// the address a counting sort's scatter would compute
			const u32 col = plan.cols[0];
			info->table_bytes = 256 * sizeof(u64);
			int done = 1;
			if (out.place)
				RSX_TRY((rankdata_place<KT, IT>(c, src, n, ka, col, out.place, info, &done)));
			if (done) {
				if (out.less || out.equal)
					RSX_TRY((rankdata_lookup<KT, IT>(c, src, n, ka, column_runs(col), (const u64 *)(c.ghist() + 256 * col), true, out.less,
					                                 out.equal)));
				info->route = RSX_RANKDATA_TABLE;
				return RSX_OK;
			}
			info->table_bytes = 0;
		}
		BitRuns runs;
		// (2^16 counters are what the LDS scheme holds, and a counter of 32 bits may have to hold n)
		if (tables && !out.place && sizeof(KT) >= 2 && kb.vbits <= 16 && (u64)n < (1ull << 32) && bit_runs(kb.vary, &runs)) {
			int done = 0;
			RSX_TRY((rankdata_count16<KT, IT>(c, src, n, ka, runs, out.less, out.equal, info, &done)));
			if (done)
				return RSX_OK;
		}
	}
	return rankdata_by_sort<KT, IT>(c, src, n, dtype, order, kb.sorted, out, info);
}

}  // namespace

extern "C" {

/* ---- rsx_sort_rankdata: every element's place in the sorted order (rsx_rankdata.hpp) ---- */
static int rankdata_args(const char *who, const void *src, size_t n, rsx_dtype dtype, rsx_order order, const void *place, const void *less,
                         const void *equal, size_t idx_bytes)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || (n && !src))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!place && !less && !equal)
		return fail(RSX_EINVAL, "%s: all three outputs are NULL", who);
	return idx_args(who, idx_bytes, n, n);   // (equal may be n itself)
}

int rsx_sort_rankdata_device(const void *d_src, size_t n, rsx_dtype dtype, rsx_order order, void *d_out_place, void *d_out_less,
                             void *d_out_equal, size_t idx_bytes, void *stream, rsx_rankdata_info *info)
{
	rsx_rankdata_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	RSX_TRY(rankdata_args("rsx_sort_rankdata_device", d_src, n, dtype, order, d_out_place, d_out_less, d_out_equal, idx_bytes));
	if (n == 0) {
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_rankdata_device", "the call waits for the plan of the keys"));
	if (n == 1) {
		// (one key: at place 0, nothing below it, itself equal)
		if (d_out_place)
			HIP_TRY(hipMemsetAsync(d_out_place, 0, idx_bytes, c->stream));
		if (d_out_less)
			HIP_TRY(hipMemsetAsync(d_out_less, 0, idx_bytes, c->stream));
		if (d_out_equal)
			RSX_TRY(put_index_device(d_out_equal, idx_bytes, 1, c->stream));
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_rankdata_device<KT, IT>(*c, (const KT *)d_src, n, dtype, order,
	                                                       RankdataOut<IT>{(IT *)d_out_place, (IT *)d_out_less, (IT *)d_out_equal}, info)));
	return RSX_OK;
}

int rsx_sort_rankdata(const void *src, size_t n, rsx_dtype dtype, rsx_order order, void *out_place, void *out_less, void *out_equal,
                      size_t idx_bytes, rsx_rankdata_info *info)
{
	rsx_rankdata_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(rankdata_args("rsx_sort_rankdata", src, n, dtype, order, out_place, out_less, out_equal, idx_bytes));
	if (n == 0) {
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	if (one_on_host(n, src)) {
		if (out_place)
			memset(out_place, 0, idx_bytes);
		if (out_less)
			memset(out_less, 0, idx_bytes);
		if (out_equal)
			put_index(out_equal, idx_bytes, 1);
		info->sort.early_exit = 1;
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const StageRow rows[4] = {{src, n * kb, n * kb, STAGE_RECS0}, {out_place, 0, n * idx_bytes}, {out_less, 0, n * idx_bytes},
	                          {out_equal, 0, n * idx_bytes}};
	return staged_call(*c, "rsx_sort_rankdata", rows, [&](void *const *d, size_t *back) {
		back[1] = back[2] = back[3] = n * idx_bytes;
		return rsx_sort_rankdata_device(d[0], n, dtype, order, d[1], d[2], d[3], idx_bytes, nullptr, info);
	});
}

}  // extern "C"
