// rsx_segments_api.hpp: rsx_sort_segments[_device] -- the host driver (the plan of the offsets, then one launch per size class over
// the kernels of rsx_segments.hpp, the existing sorts on the few segments too long for LDS, or rsx_sort_lex_device on (segment, key)
// and a gather) and its entry points; part of librsx.so's host side, included by rsx.hip behind rsx_lex_api.hpp.
#pragma once

namespace {

static_assert((unsigned)SEGMENTS_CLASSES == (unsigned)RSX_SEGMENTS_CLASSES, "rsx.h and rsx_segments_shape.hpp disagree");
static_assert((unsigned)SEGMENTS_MAX_LONG_LISTED == (unsigned)SEGMENTS_MAX_LONG_COMPILED && SEGMENTS_MAX_LONG_DEFAULT <= SEGMENTS_MAX_LONG_COMPILED,
              "rsx_env.hpp and rsx_segments_shape.hpp disagree");

// ---- rsx_sort_segments_device: many independent arrays sorted in one call (rsx_segments.hpp) ---------------------
template <typename KT, typename IT> struct SegmentsArgs {
	const KT *src;
	size_t n;
	const IT *offsets;   // m + 1 entries, or nullptr: m rows of row_len keys
	size_t m;
	u64 row_len;
	KT *out_keys;        // either may be nullptr, not both
	IT *out_idx;
	bool local;          // RSX_SEGMENTS_LOCAL_IDX
};

// segtab = [SegmentsPlan 256][rows (wgs + 1) x 8 u64][starts (wgs + 1) x 8 u64][long table 4096 x 2 u64][list m u32]
struct SegmentsTab {
	SegmentsPlan *plan;
	u64 *rows, *starts, *longtab;
	u32 *list;
};
inline size_t segments_tab_bytes(u32 wgs, size_t m)
{
	return 256 + 2 * (size_t)(wgs + 1) * SEGMENTS_ROW * sizeof(u64) + (size_t)SEGMENTS_MAX_LONG_LISTED * 2 * sizeof(u64) + m * sizeof(u32);
}
inline SegmentsTab segments_tab(void *p, u32 wgs)
{
	SegmentsTab t;
	char *b = (char *)p;
	t.plan = (SegmentsPlan *)b;
	t.rows = (u64 *)(b + 256);
	t.starts = t.rows + (size_t)(wgs + 1) * SEGMENTS_ROW;
	t.longtab = t.starts + (size_t)(wgs + 1) * SEGMENTS_ROW;
	t.list = (u32 *)(t.longtab + (size_t)SEGMENTS_MAX_LONG_LISTED * 2);
	return t;
}
static_assert(sizeof(SegmentsPlan) <= 256, "the plan record has 256 bytes of segtab");

// the plan: from the offsets on the device (checked there, before anything is written), or on the host for uniform rows
template <typename KT, typename IT> int segments_plan(Ctx &c, const SegmentsArgs<KT, IT> &a, u32 cap, SegmentsPlan *plan, SegmentsTab *tab)
{
	memset(plan, 0, sizeof(*plan));
	memset(tab, 0, sizeof(*tab));
	if (!a.offsets) {
		const u32 cls = segments_class(a.row_len, cap);
		plan->max_len = a.row_len;
		plan->count[cls] = plan->listed[cls] = a.m;
		return RSX_OK;
	}
	const SegmentsPlanGrid g = segments_plan_grid((u64)a.m);
	RSX_TRY(c.segtab.ensure(segments_tab_bytes(g.wgs, a.m)));
	RSX_TRY(c.ensure_segplan());
	*tab = segments_tab(c.segtab.p, g.wgs);
	hipLaunchKernelGGL((rsx_segments_plan_kernel<IT, false>), dim3(g.wgs), dim3(SEGMENTS_PLAN_THREADS), 0, c.stream, a.offsets, (u64)a.m, (u64)a.n, cap, g,
	                   tab->rows, (const u64 *)nullptr, (u32 *)nullptr, (u64 *)nullptr);
	hipLaunchKernelGGL(rsx_segments_scan_kernel, dim3(1), dim3(64), 0, c.stream, (const u64 *)tab->rows, tab->starts, g.wgs, tab->plan,
	                   c.dev_host_segplan);
	hipLaunchKernelGGL((rsx_segments_plan_kernel<IT, true>), dim3(g.wgs), dim3(SEGMENTS_PLAN_THREADS), 0, c.stream, a.offsets, (u64)a.m, (u64)a.n, cap, g,
	                   (u64 *)nullptr, (const u64 *)tab->starts, tab->list, tab->longtab);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c.stream));
	*plan = *c.host_segplan;
	if (plan->bad)
		return fail(RSX_EINVAL, "rsx_sort_segments: bad offsets (they must not decrease, offsets[0] must be 0 and offsets[m] must be n = %zu)", a.n);
	return RSX_OK;
}

// one launch of rsx_segments_sort_kernel over a class's part of the list
template <typename KT, typename IT, bool IDX, u32 NW>
int segments_launch(Ctx &c, const SegmentsArgs<KT, IT> &a, const u32 *list, u64 count, u32 cls, u64 max_len, KdfArgs<KT> ka)
{
	const u32 cap = segments_cap((u32)sizeof(KT), IDX);
	const u32 stride = segments_stride(cls, max_len, cap);
	const u32 lds = segments_lds_bytes(cls, (u32)sizeof(KT), IDX, max_len);
	auto kernel = rsx_segments_sort_kernel<KT, IT, IDX, NW>;
	static std::atomic<int> raised_on{-1};   // (per instantiation: the device whose limit of dynamic LDS was raised last)
	if (raised_on.load() != c.device) {
		if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEGMENTS_LDS_BYTES) != hipSuccess)
			(void)hipGetLastError();   // (a runtime that has no such limit to raise)
		raised_on.store(c.device);
	}
	const u64 grid = segments_grid(cls, count);
	if (grid > 0x7FFFFFFFull)
		return fail(RSX_EINVAL, "rsx_sort_segments: %llu workgroups in one launch", (unsigned long long)grid);
	hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(segments_wg_threads(cls)), lds, c.stream, a.src, a.offsets, a.row_len, list, count, ka, stride,
	                   a.out_keys, (void *)a.out_idx, sizeof(IT) == 8, a.local);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// the segments that fit LDS: one launch per class that has any
template <typename KT, typename IT, bool IDX>
int segments_lds(Ctx &c, const SegmentsArgs<KT, IT> &a, const SegmentsPlan &plan, const SegmentsTab &tab, int dtype, int order)
{
	const KdfArgs<KT> ka = make_kdf<KT>(dtype, order);
	for (u32 cls = SEGMENTS_COPY; cls <= SEGMENTS_BLOCK; ++cls) {
		const u64 count = plan.listed[cls];
		if (!count)
			continue;
		const u32 *list = a.offsets ? tab.list + plan.list_start[cls] : nullptr;
		if (cls == SEGMENTS_COPY) {
			const u64 grid = segments_grid(cls, count);
			if (grid > 0x7FFFFFFFull)
				return fail(RSX_EINVAL, "rsx_sort_segments: %llu workgroups in one launch", (unsigned long long)grid);
			hipLaunchKernelGGL((rsx_segments_copy_kernel<KT, IT>), dim3((unsigned)grid), dim3(256), 0, c.stream, a.src, a.offsets, a.row_len, list, count,
			                   a.out_keys, (void *)a.out_idx, sizeof(IT) == 8, a.local);
			HIP_TRY(hipGetLastError());
		} else if (cls == SEGMENTS_WAVE) {
			RSX_TRY((segments_launch<KT, IT, IDX, 1>(c, a, list, count, cls, plan.max_len, ka)));
		} else if (cls == SEGMENTS_GROUP) {
			RSX_TRY((segments_launch<KT, IT, IDX, 4>(c, a, list, count, cls, plan.max_len, ka)));
		} else {
			RSX_TRY((segments_launch<KT, IT, IDX, 16>(c, a, list, count, cls, plan.max_len, ka)));
		}
	}
	return RSX_OK;
}

// MIXED: the segments too long for LDS, one after the other through the plain sorts on their sub-ranges.  Buffers: lex's --
// lexidx = the two halves of a rank sort, lexkeys = [a copy of the segment][the second buffer of its sort] (keys alone are wanted)
template <typename KT, typename IT>
int segments_long(Ctx &c, const SegmentsArgs<KT, IT> &a, const SegmentsPlan &plan, const SegmentsTab &tab, int dtype, int order, rsx_info *si)
{
	const u64 n_long = plan.count[SEGMENTS_LONG];
	std::vector<u64> lt(2 * (size_t)n_long);
	if (a.offsets) {
		HIP_TRY(hipMemcpyAsync(lt.data(), tab.longtab, lt.size() * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
	} else {
		for (u64 i = 0; i < n_long; ++i) {
			lt[2 * i] = i * a.row_len;
			lt[2 * i + 1] = a.row_len;
		}
	}
	for (u64 i = 0; i < n_long; ++i) {
		const u64 start = lt[2 * i], len = lt[2 * i + 1];
		info_clear(si, dtype);
		if (a.out_idx) {
			RSX_TRY(c.lexidx.ensure(2 * (size_t)len * sizeof(IT)));
			void *res = nullptr;
			RSX_TRY((sort_rank_device<KT, IT>(c, a.src + start, (IT *)c.lexidx.p, (size_t)len, dtype, order, &res, si)));
			hipLaunchKernelGGL((rsx_segments_long_kernel<KT, IT>), dim3(small_grid(len, 256, 2048)), dim3(256), 0, c.stream, a.src, (const IT *)res, start,
			                   len, a.out_keys, a.out_idx, a.local);
			HIP_TRY(hipGetLastError());
		} else {
			const size_t stride = ((size_t)len * sizeof(KT) + 255) & ~(size_t)255;
			RSX_TRY(c.lexkeys.ensure(2 * stride));
			KT *k0 = (KT *)c.lexkeys.p, *k1 = (KT *)((char *)c.lexkeys.p + stride);
			HIP_TRY(hipMemcpyAsync(k0, a.src + start, (size_t)len * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
			void *res = nullptr;
			RSX_TRY((sort_keys_device<KT>(c, k0, k1, (size_t)len, dtype, order, &res, si)));
			HIP_TRY(hipMemcpyAsync(a.out_keys + start, res, (size_t)len * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
		}
	}
	return RSX_OK;
}

// LEX: the documented workaround made internal.  segwork = [ids n, of the narrowest type that holds m][the permutation n]
template <typename KT, typename IT, typename DT>
int segments_by_lex(Ctx &c, const SegmentsArgs<KT, IT> &a, int dtype, int order, rsx_lex_info *li)
{
	const size_t n = a.n, idpad = (n * sizeof(DT) + 255) & ~(size_t)255;
	RSX_TRY(c.segwork.ensure(idpad + n * sizeof(IT)));
	DT *ids = (DT *)c.segwork.p;
	IT *perm = (IT *)((char *)c.segwork.p + idpad);
	hipLaunchKernelGGL((rsx_segments_ids_kernel<IT, DT>), dim3(small_grid(n, 256, 4096)), dim3(256), 0, c.stream, a.offsets, a.row_len, (u64)a.m, (u64)n, ids);
	HIP_TRY(hipGetLastError());
	const rsx_lex_col cols[2] = {{ids, (uint32_t)unsigned_dtype(sizeof(DT)), RSX_ASCENDING}, {a.src, (uint32_t)dtype, (uint32_t)order}};
	memset(li, 0, sizeof(*li));
	li->ncols = 2;
	li->pack_bytes = env().lex_pack_bytes;
	lex_plan(cols, 2, li->pack_bytes, li);
	RSX_TRY((sort_lex_device<IT>(c, cols, n, perm, li)));
	hipLaunchKernelGGL((rsx_segments_gather_kernel<KT, IT, DT>), dim3(small_grid(n, 256, 4096)), dim3(256), 0, c.stream, a.src, (const IT *)perm,
	                   (const DT *)ids, a.offsets, a.row_len, (u64)n, a.out_keys, a.out_idx, a.local);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// is the LDS route the default for a call whose segments fall in these classes?  (the measured classes)
inline bool segments_lds_default(const SegmentsPlan &plan)
{
	for (u32 cls = SEGMENTS_WAVE; cls <= SEGMENTS_BLOCK; ++cls)
		if (plan.count[cls] && !((u32)SEGMENTS_DEFAULT_CLASSES >> cls & 1u))
			return false;
	return true;
}

// n > 0 and m > 0
template <typename KT, typename IT>
int sort_segments_device(Ctx &c, const SegmentsArgs<KT, IT> &a, int dtype, int order, rsx_segments_info *info)
{
	const bool with_idx = a.out_idx != nullptr;
	const u32 cap = segments_cap((u32)sizeof(KT), with_idx);
	info->cap = cap;
	SegmentsPlan plan;
	SegmentsTab tab;
	RSX_TRY((segments_plan<KT, IT>(c, a, cap, &plan, &tab)));
	const u64 n_long = plan.count[SEGMENTS_LONG];
	info->max_len = plan.max_len;
	info->n_long = n_long;
	for (u32 cls = 0; cls < SEGMENTS_CLASSES; ++cls)
		info->class_count[cls] = plan.count[cls];
	const u32 force = env().segments_force;
	// (without the verified order of LDS atomics there is no LDS route; more long segments than RSX_SEGMENTS_MAX_LONG: no host loop)
	const bool possible = c.fast && force != 2 && n_long <= env().segments_max_long;
	if (possible && (force == 1 || segments_lds_default(plan))) {
		if (with_idx)
			RSX_TRY((segments_lds<KT, IT, true>(c, a, plan, tab, dtype, order)));
		else
			RSX_TRY((segments_lds<KT, IT, false>(c, a, plan, tab, dtype, order)));
		info->route = RSX_SEGMENTS_LDS;
		if (n_long) {
			info->route = RSX_SEGMENTS_MIXED;
			RSX_TRY((segments_long<KT, IT>(c, a, plan, tab, dtype, order, &info->sort)));
		}
		return RSX_OK;
	}
	info->route = RSX_SEGMENTS_LEX;
	if (a.n == 1) {   // one key: nothing to order
		if (a.out_keys)
			HIP_TRY(hipMemcpyAsync(a.out_keys, a.src, sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
		if (a.out_idx)
			HIP_TRY(hipMemsetAsync(a.out_idx, 0, sizeof(IT), c.stream));
		return RSX_OK;
	}
	switch (segments_id_bytes((u64)a.m)) {
	case 1: return segments_by_lex<KT, IT, uint8_t>(c, a, dtype, order, &info->lex);
	case 2: return segments_by_lex<KT, IT, uint16_t>(c, a, dtype, order, &info->lex);
	default: return segments_by_lex<KT, IT, u32>(c, a, dtype, order, &info->lex);
	}
}

}  // namespace

extern "C" {

/* ---- rsx_sort_segments: many independent arrays sorted in one call (rsx_segments.hpp) ---- */
static int segments_args(const char *who, const void *src, size_t n, const void *offsets, size_t m, size_t idx_bytes, rsx_dtype dtype, rsx_order order,
                         const void *out_keys, const void *out_idx, uint32_t flags)
{
	const size_t kb = dtype_size(dtype);
	if (!kb || (order != RSX_ASCENDING && order != RSX_DESCENDING) || (n && !src) || (flags & ~(uint32_t)RSX_SEGMENTS_LOCAL_IDX))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!out_keys && !out_idx)
		return fail(RSX_EINVAL, "%s: both of out_keys and out_idx are NULL", who);
	if (n && out_keys == src)
		return fail(RSX_EINVAL, "%s: out_keys is src (the sort is not done in place)", who);
	RSX_TRY(idx_args(who, idx_bytes, n, n));   // (an offset may be n itself)
	if ((uint64_t)m > 0xFFFFFFFEull)
		return fail(RSX_EINVAL, "%s: m = %zu does not fit a 4-byte segment number", who, m);
	if (n && out_keys) {
		const uintptr_t s = (uintptr_t)src, k = (uintptr_t)out_keys;
		if (k < s + n * kb && s < k + n * kb)
			return fail(RSX_EINVAL, "%s: out_keys overlaps src", who);
	}
	if (n && m && !offsets && n % m)
		return fail(RSX_EINVAL, "%s: n = %zu is not a whole number of m = %zu rows (offsets is NULL)", who, n, m);
	return RSX_OK;
}

int rsx_sort_segments_device(const void *d_src, size_t n, const void *d_offsets, size_t m, size_t idx_bytes, rsx_dtype dtype, rsx_order order,
                             void *d_out_keys, void *d_out_idx, uint32_t flags, void *stream, rsx_segments_info *info)
{
	rsx_segments_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	RSX_TRY(segments_args("rsx_sort_segments_device", d_src, n, d_offsets, m, idx_bytes, dtype, order, d_out_keys, d_out_idx, flags));
	if (n == 0 || m == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_segments_device", "the call waits for its plan"));
	RSX_DISPATCH_KT_W(dtype, idx_bytes, IT,
	                  return (sort_segments_device<KT, IT>(*c, SegmentsArgs<KT, IT>{(const KT *)d_src, n, (const IT *)d_offsets, m,
	                                                                                 d_offsets ? 0ull : (u64)(n / m), (KT *)d_out_keys,
	                                                                                 (IT *)d_out_idx, (flags & RSX_SEGMENTS_LOCAL_IDX) != 0},
	                                                       dtype, order, info)));
	return RSX_OK;
}

int rsx_sort_segments(const void *src, size_t n, const void *offsets, size_t m, size_t idx_bytes, rsx_dtype dtype, rsx_order order, void *out_keys,
                      void *out_idx, uint32_t flags, rsx_segments_info *info)
{
	rsx_segments_info local;
	info = info_or(info, &local);
	info_clear(&info->sort, dtype);
	info->key_bytes = (uint32_t)dtype_size(dtype);
	const size_t kb = dtype_size(dtype);
	RSX_TRY(segments_args("rsx_sort_segments", src, n, offsets, m, idx_bytes, dtype, order, out_keys, out_idx, flags));
	if (n == 0 || m == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, nullptr);
	const size_t ob = (m + 1) * idx_bytes;
	const StageRow rows[4] = {{src, n * kb, n * kb, STAGE_RECS0}, {offsets, ob, ob}, {out_keys, 0, n * kb}, {out_idx, 0, n * idx_bytes}};
	return staged_call(*c, "rsx_sort_segments", rows, [&](void *const *d, size_t *back) {
		back[2] = n * kb, back[3] = n * idx_bytes;
		return rsx_sort_segments_device(d[0], n, d[1], m, idx_bytes, dtype, order, d[2], d[3], flags, nullptr, info);
	});
}

}  // extern "C"
