// rsx_lex_api.hpp: rsx_sort_lex[_device] -- the host driver (column groups packed by the kernels of rsx_lex.hpp, sorted last group
// first) and its entry points; part of librsx.so's host side, included by rsx.hip behind the routes and rsx_api.hpp.
#pragma once

namespace {

// ---- rsx_sort_lex_device: stable argsort by several key columns (rsx_lex.hpp) ------------------------------------------
// The reference's stability argument one level up: sort by the least significant column first, then stably by the next.
// GROUPING (deterministic; tests assert it): walk from the last column towards column 0 and put a column into the current
// group while the group's bytes plus the column's are at most P = Env::lex_pack_bytes; a column wider than P is a group of
// its own.  group[0] holds the LAST columns and is sorted first.
void lex_plan(const rsx_lex_col *cols, size_t ncols, u32 P, rsx_lex_info *info)
{
	u32 ng = 0, bytes = 0;
	size_t end = ncols;   // one past the last column of the group being filled
	auto emit = [&](size_t first) {
		rsx_lex_group &g = info->group[ng++];
		g.first_col = (u32)first;
		g.ncols = (u32)(end - first);
		g.key_bytes = bytes;
		g.sorted_as = (ng == 1 && g.ncols == 1) ? cols[first].dtype : bytes <= 2 ? (u32)RSX_U16 : bytes <= 4 ? (u32)RSX_U32 : (u32)RSX_U64;
	};
	for (size_t ci = ncols; ci-- > 0;) {
		const u32 w = (u32)dtype_size((int)cols[ci].dtype);
		if (bytes && bytes + w > P) {
			emit(ci + 1);
			end = ci + 1;
			bytes = 0;
		}
		bytes += w;
	}
	emit(0);
	info->ngroups = ng;
}

// the kernel's descriptors of one group: the group's first column in the highest bits used
LexArgs lex_args(const rsx_lex_col *cols, const rsx_lex_group &g, const void *perm)
{
	LexArgs a;
	memset(&a, 0, sizeof(a));
	a.ncols = g.ncols;
	a.perm_vec = (((uintptr_t)perm) & 15) == 0;
	u32 shift = 8 * g.key_bytes;
	for (u32 j = 0; j < g.ncols; ++j) {
		const rsx_lex_col &col = cols[g.first_col + j];
		const u32 w = (u32)dtype_size((int)col.dtype);
		shift -= 8 * w;
		LexCol &d = a.col[j];
		d.p = col.data;
		d.wlog2 = w == 1 ? 0u : w == 2 ? 1u : w == 4 ? 2u : 3u;
		d.shift = shift;
		d.vec = (((uintptr_t)col.data) & (4 * w - 1)) == 0;
		switch (w) {
		case 1: { const KdfArgs<uint8_t> k = make_kdf<uint8_t>((int)col.dtype, (int)col.order); d.fmask = k.fmask; d.sflip = k.sflip; d.desc = k.desc; } break;
		case 2: { const KdfArgs<uint16_t> k = make_kdf<uint16_t>((int)col.dtype, (int)col.order); d.fmask = k.fmask; d.sflip = k.sflip; d.desc = k.desc; } break;
		case 4: { const KdfArgs<u32> k = make_kdf<u32>((int)col.dtype, (int)col.order); d.fmask = k.fmask; d.sflip = k.sflip; d.desc = k.desc; } break;
		default: { const KdfArgs<u64> k = make_kdf<u64>((int)col.dtype, (int)col.order); d.fmask = k.fmask; d.sflip = k.sflip; d.desc = k.desc; } break;
		}
	}
	return a;
}

// one group's keys packed (*cur == nullptr: group 0) or gathered through *cur, then sorted: group 0 by the rank sort, which
// makes the permutation; every later group by the key + payload sort with the permutation as payload (*cur / *other: where it
// is, and the second buffer of its sort)
template <typename OT, typename IT>
int lex_sort_group(Ctx &c, const rsx_lex_col *cols, const rsx_lex_group &g, size_t n, OT *k0, OT *k1, IT *base, IT *alt, IT **cur, IT **other,
                   rsx_info *si)
{
	const LexArgs a = lex_args(cols, g, *cur);
	const u64 quads = (u64)n / 4;
	const dim3 grid((unsigned)std::max<u64>(1, std::min<u64>(LEX_MAX_GRID, (quads + LEX_THREADS - 1) / LEX_THREADS))), block(LEX_THREADS);
	if (!*cur) {
		hipLaunchKernelGGL((rsx_lex_pack_kernel<OT, u32, false>), grid, block, 0, c.stream, a, (const u32 *)nullptr, k0, (u64)n);
		HIP_TRY(hipGetLastError());
		void *res = nullptr;
		RSX_TRY((sort_rank_device<OT, IT>(c, (const OT *)k0, base, n, (int)g.sorted_as, RSX_ASCENDING, &res, si)));
		*cur = (IT *)res;
		*other = *cur == base ? alt : base;
		return RSX_OK;
	}
	hipLaunchKernelGGL((rsx_lex_pack_kernel<OT, IT, true>), grid, block, 0, c.stream, a, (const IT *)*cur, k0, (u64)n);
	HIP_TRY(hipGetLastError());
	RSX_TRY((sort_pairs_device<OT, IT>(c, k0, k1, *cur, *other, n, (int)g.sorted_as, RSX_ASCENDING, si)));
	if (si->result_in_aux)
		std::swap(*cur, *other);
	return RSX_OK;
}

template <typename IT>
int sort_lex_device(Ctx &c, const rsx_lex_col *cols, size_t n, IT *out, rsx_lex_info *info)
{
	// Buffers of this call's own, apart from everything the inner sorts use themselves (Ctx::keys, vals, seg, slack*, ...):
	// [keys n][keys n] of the widest packed type, and indices [n][n][n] -- the rank sort of group 0 works in the first two
	// (contiguous, as rsx_sort_rank_device wants them) and leaves the permutation in one of them; the second buffer of the
	// key + payload sorts is the first one, or the third where the first holds the permutation (256-byte aligned both).
	size_t widest = 0;
	for (u32 gi = 0; gi < info->ngroups; ++gi) {
		const rsx_lex_group &g = info->group[gi];
		if (gi > 0 || g.ncols > 1)
			widest = std::max<size_t>(widest, dtype_size((int)g.sorted_as));
	}
	const size_t kstride = (n * widest + 255) & ~(size_t)255, istride = (2 * n * sizeof(IT) + 255) & ~(size_t)255;
	if (widest)
		RSX_TRY(c.lexkeys.ensure(2 * kstride));
	RSX_TRY(c.lexidx.ensure(istride + n * sizeof(IT)));
	IT *base = (IT *)c.lexidx.p, *alt = (IT *)((char *)c.lexidx.p + istride), *cur = nullptr, *other = nullptr;
	void *k0 = c.lexkeys.p, *k1 = (char *)c.lexkeys.p + kstride;
	bool all_in_order = true;
	for (u32 gi = 0; gi < info->ngroups; ++gi) {
		rsx_lex_group &g = info->group[gi];
		rsx_info si;
		info_clear(&si, (int)g.sorted_as);
		if (gi == 0 && g.ncols == 1) {
			// a lone column: the rank sort on the caller's column itself, with its own type and order -- no copy, no kernel
			const rsx_lex_col &col = cols[g.first_col];
			void *res = nullptr;
			int rc = RSX_EINVAL;
			RSX_DISPATCH_KT((int)col.dtype, rc = (sort_rank_device<KT, IT>(c, (const KT *)col.data, base, n, (int)col.dtype, (int)col.order, &res, &si)));
			RSX_TRY(rc);
			cur = (IT *)res;
			other = cur == base ? alt : base;
		} else if (g.sorted_as == RSX_U16) {
			RSX_TRY((lex_sort_group<uint16_t, IT>(c, cols, g, n, (uint16_t *)k0, (uint16_t *)k1, base, alt, &cur, &other, &si)));
		} else if (g.sorted_as == RSX_U32) {
			RSX_TRY((lex_sort_group<u32, IT>(c, cols, g, n, (u32 *)k0, (u32 *)k1, base, alt, &cur, &other, &si)));
		} else {
			RSX_TRY((lex_sort_group<u64, IT>(c, cols, g, n, (u64 *)k0, (u64 *)k1, base, alt, &cur, &other, &si)));
		}
		g.kept_cols = si.ncols;
		g.hybrid = si.hybrid;
		g.in_order = si.early_exit == 2;   // (the pre-sorted exit: group 0 has written 0 .. n-1, a later group left the permutation where it was)
		all_in_order = all_in_order && g.in_order;
	}
	if (all_in_order)
		info->early_exit = 2;
	HIP_TRY(hipMemcpyAsync(out, cur, n * sizeof(IT), hipMemcpyDeviceToDevice, c.stream));
	return RSX_OK;
}

}  // namespace

extern "C" {

/* ---- rsx_sort_lex: stable argsort by several key columns (rsx_lex.hpp) ---- */
static int lex_args_check(const char *who, const rsx_lex_col *cols, size_t ncols, size_t n, const void *out_idx, size_t idx_bytes)
{
	if (!cols)
		return fail(RSX_EINVAL, "%s: cols is NULL", who);
	if (ncols == 0 || ncols > RSX_LEX_MAX_COLS)
		return fail(RSX_EINVAL, "%s: ncols = %zu (1 .. %d columns)", who, ncols, (int)RSX_LEX_MAX_COLS);
	for (size_t i = 0; i < ncols; ++i) {
		if (!dtype_size((int)cols[i].dtype))
			return fail(RSX_EINVAL, "%s: column %zu: unknown dtype %u", who, i, cols[i].dtype);
		if (cols[i].order != RSX_ASCENDING && cols[i].order != RSX_DESCENDING)
			return fail(RSX_EINVAL, "%s: column %zu: unknown order %u", who, i, cols[i].order);
		if (n && !cols[i].data)
			return fail(RSX_EINVAL, "%s: column %zu is NULL", who, i);
	}
	RSX_TRY(idx_args(who, idx_bytes, n, out_idx ? idx_last(n) : 0));   // (a missing output is reported before an n that does not fit)
	if (n && !out_idx)
		return fail(RSX_EINVAL, "%s: the output is NULL", who);
	return RSX_OK;
}

static rsx_lex_info *lex_info(rsx_lex_info *info, rsx_lex_info *local, size_t ncols, size_t n)
{
	info = info_or(info, local);
	info->ncols = (uint32_t)std::min<size_t>(ncols, RSX_LEX_MAX_COLS);
	info->pack_bytes = env().lex_pack_bytes;
	info->early_exit = n < 2 ? 1 : 0;
	return info;
}

int rsx_sort_lex_device(const rsx_lex_col *cols, size_t ncols, size_t n, void *d_out_idx, size_t idx_bytes, void *stream, rsx_lex_info *info)
{
	rsx_lex_info local;
	info = lex_info(info, &local, ncols, n);
	RSX_TRY(lex_args_check("rsx_sort_lex_device", cols, ncols, n, d_out_idx, idx_bytes));
	if (n == 0)
		return RSX_OK;
	RSX_LOCKED_CTX(c, stream);
	RSX_TRY(refuse_capture(stream, "rsx_sort_lex_device", "the call waits between its sorts"));
	if (n == 1) {
		HIP_TRY(hipMemsetAsync(d_out_idx, 0, idx_bytes, c->stream));
		return RSX_OK;
	}
	lex_plan(cols, ncols, info->pack_bytes, info);
	if (idx_bytes == 4)
		return sort_lex_device<u32>(*c, cols, n, (u32 *)d_out_idx, info);
	return sort_lex_device<u64>(*c, cols, n, (u64 *)d_out_idx, info);
}

int rsx_sort_lex(const rsx_lex_col *cols, size_t ncols, size_t n, void *out_idx, size_t idx_bytes, rsx_lex_info *info)
{
	rsx_lex_info local;
	info = lex_info(info, &local, ncols, n);
	RSX_TRY(lex_args_check("rsx_sort_lex", cols, ncols, n, out_idx, idx_bytes));
	if (n == 0)
		return RSX_OK;
	// one row, every pointer the host's: index 0 (with a device's pointer among them the call goes on, to its error if they are mixed)
	bool on_host = one_on_host(n, out_idx);
	for (size_t i = 0; on_host && i < ncols; ++i)
		on_host = one_on_host(n, cols[i].data);
	if (on_host) {
		memset(out_idx, 0, idx_bytes);
		return RSX_OK;
	}
	RSX_LOCKED_CTX(c, nullptr);
	const void *ps[RSX_LEX_MAX_COLS + 1];
	for (size_t i = 0; i < ncols; ++i)
		ps[i] = cols[i].data;
	ps[ncols] = out_idx;
	const PtrKind kind = pointer_kind(ps, ncols + 1);
	if (kind == PTR_MIXED)
		return mixed_pointers("rsx_sort_lex");
	if (kind == PTR_DEVICE) {
		RSX_TRY(rsx_sort_lex_device(cols, ncols, n, out_idx, idx_bytes, nullptr, info));
		HIP_TRY(hipStreamSynchronize(c->stream));
		return RSX_OK;
	}
	// host buffers: every DISTINCT column staged once, a slot each, and one for the n indices, which are brought back
	rsx_lex_col dcols[RSX_LEX_MAX_COLS];
	size_t bytes[RSX_LEX_MAX_COLS + 1], off[RSX_LEX_MAX_COLS + 1], first[RSX_LEX_MAX_COLS];
	for (size_t i = 0; i < ncols; ++i) {
		const size_t w = dtype_size((int)cols[i].dtype);
		size_t j = 0;
		while (j < i && !(cols[j].data == cols[i].data && dtype_size((int)cols[j].dtype) == w))
			++j;
		first[i] = j;
		bytes[i] = j == i ? n * w : STAGE_ABSENT;
	}
	bytes[ncols] = n * idx_bytes;
	RSX_TRY(c->stage.ensure(stage_layout(bytes, ncols + 1, off)));
	char *stage = (char *)c->stage.p;
	for (size_t i = 0; i < ncols; ++i) {
		dcols[i] = cols[i];
		dcols[i].data = stage + off[first[i]];
		if (first[i] == i)
			HIP_TRY(hipMemcpyAsync(stage + off[i], cols[i].data, bytes[i], hipMemcpyHostToDevice, c->stream));
	}
	RSX_TRY(rsx_sort_lex_device(dcols, ncols, n, stage + off[ncols], idx_bytes, nullptr, info));
	HIP_TRY(hipMemcpyAsync(out_idx, stage + off[ncols], n * idx_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return RSX_OK;
}

}  // extern "C"
