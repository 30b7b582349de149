// rsx_keybits_api.hpp: what the host drivers of rsx_sort_unique*, rsx_sort_group* and rsx_sort_rankdata* share -- the front end (a
// sample of the keys, the plan, the varying bits), the bitmap of the packed values, the heads of a sorted array, the index sort of a
// workspace copy and its keys-only counterpart, single indices (the arithmetic: rsx_keybits.hpp); part of librsx.so's host side,
// included by rsx.hip behind the routes and rsx_api.hpp, in front of the three drivers.
#pragma once

namespace {

static_assert(KEYBITS_CHUNK_WORDS == UNIQUE_CHUNK_WORDS, "bitmap_shape counts the read-out's chunks");

// ---- the front end: which bits of the keys vary -----------------------------------------------------------------------------
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

struct KeyBits {
	bool planned = false;   // false: the sample sent the keys to the sort, and nothing below is known
	Plan plan{};
	u64 vary = 0;           // the bits of the KDF key that are not the same in all keys
	u32 vbits = 0;          // ... how many
	bool sorted = false;    // the plan found the input in order
};

// The sample can only PROVE that many bits vary (a bit that differs between two sampled keys differs among the keys): more than
// `sample_limit` -- what the largest bitmap or table of the caller takes -- and the keys go to the sort as if the entry point were
// the sort's.  Else the plan, read out into the caller's info.
template <typename KT>
int keybits_front(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, u32 sample_limit, rsx_info *sort, uint32_t *varying_bits, KeyBits *kb)
{
	RSX_TRY(c.urecs.ensure(64 + 64 * sizeof(UniqueRec)));
	if (unique_sample_wanted<KT>(c, n)) {
		const u64 init[2] = {0, ~0ull};
		u64 got[2];
		HIP_TRY(hipMemcpyAsync(unique_hdr(c), init, sizeof init, hipMemcpyHostToDevice, c.stream));
		hipLaunchKernelGGL((rsx_unique_sample_kernel<KT>), dim3(1), dim3(1024), 0, c.stream, src, (u64)n, ka, unique_hdr(c));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(got, unique_hdr(c), sizeof got, hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
		if ((u32)__builtin_popcountll(got[0] ^ got[1]) > sample_limit)
			return RSX_OK;
	}
	RSX_TRY(plan_phase<KT>(c, src, n, ka, &kb->plan, 0));
	kb->planned = true;
	info_from_plan(sort, kb->plan);
	kb->vary = ((u64)kb->plan.vary_hi << 32) | kb->plan.vary_lo;
	kb->vbits = (u32)__builtin_popcountll(kb->vary);
	*varying_bits = kb->vbits;
	kb->sorted = kb->plan.sorted != 0;
	if (kb->sorted)
		sort->early_exit = 2;
	return RSX_OK;
}

// ---- the bitmap: every key sets the bit of its packed value, the set bits are counted per chunk and scanned -------------------
// `s` = bitmap_shape(vbits).  *done = 0: no room (not an error: the caller takes the sort).  Behind it the records say where each
// chunk's distinct keys begin and the header holds their number (unique_total): the caller reads the bitmap out.
template <typename KT>
int keybits_bitmap(Ctx &c, const KT *src, size_t n, KdfArgs<KT> ka, u64 vary, const BitRuns &runs, const BitmapShape &s, int *done)
{
	static_assert(sizeof(KT) >= 2, "one-byte keys have one column: the callers keep the mark kernels out of their build");
	*done = 0;
	if (c.ubits.ensure(s.bytes) != RSX_OK || c.urecs.ensure(64 + (size_t)s.chunks * sizeof(UniqueRec)) != RSX_OK)
		return RSX_OK;
	u32 *bitmap = (u32 *)c.ubits.p;
	HIP_TRY(hipMemsetAsync(bitmap, 0, s.bytes, c.stream));
	const unsigned grid = sweep_grid(n, sizeof(KT), s.full);
	if (s.lds_bits == 16)
		hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 16>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
	else if (s.lds_bits == 18)
		hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 18>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
	else if (s.lds_bits == 20)
		hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 20>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
	else
		hipLaunchKernelGGL((rsx_unique_mark_kernel<KT, 0>), dim3(grid), dim3(1024), 0, c.stream, src, (u64)n, ka, runs, bitmap);
	hipLaunchKernelGGL((rsx_unique_expand_kernel<KT, 0>), dim3((unsigned)s.chunks), dim3(256), 0, c.stream, (const u32 *)bitmap,
	                   unique_recs(c), (KT *)nullptr, src, ka, runs, (KT)vary);
	hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(1024), 0, c.stream, unique_recs(c), s.chunks, unique_hdr(c));
	*done = 1;
	return RSX_OK;
}

// ---- the heads of the sorted array `in`: counted per tile and scanned.  *tiles: the grid of the pass that writes by them -------
template <typename KT> int keybits_heads(Ctx &c, const KT *in, size_t n, u64 *tiles)
{
	*tiles = ((u64)n + unique_heads_tile<KT>() - 1) / unique_heads_tile<KT>();
	RSX_TRY(c.urecs.ensure(64 + (size_t)*tiles * sizeof(UniqueRec)));
	hipLaunchKernelGGL((rsx_unique_heads_kernel<KT, 0>), dim3((unsigned)*tiles), dim3(UNIQUE_HEADS_THREADS), 0, c.stream, in, (u64)n, unique_recs(c),
	                   (KT *)nullptr, (void *)nullptr, 0u);
	hipLaunchKernelGGL(rsx_unique_scan_kernel, dim3(1), dim3(1024), 0, c.stream, unique_recs(c), *tiles, unique_hdr(c));
	return RSX_OK;
}

// ---- the stable key + index sort of a workspace copy of the keys (keys[0], keys[1]; the indices in the halves of vals[0]) ------
// ... none where the plan found the input `sorted`: the keys themselves, no permutation
template <typename KT, typename IT> struct IndexSorted {
	const KT *in;      // the keys in order
	const IT *perm;    // where each of them stood
	IT *spare;         // n indices nobody holds: the half of vals[0] the result is not in
};
template <typename KT, typename IT>
int keybits_index_sort(Ctx &c, const KT *src, size_t n, int dtype, int order, bool sorted, rsx_info *sort, IndexSorted<KT, IT> *r)
{
	*r = IndexSorted<KT, IT>{src, nullptr, nullptr};
	if (sorted)
		return RSX_OK;
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
	*sort = si;
	*r = si.result_in_aux ? IndexSorted<KT, IT>{k1, v1, v0} : IndexSorted<KT, IT>{k0, v0, v1};
	return RSX_OK;
}

// ... and the keys-only sort of such a copy (keys[0], keys[1]): *sorted = the keys in order (rsx_sort_locate*, rsx_sort_join*)
template <typename KT> int keybits_keys_sort(Ctx &c, const KT *src, size_t n, int dtype, int order, rsx_info *sort, const KT **sorted)
{
	RSX_TRY(c.keys[0].ensure(n * sizeof(KT)));
	RSX_TRY(c.keys[1].ensure(n * sizeof(KT)));
	HIP_TRY(hipMemcpyAsync(c.keys[0].p, src, n * sizeof(KT), hipMemcpyDeviceToDevice, c.stream));
	void *res = nullptr;
	RSX_TRY(sort_keys_device<KT>(c, (KT *)c.keys[0].p, (KT *)c.keys[1].p, n, dtype, order, &res, sort));
	*sorted = (const KT *)res;
	return RSX_OK;
}

// ---- one index or count of 4 or 8 bytes: on the host; on the device, through with the copy before `v` goes out of scope -------
inline void put_index(void *p, size_t idx_bytes, u64 v)
{
	if (idx_bytes == 4)
		*(uint32_t *)p = (uint32_t)v;
	else
		*(uint64_t *)p = v;
}
inline int put_index_device(void *d, size_t idx_bytes, u64 v, hipStream_t stream)
{
	const u32 v32 = (u32)v;
	HIP_TRY(hipMemcpyAsync(d, idx_bytes == 4 ? (const void *)&v32 : (const void *)&v, idx_bytes, hipMemcpyHostToDevice, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	return RSX_OK;
}

}  // namespace
