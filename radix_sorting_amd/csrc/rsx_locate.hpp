// rsx_locate.hpp -- the kernels of rsx_sort_locate_device: where given values fall in the sorted order of the keys (less, equal per
// value) and which of the values' bins every key falls in (README.md "Counting sort": the prefix sums of the counts answer it --
// here the counts are of the keys BETWEEN the values, one read of the keys, nothing sorted).  The arithmetic is rsx_locate_shape.hpp's.
//
//   rsx_locate_prepare_kernel     the sorted values -> the distinct edges E, cum (values at or below each edge), the start table,
//                                 the number of halvings; one workgroup, stops counting behind the cut-off
//   rsx_locate_search_kernel      the search route's one read of the keys: per key a start-table lookup and `steps` halvings over
//                                 the edges in LDS, an LDS add nobody waits for into one of R sets of counters, the bin read
//                                 from cum; a workgroup ends by storing its summed counters as one row
//   rsx_locate_colsum_kernel      the rows summed by column
//   rsx_locate_finish_kernel      the bin totals scanned, less / equal of every caller value read at its edge
//   rsx_locate_scan256_kernel     the table route of 1-byte keys: 256 counts -> exclusive offsets
//   rsx_locate_descents_kernel    the sort route: is the input in order already?
//   rsx_locate_sorted_values_kernel   ... two binary searches per value over the sorted keys
//   rsx_locate_sorted_bins_kernel     ... one binary search per key over the sorted values, its top levels from a sample in LDS
//
// No kernel here adds to device memory atomically, none waits for another workgroup: the counters are LDS adds whose return
// value nobody reads (their order does not matter: they are sums), rows and totals are plain stores.
#pragma once

#include "rsx_locate_shape.hpp"
#include "rsx_rankdata.hpp"

namespace rsx {

// [D, shift, steps, pad] as the prepare kernel leaves it for the host
struct LocateHdr {
	u32 distinct, shift, steps, pad;
};

// sv[0 .. m): the caller's values in sorted order (raw; ascending in K).  E[d] = the d-th distinct derived key, cum[d] = the
// position of its first occurrence = the values below it (cum[D] = m), for d < max_d; counting stops once more than max_d
// heads are seen (hdr->distinct = what was counted by then, > max_d: the caller takes the sort route).  Otherwise start[0 .. 256]
// and hdr->shift / steps by rsx_locate_shape.hpp's rules.
template <typename KT>
__global__ __launch_bounds__(LOCATE_THREADS) void rsx_locate_prepare_kernel(const KT *__restrict__ sv, u64 m, KdfArgs<KT> ka, u32 max_d,
                                                                            KT *__restrict__ E, u64 *__restrict__ cum,
                                                                            u32 *__restrict__ start, LocateHdr *__restrict__ hdr)
{
	constexpr u32 WAVES = LOCATE_THREADS / 64;
	__shared__ KT s_E[LOCATE_MAX_VALUES];
	__shared__ u32 s_w[WAVES];
	__shared__ u32 s_start[LOCATE_START_ENTRIES];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	u32 carry = 0;
	for (u64 base = 0; base < m && carry <= max_d; base += LOCATE_THREADS) {
		const u64 i = base + tid;
		KT k = 0;
		bool head = false;
		if (i < m) {
			k = kdf_apply(sv[i], ka);
			head = locate_is_head<KT>(i, k, i ? kdf_apply(sv[i - 1], ka) : k);
		}
		const u64 bal = __ballot(head);
		if (lane == 0)
			s_w[wave] = (u32)__popcll(bal);
		__syncthreads();
		u32 before = carry, total = 0;
#pragma unroll
		for (u32 w = 0; w < WAVES; ++w) {
			const u32 c = s_w[w];
			before += w < wave ? c : 0u;
			total += c;
		}
		const u32 d = before + (u32)__popcll(bal & (((u64)1 << lane) - 1u));
		if (head && d < max_d) {
			s_E[d] = k;
			E[d] = k;
			cum[d] = i;
		}
		carry += total;
		__syncthreads();
	}
	const u32 D = carry;
	if (D > max_d) {
		if (tid == 0)
			*hdr = LocateHdr{D, 0u, 0u, 0u};
		return;
	}
	__syncthreads();
	const u32 shift = locate_shift<KT>(s_E[0], s_E[D - 1u]);
	if (tid < LOCATE_START_ENTRIES) {
		const u32 s = locate_start_entry<KT>(s_E, D, shift, tid);
		s_start[tid] = s;
		start[tid] = s;
	}
	__syncthreads();
	if (tid == 0) {
		cum[D] = m;
		*hdr = LocateHdr{D, shift, locate_steps(locate_max_span(s_start)), 0u};
	}
}

// The search route's read of the keys.  Workgroup w owns the whole tiles [w * share_tiles, (w + 1) * share_tiles) of the keys
// behind the first 16-byte boundary (`head` keys in front of it); workgroup 0 also the keys in front of the boundary and behind
// the last whole tile, one by one.  LDS as rsx_locate_shape.hpp's locate_lds lays it out; lane l adds to set l % sets.
// rows[w][0 .. 2 (D + 1)): the workgroup's counts, 64 bits each -- stored once at the end, and added to before that whenever
// `flush_tiles` tiles have gone by (so that no 32-bit counter wraps).  bin[i] = cum[b] (BELOW: cum[b - eq]) where WANT_BIN.
template <typename KT, typename IT, bool WANT_BIN, bool BELOW>
__global__ __launch_bounds__(LOCATE_THREADS) void rsx_locate_search_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka,
                                                                           const KT *__restrict__ gE, const u64 *__restrict__ gcum,
                                                                           const u32 *__restrict__ gstart, u32 D, u32 shift, u32 steps,
                                                                           LocateLds lds, u64 share_tiles, u64 flush_tiles,
                                                                           u64 *__restrict__ rows, IT *__restrict__ bin)
{
	__shared__ __attribute__((aligned(16))) unsigned char s_mem[LOCATE_LDS_BYTES];
	KT *const s_E = (KT *)s_mem;
	IT *const s_cum = (IT *)(s_mem + lds.cum_off);
	u32 *const s_start = (u32 *)(s_mem + lds.start_off);
	u32 *const s_cnt = (u32 *)(s_mem + lds.cnt_off);
	const u32 tid = threadIdx.x, ncnt = locate_counters(D);
	for (u32 i = tid; i < D; i += LOCATE_THREADS)
		s_E[i] = gE[i];
	if (WANT_BIN)
		for (u32 i = tid; i <= D; i += LOCATE_THREADS)
			s_cum[i] = (IT)gcum[i];
	if (tid < LOCATE_START_ENTRIES)
		s_start[tid] = gstart[tid];
	for (u32 i = tid; i < lds.sets * ncnt; i += LOCATE_THREADS)
		s_cnt[i] = 0;
	__syncthreads();
	u32 *const my_cnt = s_cnt + ((tid & 63u) % lds.sets) * ncnt;
	auto locate = [&](const KT raw) -> IT {
		u32 eq;
		const u32 b = locate_search<KT, u32>(s_E, D, s_start, shift, steps, kdf_apply(raw, ka), &eq);
		atomicAdd(&my_cnt[locate_counter(b, eq)], 1u);
		return WANT_BIN ? s_cum[locate_bin_entry(b, eq, BELOW)] : (IT)0;
	};
	u64 *const row = rows + (u64)blockIdx.x * ncnt;
	bool flushed = false;
	auto flush = [&]() {
		__syncthreads();
		for (u32 i = tid; i < ncnt; i += LOCATE_THREADS) {
			u64 sum = flushed ? row[i] : 0;
			for (u32 r = 0; r < lds.sets; ++r) {
				sum += s_cnt[r * ncnt + i];
				s_cnt[r * ncnt + i] = 0;
			}
			row[i] = sum;
		}
		flushed = true;
		__syncthreads();
	};
	constexpr u32 V = 16 / sizeof(KT);                 // keys of one 16-byte load
	constexpr u32 NV = LOCATE_TILE / LOCATE_THREADS / V;   // loads per thread and tile
	constexpr u32 OV = V * sizeof(IT) >= 16 ? 16 / sizeof(IT) : V;
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	u64 head = ((16u - (u32)((uintptr_t)src & 15u)) & 15u) / sizeof(KT);
	if (head > n)
		head = n;
	const u64 body = n - head;
	const u64 tiles = body / LOCATE_TILE;
	const kvec_t *vsrc = (const kvec_t *)(src + head);
	const bool bin_ok = WANT_BIN && (((uintptr_t)(bin + head)) & (OV * sizeof(IT) - 1u)) == 0;
	const u64 t_lo = (u64)blockIdx.x * share_tiles, t_hi = t_lo + share_tiles < tiles ? t_lo + share_tiles : tiles;
	u64 since = 0;
	constexpr u32 U = 2;   // tiles whose loads are in flight together
	for (u64 t = t_lo; t < t_hi; t += U) {
		kvec_t x[U][NV];
#pragma unroll
		for (u32 u = 0; u < U; ++u)
			if (t + u < t_hi) {
#pragma unroll
				for (u32 v = 0; v < NV; ++v)
					x[u][v] = vsrc[(t + u) * (LOCATE_TILE / V) + v * LOCATE_THREADS + tid];
			}
#pragma unroll
		for (u32 u = 0; u < U; ++u)
			if (t + u < t_hi) {
#pragma unroll
				for (u32 v = 0; v < NV; ++v) {
					IT g[V];
#pragma unroll
					for (u32 e = 0; e < V; ++e)
						g[e] = locate(x[u][v][e]);
					if (WANT_BIN)
						rankdata_store<IT, V>(bin + head + ((t + u) * (LOCATE_TILE / V) + v * LOCATE_THREADS + tid) * V, g, bin_ok);
				}
			}
		since += U;
		if (since >= flush_tiles) {
			flush();
			since = 0;
		}
	}
	if (blockIdx.x == 0) {
		auto one = [&](u64 i) {
			const IT g = locate(src[i]);
			if (WANT_BIN)
				bin[i] = g;
		};
		if (tid < head)
			one(tid);
		for (u64 i = head + tiles * LOCATE_TILE + tid; i < n; i += LOCATE_THREADS)
			one(i);
	}
	flush();
}

// tot[c] = the sum of rows[0 .. nrows)[c]: 64 neighbouring columns per workgroup (a row's loads are one contiguous 512 bytes),
// sixteen threads per column that take every sixteenth row each
__global__ __launch_bounds__(1024) void rsx_locate_colsum_kernel(const u64 *__restrict__ rows, u32 nrows, u32 ncols, u64 *__restrict__ tot)
{
	__shared__ u64 s_part[16][64];
	const u32 tid = threadIdx.x, c = tid & 63u, q = tid >> 6;
	const u32 col = blockIdx.x * 64u + c;
	u64 sum = 0;
	if (col < ncols) {
#pragma unroll 4
		for (u32 r = q; r < nrows; r += 16u)
			sum += rows[(u64)r * ncols + col];
	}
	s_part[q][c] = sum;
	__syncthreads();
	if (q == 0 && col < ncols) {
#pragma unroll
		for (u32 p = 1; p < 16u; ++p)
			sum += s_part[p][c];
		tot[col] = sum;
	}
}

// less / equal of the caller's values from the summed counters `tot` (2 (D + 1) of them): every workgroup scans the D + 1 bin
// totals in LDS, then looks each of its values up among the edges (it IS one of them) -- locate_less, locate_equal.
template <typename KT, typename IT>
__global__ __launch_bounds__(1024) void rsx_locate_finish_kernel(const KT *__restrict__ vals, u64 m, KdfArgs<KT> ka, const KT *__restrict__ E, u32 D,
                                                                 const u64 *__restrict__ tot, IT *__restrict__ less, IT *__restrict__ equal)
{
	constexpr u32 CH = (LOCATE_MAX_VALUES + 1 + 1023) / 1024;   // bins per thread
	__shared__ u64 s_incl[CH * 1024];
	__shared__ u64 s_part[1024];
	const u32 tid = threadIdx.x, bins = D + 1u;
	u64 sum = 0;
#pragma unroll
	for (u32 j = 0; j < CH; ++j) {
		const u32 b = tid * CH + j;
		sum += b < bins ? locate_total(tot, b) : 0;
		s_incl[b] = sum;
	}
	s_part[tid] = sum;
	__syncthreads();
	for (u32 off = 1; off < 1024; off <<= 1) {
		const u64 add = tid >= off ? s_part[tid - off] : 0;
		__syncthreads();
		s_part[tid] += add;
		__syncthreads();
	}
	const u64 before = s_part[tid] - sum;
#pragma unroll
	for (u32 j = 0; j < CH; ++j)
		s_incl[tid * CH + j] += before;
	__syncthreads();
	const u64 stride = (u64)gridDim.x * 1024u;
	for (u64 j = (u64)blockIdx.x * 1024u + tid; j < m; j += stride) {
		const KT k = kdf_apply(vals[j], ka);
		u32 lo = 0, hi = D;
		while (lo < hi) {
			const u32 mid = (lo + hi) / 2u;
			if (E[mid] < k)
				lo = mid + 1u;
			else
				hi = mid;
		}
		if (less)
			less[j] = (IT)locate_less(s_incl, lo);
		if (equal)
			equal[j] = (IT)locate_equal(tot, lo);
	}
}

// counts[256] -> offs[0 .. 256] exclusive, offs[256] = offs[257] = total (258 entries: the lookup kernel reads one entry behind the one
// it is given, and is given offs + 1 for the bins of the keys AT or below)
__global__ __launch_bounds__(256) void rsx_locate_scan256_kernel(const u64 *__restrict__ counts, u64 *__restrict__ offs, u64 total)
{
	__shared__ u64 s[256];
	const u32 tid = threadIdx.x;
	const u64 own = counts[tid];
	s[tid] = own;
	__syncthreads();
	for (u32 off = 1; off < 256; off <<= 1) {
		const u64 add = tid >= off ? s[tid - off] : 0;
		__syncthreads();
		s[tid] += add;
		__syncthreads();
	}
	offs[tid] = s[tid] - own;
	if (tid < 2u)
		offs[256u + tid] = total;
}

// *flag = 1 where a derived key is above its successor's (a plain store: every writer stores the same word)
template <typename KT>
__global__ __launch_bounds__(256) void rsx_locate_descents_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, u32 *__restrict__ flag)
{
	const u64 stride = (u64)gridDim.x * 256u;
	bool any = false;
	for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i + 1 < n; i += stride)
		any |= kdf_apply(src[i], ka) > kdf_apply(src[i + 1], ka);
	if (any)
		*flag = 1u;
}

// the number of the sorted raw keys a[lo .. hi) whose derived key is below k (OR_EQUAL: at or below)
template <typename KT, bool OR_EQUAL>
__device__ __forceinline__ u64 locate_count_sorted(const KT *__restrict__ a, u64 lo, u64 hi, KT k, KdfArgs<KT> ka)
{
	while (lo < hi) {
		const u64 mid = lo + (hi - lo) / 2u;
		const KT x = kdf_apply(a[mid], ka);
		if (OR_EQUAL ? x <= k : x < k)
			lo = mid + 1u;
		else
			hi = mid;
	}
	return lo;
}

// sk[0 .. n): the keys in sorted order.  less[j] = keys below vals[j], equal[j] = keys equal to it; each may be nullptr.
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_locate_sorted_values_kernel(const KT *__restrict__ sk, u64 n, const KT *__restrict__ vals, u64 m,
                                                                       KdfArgs<KT> ka, IT *__restrict__ less, IT *__restrict__ equal)
{
	const u64 stride = (u64)gridDim.x * 256u;
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < m; j += stride) {
		const KT k = kdf_apply(vals[j], ka);
		const u64 lo = locate_count_sorted<KT, false>(sk, 0, n, k, ka);
		if (less)
			less[j] = (IT)lo;
		if (equal)
			equal[j] = (IT)(locate_count_sorted<KT, true>(sk, lo, n, k, ka) - lo);
	}
}

// sv[0 .. m): the values in sorted order, m >= 1.  bin[i] = values at or below src[i] (BELOW: strictly below).  The values are
// cut into at most 4096 blocks of `block` values; the derived key of each block's last value is held in LDS: twelve levels of
// the search run there, the rest over the one block in device memory.
template <typename KT, typename IT, bool BELOW>
__global__ __launch_bounds__(1024) void rsx_locate_sorted_bins_kernel(const KT *__restrict__ src, u64 n, const KT *__restrict__ sv, u64 m,
                                                                      u64 block, KdfArgs<KT> ka, IT *__restrict__ bin)
{
	__shared__ KT s_last[4096];
	const u32 tid = threadIdx.x;
	const u32 blocks = (u32)((m + block - 1) / block);
	for (u32 i = tid; i < blocks; i += 1024u) {
		const u64 end = (u64)(i + 1u) * block < m ? (u64)(i + 1u) * block : m;
		s_last[i] = kdf_apply(sv[end - 1u], ka);
	}
	__syncthreads();
	const u64 stride = (u64)gridDim.x * 1024u;
	for (u64 i = (u64)blockIdx.x * 1024u + tid; i < n; i += stride) {
		const KT k = kdf_apply(src[i], ka);
		u32 lo = 0, hi = blocks;   // blocks that lie wholly on the counted side
		while (lo < hi) {
			const u32 mid = (lo + hi) / 2u;
			if (BELOW ? s_last[mid] < k : s_last[mid] <= k)
				lo = mid + 1u;
			else
				hi = mid;
		}
		u64 count = lo < blocks ? (u64)lo * block : m;   // (the last block may be short)
		if (lo < blocks) {
			const u64 end = count + block < m ? count + block : m;
			count = locate_count_sorted<KT, !BELOW>(sv, count, end, k, ka);
		}
		bin[i] = (IT)count;
	}
}

}  // namespace rsx
