// rsx_nth.hpp -- the kernels of rsx_sort_nth_device: the elements at a handful of given ranks of the stable sorted order,
// without sorting the rest.  What rsx_topk.hpp does for ONE rank, carried through the same digit histograms for up to
// NTH_MAX_RANKS ranks at once: nine deciles cost the same reads of the input as one median.
//
// MSD digits of the derived keys, 8 bits at a time, most significant byte first; constant byte columns are NOT skipped.  The
// state between kernels is an NthCtl in device memory: one record per distinct rank (prefix found so far, rank still wanted
// inside its bucket, elements below its bucket) and the sorted list of ACTIVE BUCKETS -- the distinct prefixes of the
// records, at most 64, all of the same depth.  The host enqueues every kernel of both courses and each one looks at
// NthCtl::mode to see whether it has work; the host reads the control block back once, behind the last of them.
//
//   rsx_nth_hist_kernel     a level's histogram: for every element whose masked derived key is an active prefix, its next
//                           digit counted in that bucket's 256 LDS counters (level 0: one bucket, no test; later levels: a
//                           256-bit mask of the active TOP digits rejects most elements before the search among prefixes),
//                           folded into the global table with one atomic per non-zero (bucket, digit) and workgroup
//   rsx_nth_pick_kernel     one workgroup: for every record the digit of its bucket that holds its rank; the active list,
//                           the buckets' sizes and bases rebuilt; buckets that together fit the candidate buffer switch to
//                           the candidate course (mode 1); every digit known without that: mode 2, the prefixes ARE the keys
//   rsx_nth_count_kernel, rsx_nth_write_kernel   (mode 1) the elements of the active buckets moved into the candidate buffer
//                           IN INDEX ORDER as (key bit pattern, index): a count per range, a write over the same ranges at
//                           the offsets the counts give -- no look-back chain, no atomics that would lose index order, which
//                           is what lets the stable sort of the candidates give the exact tie order
//   rsx_nth_gather_kernel   m threads: the sorted candidates read at base(bucket) + rank in bucket, n_less / n_equal by two
//                           binary searches inside the bucket, outputs written in the caller's order of ranks
//   rsx_nth_sorted_kernel   the sort route: the same answers read through the ranks of a whole rank sort
#pragma once

#include "rsx_topk.hpp"

namespace rsx {

// NTH_ITER sweeps of NTH_THREADS threads x one 16-byte vector make a tile; a workgroup's range is a whole number of tiles
enum : u32 { NTH_THREADS = 512, NTH_ITER = 4, NTH_MAX_GROUPS = 1024, NTH_MAX_RANKS = 64 };
template <typename KT> constexpr u32 nth_tile() { return NTH_ITER * NTH_THREADS * (16u / (u32)sizeof(KT)); }

struct NthRec {
	u64 prefix;   // the derived-key bits found so far
	u64 k_rem;    // the rank wanted inside its bucket (0-based)
	u64 below;    // elements whose derived key lies below the bucket
	u32 bucket;   // the bucket's place in the active list
	u32 pad;
};

// mode: 0 = the next digit is looked for in the input, 1 = the active buckets go to the candidate buffer, 2 = every digit is
// known and the buckets did not go there (the answer is read off the records)
struct NthCtl {
	u32 mode;
	u32 nrec;          // distinct ranks
	u32 nact;          // active buckets
	u32 input_reads;
	u32 digit_passes;
	u32 pad[3];
	u64 mask;          // which bits of the derived keys the prefixes hold
	u64 cand_n;        // (mode 1) elements of all active buckets
	u64 topmask[4];    // one bit per top digit that some active prefix has
	u64 act_prefix[NTH_MAX_RANKS];   // ascending
	u64 act_size[NTH_MAX_RANKS];
	u64 act_base[NTH_MAX_RANKS];     // exclusive sum of the sizes: where the bucket starts among the sorted candidates
	NthRec rec[NTH_MAX_RANKS];       // ascending by rank, hence by prefix
};

__device__ __forceinline__ bool nth_top_active(u32 top, u64 m0, u64 m1, u64 m2, u64 m3)
{
	const u64 w = top < 128u ? (top < 64u ? m0 : m1) : (top < 192u ? m2 : m3);
	return (w >> (top & 63u)) & 1ull;
}

// the place of km among the ascending active prefixes, or -1
template <typename KT> __device__ __forceinline__ int nth_find(KT km, const KT *s_act, u32 nact)
{
	u32 lo = 0, hi = nact;
	while (lo < hi) {
		const u32 mid = (lo + hi) >> 1;
		if (s_act[mid] < km)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < nact && s_act[lo] == km ? (int)lo : -1;
}

// Workgroup g counts the digit `shift` of the elements [g * chunk, (g + 1) * chunk) per active bucket.
template <typename KT, int LEVEL0>
__global__ __launch_bounds__(NTH_THREADS) void rsx_nth_hist_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, const NthCtl *ctl,
                                                                    u64 *__restrict__ table, u64 chunk, u32 shift)
{
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 TOP = 8 * ((u32)sizeof(KT) - 1);
	if (ctl->mode != 0)
		return;
	__shared__ u32 h[LEVEL0 ? 256 : NTH_MAX_RANKS * 256];
	__shared__ KT s_act[NTH_MAX_RANKS];
	const u32 tid = threadIdx.x;
	const u32 nact = LEVEL0 ? 1u : min(ctl->nact, (u32)NTH_MAX_RANKS);
	for (u32 i = tid; i < nact * 256u; i += NTH_THREADS)
		h[i] = 0;
	if (!LEVEL0 && tid < nact)
		s_act[tid] = (KT)ctl->act_prefix[tid];
	__syncthreads();
	const KT mask = (KT)ctl->mask;
	const u64 m0 = ctl->topmask[0], m1 = ctl->topmask[1], m2 = ctl->topmask[2], m3 = ctl->topmask[3];
	const bool aligned = ((uintptr_t)src & 15u) == 0;
	const u64 lo = (u64)blockIdx.x * chunk;
	const u64 hi = lo + chunk < n ? lo + chunk : n;
	for (u64 i0 = lo + (u64)tid * V; i0 < hi; i0 += (u64)NTH_THREADS * V) {
		KT x[V];
		topk_load<KT, V>(src, i0, hi, aligned, x);
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			if (i0 + e < hi) {
				const KT kd = kdf_apply(x[e], ka);
				const u32 d = (u32)((u64)kd >> shift) & 255u;
				if (LEVEL0) {
					atomicAdd(&h[d], 1u);
				} else if (nth_top_active((u32)((u64)kd >> TOP) & 255u, m0, m1, m2, m3)) {
					const int b = nth_find<KT>((KT)(kd & mask), s_act, nact);
					if (b >= 0)
						atomicAdd(&h[(u32)b * 256u + d], 1u);
				}
			}
		}
	}
	__syncthreads();
	for (u32 i = tid; i < nact * 256u; i += NTH_THREADS) {
		const u32 c = h[i];
		if (c)
			atomicAdd(&table[i], (u64)c);
	}
}

// For every record the digit of its bucket that holds its rank, from the table the histogram left (whose rows are zeroed for
// the next one); then the active list rebuilt.  Buckets that together hold at most `cap` elements go to the candidate buffer;
// after the last digit (shift == 0) they only do if indices are wanted -- the prefixes are the keys.
template <typename KT>
__global__ __launch_bounds__(256) void rsx_nth_pick_kernel(NthCtl *ctl, u64 *__restrict__ table, u32 shift, u64 cap, u32 want_idx)
{
	constexpr u32 TOP = 8 * ((u32)sizeof(KT) - 1);
	if (ctl->mode != 0)
		return;
	__shared__ u64 s_prefix[NTH_MAX_RANKS], s_krem[NTH_MAX_RANKS], s_below[NTH_MAX_RANKS], s_size[NTH_MAX_RANKS];
	__shared__ u64 s_bp[NTH_MAX_RANKS], s_bs[NTH_MAX_RANKS], s_top[4];
	__shared__ u32 s_first[NTH_MAX_RANKS + 1];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 nrec = min(ctl->nrec, (u32)NTH_MAX_RANKS), nact = min(ctl->nact, (u32)NTH_MAX_RANKS);
	if (tid < 4u)
		s_top[tid] = 0;
	if (tid < nrec) {
		const u32 b = ctl->rec[tid].bucket;
		if (tid == 0 || ctl->rec[tid - 1].bucket != b)
			s_first[b & 63u] = tid;
		s_prefix[tid] = ctl->rec[tid].prefix;
		s_below[tid] = ctl->rec[tid].below;
		s_krem[tid] = 0;
		s_size[tid] = 0;
	}
	if (tid == 0)
		s_first[nact] = nrec;
	__syncthreads();
	// a wave per bucket, four digits per lane
	for (u32 b = wave; b < nact; b += 4u) {
		u64 *row = table + (size_t)b * 256u + 4u * lane;
		u64 c[4], sum = 0;
#pragma unroll
		for (u32 e = 0; e < 4u; ++e) {
			c[e] = row[e];
			row[e] = 0;
			sum += c[e];
		}
		const u64 incl = topk_wave_incl_sum<u64>(sum, lane);
		const u64 excl = incl - sum;
		const u32 r1 = min(s_first[b + 1], nrec);
		for (u32 r = s_first[b]; r < r1; ++r) {
			const u64 k = ctl->rec[r].k_rem;
			if (excl <= k && k < incl) {
				u64 e0 = excl;
				bool done = false;
#pragma unroll
				for (u32 e = 0; e < 4u; ++e) {
					if (!done && k < e0 + c[e]) {
						s_prefix[r] = ctl->rec[r].prefix | ((u64)(4u * lane + e) << shift);
						s_krem[r] = k - e0;
						s_below[r] = ctl->rec[r].below + e0;
						s_size[r] = c[e];
						done = true;
					}
					e0 += c[e];
				}
			}
		}
	}
	__syncthreads();
	// the distinct prefixes of the records (ascending with the ranks) are the next level's buckets
	u64 p = 0;
	u32 b = 0, nact2 = 0;
	if (wave == 0) {
		const bool on = lane < nrec;
		p = on ? s_prefix[lane] : 0;
		const bool first = on && (lane == 0 || p != s_prefix[lane - 1]);
		const u64 m = __ballot(first);
		b = on ? (u32)__popcll(m & ((2ull << lane) - 1ull)) - 1u : 0u;
		nact2 = (u32)__popcll(m);
		if (first) {
			s_bp[b] = p;
			s_bs[b] = s_size[lane];
			const u32 top = (u32)(p >> TOP) & 255u;
			atomicOr(&s_top[top >> 6], 1ull << (top & 63u));
		}
	}
	__syncthreads();
	if (wave == 0) {
		const u64 sz = lane < nact2 ? s_bs[lane] : 0;
		const u64 incl = topk_wave_incl_sum<u64>(sz, lane);
		const u64 total = __shfl(incl, 63);
		if (lane < nact2) {
			ctl->act_prefix[lane] = s_bp[lane];
			ctl->act_size[lane] = sz;
			ctl->act_base[lane] = incl - sz;
		}
		if (lane < nrec) {
			ctl->rec[lane].prefix = p;
			ctl->rec[lane].k_rem = s_krem[lane];
			ctl->rec[lane].below = s_below[lane];
			ctl->rec[lane].bucket = b;
		}
		if (lane < 4u)
			ctl->topmask[lane] = s_top[lane];
		if (lane == 0) {
			ctl->nact = nact2;
			ctl->mask |= 0xFFull << shift;
			ctl->digit_passes += 1;
			ctl->input_reads += 1;
			u32 mode = 0;
			if (shift == 0)
				mode = want_idx && total <= cap ? 1u : 2u;
			else if (total <= cap)
				mode = 1u;
			if (mode == 1u)
				ctl->cand_n = total;
			ctl->mode = mode;
		}
	}
}

// (mode 1) goff[g] = elements of range g that lie in an active bucket
template <typename KT>
__global__ __launch_bounds__(NTH_THREADS) void rsx_nth_count_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, NthCtl *ctl,
                                                                     u64 *__restrict__ goff, u64 chunk)
{
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 TOP = 8 * ((u32)sizeof(KT) - 1);
	if (ctl->mode != 1)
		return;
	__shared__ KT s_act[NTH_MAX_RANKS];
	__shared__ u32 s_cnt;
	const u32 tid = threadIdx.x;
	const u32 nact = min(ctl->nact, (u32)NTH_MAX_RANKS);
	if (tid < nact)
		s_act[tid] = (KT)ctl->act_prefix[tid];
	if (tid == 0)
		s_cnt = 0;
	__syncthreads();
	const KT mask = (KT)ctl->mask;
	const u64 m0 = ctl->topmask[0], m1 = ctl->topmask[1], m2 = ctl->topmask[2], m3 = ctl->topmask[3];
	const bool aligned = ((uintptr_t)src & 15u) == 0;
	const u64 lo = (u64)blockIdx.x * chunk;
	const u64 hi = lo + chunk < n ? lo + chunk : n;
	u32 cnt = 0;
	for (u64 i0 = lo + (u64)tid * V; i0 < hi; i0 += (u64)NTH_THREADS * V) {
		KT x[V];
		topk_load<KT, V>(src, i0, hi, aligned, x);
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			if (i0 + e < hi) {
				const KT kd = kdf_apply(x[e], ka);
				if (nth_top_active((u32)((u64)kd >> TOP) & 255u, m0, m1, m2, m3))
					cnt += nth_find<KT>((KT)(kd & mask), s_act, nact) >= 0 ? 1u : 0u;
			}
		}
	}
	cnt = topk_wave_sum<u32>(cnt);
	if ((tid & 63u) == 0 && cnt)
		atomicAdd(&s_cnt, cnt);
	__syncthreads();
	if (tid == 0) {
		goff[blockIdx.x] = s_cnt;
		if (blockIdx.x == 0)
			ctl->input_reads += 1;
	}
}

// (mode 1) range g's elements of the active buckets written in index order behind those of the ranges before it; keys travel as
// the caller's bit patterns, ci may be NULL (no indices wanted)
template <typename KT, typename IT>
__global__ __launch_bounds__(NTH_THREADS) void rsx_nth_write_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, NthCtl *ctl,
                                                                     const u64 *__restrict__ goff, u64 chunk, KT *__restrict__ ck,
                                                                     IT *__restrict__ ci, u64 cap)
{
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 TOP = 8 * ((u32)sizeof(KT) - 1);
	constexpr u32 WAVES = NTH_THREADS / 64;
	if (ctl->mode != 1)
		return;
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 g = blockIdx.x;
	if (g == 0 && tid == 0)
		ctl->input_reads += 1;
	if (!goff[g])
		return;
	__shared__ KT s_act[NTH_MAX_RANKS];
	__shared__ u64 s_a[WAVES];
	__shared__ u32 s_w[WAVES];
	const u32 nact = min(ctl->nact, (u32)NTH_MAX_RANKS);
	if (tid < nact)
		s_act[tid] = (KT)ctl->act_prefix[tid];
	u64 a = 0;
	for (u32 q = tid; q < g; q += NTH_THREADS)
		a += goff[q];
	a = topk_wave_sum<u64>(a);
	if (lane == 0)
		s_a[wave] = a;
	__syncthreads();
	u64 at = 0;
#pragma unroll
	for (u32 w = 0; w < WAVES; ++w)
		at += s_a[w];
	const KT mask = (KT)ctl->mask;
	const u64 m0 = ctl->topmask[0], m1 = ctl->topmask[1], m2 = ctl->topmask[2], m3 = ctl->topmask[3];
	const bool aligned = ((uintptr_t)src & 15u) == 0;
	const u64 lo = (u64)g * chunk;
	const u64 hi = lo + chunk < n ? lo + chunk : n;
	for (u64 t0 = lo; t0 < hi; t0 += (u64)NTH_THREADS * V) {
		const u64 i0 = t0 + (u64)tid * V;
		KT x[V];
		u32 fi = 0;
		if (i0 < hi) {
			topk_load<KT, V>(src, i0, hi, aligned, x);
#pragma unroll
			for (u32 e = 0; e < V; ++e) {
				const KT kd = kdf_apply(x[e], ka);
				const bool in = i0 + e < hi && nth_top_active((u32)((u64)kd >> TOP) & 255u, m0, m1, m2, m3) &&
				                nth_find<KT>((KT)(kd & mask), s_act, nact) >= 0;
				fi |= (in ? 1u : 0u) << e;
			}
		} else {
#pragma unroll
			for (u32 e = 0; e < V; ++e)
				x[e] = 0;
		}
		const u32 cnt = (u32)__popc(fi);
		const u32 incl = topk_wave_incl_sum<u32>(cnt, lane);
		if (lane == 63u)
			s_w[wave] = incl;
		__syncthreads();
		u32 before = incl - cnt, total = 0;
#pragma unroll
		for (u32 w = 0; w < WAVES; ++w) {
			const u32 s = s_w[w];
			before += w < wave ? s : 0u;
			total += s;
		}
		u64 o = at + before;
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			if ((fi >> e) & 1u) {
				const u64 pos = o++;
				if (pos < cap) {
					ck[pos] = x[e];
					if (ci)
						ci[pos] = (IT)(i0 + e);
				}
			}
		}
		at += total;
		__syncthreads();
	}
}

// The answers in the caller's order: position j asks for record map[j].  Mode 1: sk / si are the candidates sorted stably by
// their derived keys, bucket after bucket in prefix order.  Mode 2: the record's prefix is the key (no index to give).
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_nth_gather_kernel(const NthCtl *ctl, const KT *__restrict__ sk, const IT *__restrict__ si,
                                                              const u32 *__restrict__ map, u64 m, KT *__restrict__ out_keys,
                                                              IT *__restrict__ out_idx, u64 *__restrict__ nless, u64 *__restrict__ nequal,
                                                              KdfArgs<KT> ka)
{
	const u32 mode = ctl->mode;
	const u64 cand_n = ctl->cand_n;
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < m; j += (u64)gridDim.x * 256u) {
		const NthRec r = ctl->rec[map[j] & (NTH_MAX_RANKS - 1u)];
		const u32 b = r.bucket & (NTH_MAX_RANKS - 1u);
		const u64 size = ctl->act_size[b];
		u64 less = r.below, eq = size;
		if (mode == 2u) {
			if (out_keys)
				out_keys[j] = kdf_invert<KT>((KT)r.prefix, ka);
		} else {
			const u64 base = ctl->act_base[b];
			const u64 end = base + size < cand_n ? base + size : cand_n;
			const u64 pos = base + r.k_rem;
			if (pos >= end)
				continue;   // (a rank outside its bucket: cannot happen)
			const KT x = sk[pos];
			const KT kd = kdf_apply(x, ka);
			u64 lo = base, hi = pos;   // the first place of the bucket whose key is not below kd
			while (lo < hi) {
				const u64 mid = lo + ((hi - lo) >> 1);
				if (kdf_apply(sk[mid], ka) < kd)
					lo = mid + 1;
				else
					hi = mid;
			}
			const u64 lb = lo;
			lo = pos + 1, hi = end;    // the first place behind pos whose key is above kd
			while (lo < hi) {
				const u64 mid = lo + ((hi - lo) >> 1);
				if (kdf_apply(sk[mid], ka) <= kd)
					lo = mid + 1;
				else
					hi = mid;
			}
			less = r.below + (lb - base);
			eq = lo - lb;
			if (out_keys)
				out_keys[j] = x;
			if (out_idx)
				out_idx[j] = si[pos];
		}
		nless[j] = less;
		nequal[j] = eq;
	}
}

// The sort route: R is the stable argsort of src; position j asks for rank want[j].  n_less / n_equal by binary search THROUGH
// the ranks (src[R[mid]]): m x log n gathers, not a pass over the input per rank.
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_nth_sorted_kernel(const KT *__restrict__ src, const IT *__restrict__ R, u64 n,
                                                              const u64 *__restrict__ want, u64 m, KT *__restrict__ out_keys,
                                                              IT *__restrict__ out_idx, u64 *__restrict__ nless, u64 *__restrict__ nequal,
                                                              KdfArgs<KT> ka)
{
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < m; j += (u64)gridDim.x * 256u) {
		const u64 r = want[j];
		if (r >= n)
			continue;   // (checked by the host)
		const IT i = R[r];
		const KT x = src[i];
		const KT kd = kdf_apply(x, ka);
		u64 lo = 0, hi = r;
		while (lo < hi) {
			const u64 mid = lo + ((hi - lo) >> 1);
			if (kdf_apply(src[R[mid]], ka) < kd)
				lo = mid + 1;
			else
				hi = mid;
		}
		const u64 lb = lo;
		lo = r + 1, hi = n;
		while (lo < hi) {
			const u64 mid = lo + ((hi - lo) >> 1);
			if (kdf_apply(src[R[mid]], ka) <= kd)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (out_keys)
			out_keys[j] = x;
		if (out_idx)
			out_idx[j] = i;
		nless[j] = lb;
		nequal[j] = lo - lb;
	}
}

// n == 1: every rank is 0
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_nth_single_kernel(const KT *__restrict__ src, u64 m, KT *__restrict__ out_keys, IT *__restrict__ out_idx)
{
	const KT x = src[0];
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < m; j += (u64)gridDim.x * 256u) {
		if (out_keys)
			out_keys[j] = x;
		if (out_idx)
			out_idx[j] = (IT)0;
	}
}

}  // namespace rsx
