// rsx_topk.hpp -- the kernels of rsx_sort_topk_device: the first k entries of the stable sorted order without sorting the
// rest (the reference README's "Hybrids" note, README.md:647-650 -- "one MSB pass and then LSB sort the sub-results" -- with
// the sub-results that cannot hold the answer never sorted).
//
// MSD radix select on derived keys, 8 bits at a time, most significant byte first; constant byte columns are NOT skipped
// (a digit every key shares costs the same read as any other).  The state between kernels is a TopkCtl in device memory:
// the host enqueues every kernel of both possible courses and each one looks at TopkCtl::mode to see whether it has work.
//
//   rsx_topk_hist_kernel    digit histogram of the elements that match the prefix found so far, per workgroup in LDS,
//                           folded into TopkCtl::table; every workgroup owns one contiguous range of the elements and
//                           also leaves its own 256 counts (and how many of its elements lie below the prefix) in a row
//   rsx_topk_pick_kernel    one workgroup walks the table: the digit that holds rank k, the elements below it
//   rsx_topk_rows_kernel    per workgroup range: elements before the selected bucket, elements in it (from the rows: the
//                           input is not read for this)
//   rsx_topk_write_kernel   the ranges written out IN INDEX ORDER at the offsets the rows give: elements before the bucket
//                           into the pair buffer; the bucket's elements into the candidate buffer (second pass over the
//                           input) or, when every digit is known, the first k - n_less of them behind the others
//   rsx_topk_gather_kernel, rsx_topk_count_kernel   the sort route: keys gathered through the first k ranks; n_less / n_equal
//
// Index order is what makes the tie rule cheap: among the elements equal to the k-th key the first k - n_less in index
// order are the ones a stable sort puts first.
#pragma once

#include "rsx_kernels.hpp"

namespace rsx {

// TOPK_ITER sweeps of TOPK_THREADS threads x one 16-byte vector make a tile; a workgroup's range is a whole number of tiles
enum : u32 { TOPK_THREADS = 512, TOPK_ITER = 4, TOPK_MAX_GROUPS = 1024, TOPK_ROW = 264 };
template <typename KT> constexpr u32 topk_tile() { return TOPK_ITER * TOPK_THREADS * (16u / (u32)sizeof(KT)); }

// mode: 0 = the next digit is looked for in the input, 1 = in the candidate buffer
struct TopkCtl {
	u64 k_rem;      // the rank wanted inside the selected bucket (1-based)
	u64 n_less;     // elements before the selected bucket
	u64 prefix;     // the derived-key bits found so far ...
	u64 mask;       // ... and which bits those are
	u64 bucket;     // elements in the selected bucket
	u64 cand_n;     // live candidates (mode 1)
	u64 pairs_n;    // pairs the second pass over the input wrote (mode 1)
	u64 kth_raw;    // the k-th key's bit pattern, once the last digit is known
	u32 mode;
	u32 input_reads;
	u32 digit_passes;
	u32 pad;
	u64 table[256];
};

template <typename T> __device__ __forceinline__ T topk_wave_incl_sum(T v, u32 lane)
{
#pragma unroll
	for (u32 off = 1; off < 64; off <<= 1) {
		const T o = __shfl_up(v, off);
		if (lane >= off)
			v += o;
	}
	return v;
}

template <typename T> __device__ __forceinline__ T topk_wave_sum(T v)
{
#pragma unroll
	for (u32 off = 32; off; off >>= 1)
		v += __shfl_xor(v, off);
	return v;
}

// V elements from i0 on, those at or behind `hi` as zero (the caller looks at valid ones only)
template <typename KT, u32 V>
__device__ __forceinline__ void topk_load(const KT *__restrict__ src, u64 i0, u64 hi, bool aligned, KT (&x)[V])
{
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	if (aligned && i0 + V <= hi) {
		const kvec_t xv = *(const kvec_t *)(src + i0);
#pragma unroll
		for (u32 e = 0; e < V; ++e)
			x[e] = xv[e];
	} else {
#pragma unroll
		for (u32 e = 0; e < V; ++e)
			x[e] = i0 + e < hi ? src[i0 + e] : (KT)0;
	}
}

// Workgroup g counts the digit `shift` of the elements [g * chunk, (g + 1) * chunk) whose derived key matches the prefix.
// FROM_CAND: the elements are the candidate buffer's, their number is TopkCtl::cand_n (the grid is sized for the capacity).
template <typename KT, int FROM_CAND>
__global__ __launch_bounds__(TOPK_THREADS) void rsx_topk_hist_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, TopkCtl *ctl,
                                                                      u32 *__restrict__ rows, u64 chunk, u32 shift)
{
	constexpr u32 V = 16 / sizeof(KT);
	if (ctl->mode != (u32)FROM_CAND)
		return;
	if (FROM_CAND)
		n = ctl->cand_n;
	__shared__ u32 h[256];
	__shared__ u32 s_below;
	const u32 tid = threadIdx.x;
	if (tid < 256u)
		h[tid] = 0;
	if (tid == 0)
		s_below = 0;
	__syncthreads();
	const KT prefix = (KT)ctl->prefix, mask = (KT)ctl->mask;
	const bool aligned = ((uintptr_t)src & 15u) == 0;
	const u64 lo = (u64)blockIdx.x * chunk;
	const u64 hi = lo + chunk < n ? lo + chunk : n;
	u32 below = 0;
	for (u64 i0 = lo + (u64)tid * V; i0 < hi; i0 += (u64)TOPK_THREADS * V) {
		KT x[V];
		topk_load<KT, V>(src, i0, hi, aligned, x);
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			if (i0 + e < hi) {
				const KT kd = kdf_apply(x[e], ka);
				const KT km = (KT)(kd & mask);
				if (km == prefix)
					atomicAdd(&h[(u32)((u64)kd >> shift) & 255u], 1u);
				else
					below += km < prefix ? 1u : 0u;
			}
		}
	}
	below = topk_wave_sum<u32>(below);
	if ((tid & 63u) == 0 && below)
		atomicAdd(&s_below, below);
	__syncthreads();
	u32 *row = rows + (size_t)blockIdx.x * TOPK_ROW;
	if (tid < 256u) {
		const u32 c = h[tid];
		row[tid] = c;
		if (c)
			atomicAdd(&ctl->table[tid], (u64)c);
	}
	if (tid == 0)
		row[256] = s_below;
}

// The digit that holds rank k_rem of the bucket, from the table the histogram left (which is zeroed for the next one).
// allow_fill: a bucket of at most `cap` elements switches to the candidate buffer (mode 1).
template <typename KT>
__global__ __launch_bounds__(256) void rsx_topk_pick_kernel(TopkCtl *ctl, u32 shift, u64 cap, u32 allow_fill, KdfArgs<KT> ka)
{
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u64 c = ctl->table[tid];
	ctl->table[tid] = 0;
	const u64 k_rem = ctl->k_rem;
	u64 incl = topk_wave_incl_sum<u64>(c, lane);
	__shared__ u64 s_w[4];
	if (lane == 63u)
		s_w[wave] = incl;
	__syncthreads();
	for (u32 w = 0; w < wave; ++w)
		incl += s_w[w];
	const u64 excl = incl - c;
	if (excl < k_rem && k_rem <= incl) {
		const u64 n_less = ctl->n_less + excl;
		const u64 prefix = ctl->prefix | ((u64)tid << shift);
		ctl->n_less = n_less;
		ctl->k_rem = k_rem - excl;
		ctl->prefix = prefix;
		ctl->mask |= 0xFFull << shift;
		ctl->bucket = c;
		ctl->digit_passes += 1;
		if (ctl->mode == 0)
			ctl->input_reads += 1;
		if (allow_fill && c <= cap) {
			ctl->mode = 1;
			ctl->cand_n = c;
			ctl->pairs_n = n_less;
		}
		if (shift == 0)
			ctl->kth_raw = (u64)kdf_invert<KT>((KT)prefix, ka);
	}
}

// goff[g] = {elements of range g before the selected bucket, elements of range g in it}: one wave per row
__global__ __launch_bounds__(1024) void rsx_topk_rows_kernel(const TopkCtl *ctl, const u32 *__restrict__ rows, u32 groups, u32 shift,
                                                             u32 want_mode, u64 *__restrict__ goff)
{
	if (ctl->mode != want_mode)
		return;
	const u32 lane = threadIdx.x & 63u;
	const u32 g = blockIdx.x * 16u + (threadIdx.x >> 6);
	if (g >= groups)
		return;
	const u32 digit = (u32)(ctl->prefix >> shift) & 255u;
	const u32 *row = rows + (size_t)g * TOPK_ROW;
	const u32x4 v = *(const u32x4 *)(row + 4u * lane);
	u32 less = lane == 0 ? row[256] : 0u, in = 0;
#pragma unroll
	for (u32 e = 0; e < 4u; ++e) {
		const u32 d = 4u * lane + e;
		less += d < digit ? v[e] : 0u;
		in += d == digit ? v[e] : 0u;
	}
	less = topk_wave_sum<u32>(less);
	in = topk_wave_sum<u32>(in);
	if (lane == 0) {
		goff[2 * (size_t)g] = less;
		goff[2 * (size_t)g + 1] = in;
	}
}

// Range g written out in index order.  An element is "before" if its masked derived key is below the prefix, "in" if it
// equals the prefix.
//   FINAL = 0 (the second pass over the input; runs in mode 1): before -> pairs[...], in -> the candidate buffer;
//   FINAL = 1 (every digit known; runs in mode FROM_CAND): before -> pairs[base + ...], in -> pairs[n_less + j] for the
//     first k_rem of them.
// Keys travel as the caller's bit patterns; the index of an input element is its position, a candidate's is sidx[i].
template <typename KT, typename IT, int FROM_CAND, int FINAL>
__global__ __launch_bounds__(TOPK_THREADS) void rsx_topk_write_kernel(const KT *__restrict__ src, const IT *__restrict__ sidx, u64 n,
                                                                       KdfArgs<KT> ka, TopkCtl *ctl, const u64 *__restrict__ goff,
                                                                       u64 chunk, KT *__restrict__ pk, IT *__restrict__ pi, u64 k,
                                                                       KT *__restrict__ ck, IT *__restrict__ ci, u64 cap)
{
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 WAVES = TOPK_THREADS / 64;
	if (ctl->mode != (FINAL ? (u32)FROM_CAND : 1u))
		return;
	if (FROM_CAND)
		n = ctl->cand_n;
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 g = blockIdx.x;
	if (!FROM_CAND && g == 0 && tid == 0)
		ctl->input_reads += 1;
	const u64 my_less = goff[2 * (size_t)g], my_in = goff[2 * (size_t)g + 1];
	if (!(my_less | my_in))
		return;
	__shared__ u64 s_a[WAVES], s_b[WAVES];
	__shared__ u32 s_w[WAVES];
	u64 a = 0, b = 0;
	for (u32 q = tid; q < g; q += TOPK_THREADS) {
		a += goff[2 * (size_t)q];
		b += goff[2 * (size_t)q + 1];
	}
	a = topk_wave_sum<u64>(a);
	b = topk_wave_sum<u64>(b);
	if (lane == 0) {
		s_a[wave] = a;
		s_b[wave] = b;
	}
	__syncthreads();
	u64 less_at = FROM_CAND ? ctl->pairs_n : 0, in_at = 0;
#pragma unroll
	for (u32 w = 0; w < WAVES; ++w) {
		less_at += s_a[w];
		in_at += s_b[w];
	}
	const u64 in_base = FINAL ? ctl->n_less : 0, in_limit = FINAL ? ctl->k_rem : cap;
	if (!my_less && in_at >= in_limit)
		return;
	const KT prefix = (KT)ctl->prefix, mask = (KT)ctl->mask;
	const bool aligned = ((uintptr_t)src & 15u) == 0;
	const u64 lo = (u64)g * chunk;
	const u64 hi = lo + chunk < n ? lo + chunk : n;
	for (u64 t0 = lo; t0 < hi; t0 += (u64)TOPK_THREADS * V) {
		const u64 i0 = t0 + (u64)tid * V;
		KT x[V];
		u32 fl = 0, fi = 0;
		if (i0 < hi) {
			topk_load<KT, V>(src, i0, hi, aligned, x);
#pragma unroll
			for (u32 e = 0; e < V; ++e) {
				const KT km = (KT)(kdf_apply(x[e], ka) & mask);
				const bool valid = i0 + e < hi;
				fl |= (valid && km < prefix ? 1u : 0u) << e;
				fi |= (valid && km == prefix ? 1u : 0u) << e;
			}
		} else {
#pragma unroll
			for (u32 e = 0; e < V; ++e)
				x[e] = 0;
		}
		// (at most 16 x 512 of either kind per sweep: two counts share a word)
		const u32 cnt = (u32)__popc(fl) | ((u32)__popc(fi) << 16);
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
		u64 ol = less_at + (before & 0xFFFFu), oi = in_at + (before >> 16);
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			if ((fl >> e) & 1u) {
				const u64 pos = ol++;
				if (pos < k) {
					pk[pos] = x[e];
					pi[pos] = FROM_CAND ? sidx[i0 + e] : (IT)(i0 + e);
				}
			}
			if ((fi >> e) & 1u) {
				const u64 j = oi++;
				if (j < in_limit) {
					if (FINAL) {
						if (in_base + j < k) {
							pk[in_base + j] = x[e];
							pi[in_base + j] = FROM_CAND ? sidx[i0 + e] : (IT)(i0 + e);
						}
					} else {
						ck[j] = x[e];
						ci[j] = (IT)(i0 + e);
					}
				}
			}
		}
		less_at += total & 0xFFFFu;
		in_at += total >> 16;
		__syncthreads();
	}
}

// the sort route: out_keys[j] = src[ranks[j]], out_idx[j] = ranks[j] for j < k; the k-th key is left in the control block
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_topk_gather_kernel(const KT *__restrict__ src, const IT *__restrict__ ranks, u64 k,
                                                               KT *__restrict__ out_keys, IT *__restrict__ out_idx, KdfArgs<KT> ka,
                                                               TopkCtl *ctl)
{
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < k; j += (u64)gridDim.x * 256u) {
		const IT r = ranks[j];
		const KT x = src[r];
		if (out_keys)
			out_keys[j] = x;
		if (out_idx)
			out_idx[j] = r;
		if (j == k - 1) {
			ctl->kth_raw = (u64)x;
			ctl->prefix = (u64)kdf_apply(x, ka);
		}
	}
}

// ... and how many elements lie below the k-th key (n_less) and how many equal it (bucket)
template <typename KT>
__global__ __launch_bounds__(TOPK_THREADS) void rsx_topk_count_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, TopkCtl *ctl)
{
	constexpr u32 V = 16 / sizeof(KT);
	const KT kth = (KT)ctl->prefix;
	const bool aligned = ((uintptr_t)src & 15u) == 0;
	u32 less = 0, eq = 0;
	__shared__ u32 s_l, s_e;
	if (threadIdx.x == 0)
		s_l = s_e = 0;
	__syncthreads();
	const u64 tile = (u64)TOPK_THREADS * V;
	for (u64 t0 = (u64)blockIdx.x * tile; t0 < n; t0 += (u64)gridDim.x * tile) {
		const u64 i0 = t0 + (u64)threadIdx.x * V;
		if (i0 >= n)
			break;
		KT x[V];
		topk_load<KT, V>(src, i0, n, aligned, x);
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			const KT kd = kdf_apply(x[e], ka);
			less += i0 + e < n && kd < kth ? 1u : 0u;
			eq += i0 + e < n && kd == kth ? 1u : 0u;
		}
	}
	less = topk_wave_sum<u32>(less);
	eq = topk_wave_sum<u32>(eq);
	if ((threadIdx.x & 63u) == 0) {
		atomicAdd(&s_l, less);
		atomicAdd(&s_e, eq);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		if (s_l)
			atomicAdd(&ctl->n_less, (u64)s_l);
		if (s_e)
			atomicAdd(&ctl->bucket, (u64)s_e);
	}
}

}  // namespace rsx
