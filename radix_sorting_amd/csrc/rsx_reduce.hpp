// rsx_reduce.hpp -- the kernels of rsx_sort_reduce_device: per group of equal keys (the groups of rsx_sort_unique, in its order)
// the number of elements and the sum, the minimum and the maximum of a second column (the arithmetic:
// rsx_reduce_shape.hpp).
//
// Where few bits of the derived keys vary, the packed varying bits (BitRuns, unique_pack) number a cell per possible key, and one
// streaming read of keys and values accumulates into the cells -- nothing is sorted and no inverse is written:
//
//   rsx_reduce_init_kernel     the table in device memory set to the identities (0, +0.0, all ones, 0)
//   rsx_reduce_cells_kernel    every element into cell pack(kdf(key)): in copies of the cells in the workgroup's LDS, merged into
//                              the table at the end (LDS), or in the table directly (!LDS)
//   rsx_reduce_readout_kernel  the cells in packed order, which is KDF order: the non-empty ones compacted into the outputs
//
// Everything else is sorted by key with the value as payload (stable: values of a group stay in input order), and then
//
//   rsx_reduce_runs_kernel     a segmented reduction by the head flags, tiled as rsx_group_heads_kernel: runs inside a tile are
//                              written, the part before a tile's first head and its last, open run go into a record per tile
//   rsx_reduce_seams_kernel    every run that crosses a tile boundary, combined left to right from those records
//
// Values are compared by their own KDF (ascending): one unsigned comparison for all six value types.  Sums are 64 bits wide:
// integers extended and added modulo 2^64, floats converted to f64 and added as doubles, every sum starting from +0.0.
#pragma once

#include "rsx_reduce_shape.hpp"
#include "rsx_unique.hpp"

namespace rsx {

template <u32 VB> struct reduce_val { typedef u32 type; };
template <> struct reduce_val<8> { typedef u64 type; };

// lanes with this many partners on one cell are reduced in the wave first (the peel of rsx_reduce_cells_kernel)
enum : u32 { REDUCE_PEEL_MIN = 16 };

// what a value adds to the sum of its group, as 64 bits
template <u32 VB, bool FLT> __device__ __forceinline__ u64 reduce_addend(typename reduce_val<VB>::type raw, u32 flags)
{
	if constexpr (FLT) {
		if constexpr (VB == 4)
			return (u64)__double_as_longlong((double)__uint_as_float(raw));
		else
			return raw;
	} else if constexpr (VB == 4) {
		return (flags & REDUCE_SIGNED) ? (u64)(long long)(int)raw : (u64)raw;
	} else {
		return raw;
	}
}
template <bool FLT> __device__ __forceinline__ u64 reduce_add(u64 a, u64 b)
{
	if constexpr (FLT)
		return (u64)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
	else
		return a + b;
}

// count, sum, smallest and largest derived value of some elements; the identity: {0, 0, ~0, 0}
template <typename VT> struct ReduceAgg {
	u32 cnt;
	u64 sum;
	VT mn, mx;
};
template <typename VT> __device__ __forceinline__ ReduceAgg<VT> reduce_none() { return ReduceAgg<VT>{0u, 0ull, (VT)~(VT)0, (VT)0}; }
// `a` then `b` (float sums are added in this order)
template <typename VT, bool FLT> __device__ __forceinline__ ReduceAgg<VT> reduce_join(const ReduceAgg<VT> &a, const ReduceAgg<VT> &b, u32 flags)
{
	ReduceAgg<VT> r;
	r.cnt = a.cnt + b.cnt;
	r.sum = (flags & REDUCE_SUM) ? reduce_add<FLT>(a.sum, b.sum) : 0ull;
	r.mn = a.mn < b.mn ? a.mn : b.mn;
	r.mx = a.mx > b.mx ? a.mx : b.mx;
	return r;
}
template <typename VT> __device__ __forceinline__ ReduceAgg<VT> reduce_shfl_up(const ReduceAgg<VT> &a, u32 off, u32 flags)
{
	ReduceAgg<VT> r;
	r.cnt = __shfl_up(a.cnt, off);
	r.sum = (flags & REDUCE_SUM) ? __shfl_up(a.sum, off) : 0ull;
	r.mn = (flags & REDUCE_MIN) ? __shfl_up(a.mn, off) : (VT)~(VT)0;
	r.mx = (flags & REDUCE_MAX) ? __shfl_up(a.mx, off) : (VT)0;
	return r;
}

// table[w], w < words (u32): all ones in [ones_lo, ones_hi) -- the minima --, zero elsewhere
__global__ __launch_bounds__(256) void rsx_reduce_init_kernel(u32 *__restrict__ table, u64 words, u64 ones_lo, u64 ones_hi)
{
	for (u64 w = (u64)blockIdx.x * 256u + threadIdx.x; w < words; w += (u64)gridDim.x * 256u)
		table[w] = (w >= ones_lo && w < ones_hi) ? ~0u : 0u;
}

// Every element i < n into cell p = pack(kdf(keys[i])): count + 1, sum + value, min / max of kdf(value) -- the parts `flags`
// wants.  A workgroup owns a contiguous share of the steps; a thread's step is E elements, whole 16-byte vectors of keys and of
// values (the values element by element where vals + head is not 16-byte aligned).  The elements before the first 16-byte
// boundary of keys and behind the last whole step are workgroup 0's, as in rsx_unique_mark_kernel.
//   LDS: lds.sets copies of the 2^cells_log2 cells in the workgroup's (dynamic) LDS, laid out by reduce_lds; a lane adds to copy
//     lane % sets.  At the end the non-empty cells, summed over the copies, go into the table with device-scope atomics.
//   !LDS: the atomics go to the table directly.
// The peel: per element the lanes that hold the packed value of the first lane are found with a ballot; REDUCE_PEEL_MIN of them or
// more are reduced in the wave and one lane adds for all of them -- a heavy key costs a wave one atomic, not 64 in a row.
// Minima and maxima are TESTED first (a stale read of the table can only show a value that is still to be improved on).
template <typename KT, u32 VB, bool FLT, bool LDS>
__global__ __launch_bounds__(REDUCE_THREADS) void rsx_reduce_cells_kernel(const KT *__restrict__ keys,
                                                                          const typename reduce_val<VB>::type *__restrict__ vals, u64 n,
                                                                          KdfArgs<KT> ka, KdfArgs<typename reduce_val<VB>::type> kv,
                                                                          BitRuns runs, u32 cells_log2, u32 flags, ReduceLds lds,
                                                                          u64 *__restrict__ table)
{
	typedef typename reduce_val<VB>::type VT;
	extern __shared__ __attribute__((aligned(16))) unsigned char s_reduce[];
	const u32 tid = threadIdx.x, lane = tid & 63u;
	const u32 C = 1u << cells_log2;
	u64 *const g_cnt = table, *const g_sum = table + C;
	VT *const g_min = (VT *)(table + 2u * (u64)C), *const g_max = g_min + C;
	unsigned char *const mine = s_reduce + (LDS ? (lane & (lds.sets - 1u)) * lds.stride : 0u);
	u64 *const s_sum = (u64 *)(mine + lds.sum_off);
	VT *const s_min = (VT *)(mine + lds.min_off), *const s_max = (VT *)(mine + lds.max_off);
	u32 *const s_cnt = (u32 *)(mine + lds.cnt_off);
	if (LDS) {
		for (u32 i = tid; i < lds.sets * C; i += REDUCE_THREADS) {
			unsigned char *const b = s_reduce + (i >> cells_log2) * lds.stride;
			const u32 cell = i & (C - 1u);
			((u32 *)(b + lds.cnt_off))[cell] = 0u;
			if (flags & REDUCE_SUM)
				((u64 *)(b + lds.sum_off))[cell] = 0ull;
			if (flags & REDUCE_MIN)
				((VT *)(b + lds.min_off))[cell] = (VT)~(VT)0;
			if (flags & REDUCE_MAX)
				((VT *)(b + lds.max_off))[cell] = (VT)0;
		}
		__syncthreads();
	}
	// `cnt` elements of cell p at once
	auto put = [&](u32 p, u32 cnt, u64 sum, VT mn, VT mx) {
		if (LDS) {
			atomicAdd(&s_cnt[p], cnt);
			if (flags & REDUCE_SUM) {
				if constexpr (FLT)
					unsafeAtomicAdd((double *)&s_sum[p], __longlong_as_double((long long)sum));
				else
					atomicAdd(&s_sum[p], sum);
			}
			if ((flags & REDUCE_MIN) && mn < s_min[p])
				atomicMin(&s_min[p], mn);
			if ((flags & REDUCE_MAX) && mx > s_max[p])
				atomicMax(&s_max[p], mx);
		} else {
			atomicAdd(&g_cnt[p], (u64)cnt);
			if (flags & REDUCE_SUM) {
				if constexpr (FLT)
					unsafeAtomicAdd((double *)&g_sum[p], __longlong_as_double((long long)sum));
				else
					atomicAdd(&g_sum[p], sum);
			}
			if ((flags & REDUCE_MIN) && mn < __atomic_load_n(&g_min[p], __ATOMIC_RELAXED))
				atomicMin(&g_min[p], mn);
			if ((flags & REDUCE_MAX) && mx > __atomic_load_n(&g_max[p], __ATOMIC_RELAXED))
				atomicMax(&g_max[p], mx);
		}
	};
	// one element per lane; every lane of the wave comes here together, `valid` says which hold one
	auto add = [&](const KT rawk, const VT rawv, const bool valid) {
		const u64 act = __ballot(valid);
		if (!act)
			return;
		const u32 p = unique_pack<KT>(kdf_apply(rawk, ka), runs) & (C - 1u);
		const u64 sum = reduce_addend<VB, FLT>(rawv, flags);
		const VT x = kdf_apply(rawv, kv);
		const u32 lead = (u32)__builtin_ctzll(act);
		const u32 first = (u32)__builtin_amdgcn_readlane((int)p, (int)lead);
		const u64 same = __ballot(valid && p == first);
		bool own = valid;
		if ((u32)__popcll(same) >= REDUCE_PEEL_MIN) {
			const bool in = (same >> lane) & 1ull;
			u64 s = in ? sum : 0ull;
			VT mn = in ? x : (VT)~(VT)0, mx = in ? x : (VT)0;
#pragma unroll
			for (u32 off = 32; off; off >>= 1) {
				if (flags & REDUCE_SUM)
					s = reduce_add<FLT>(s, __shfl_xor(s, off));
				if (flags & REDUCE_MIN) {
					const VT o = __shfl_xor(mn, off);
					mn = o < mn ? o : mn;
				}
				if (flags & REDUCE_MAX) {
					const VT o = __shfl_xor(mx, off);
					mx = o > mx ? o : mx;
				}
			}
			if (lane == lead)
				put(first, (u32)__popcll(same), s, mn, mx);
			own = valid && !in;
		}
		if (own)
			put(p, 1u, sum, x, x);
	};
	constexpr u32 E = (16u / sizeof(KT) > 16u / VB) ? 16u / (u32)sizeof(KT) : 16u / VB;
	constexpr u32 KPV = 16u / sizeof(KT), VPV = 16u / VB;   // elements of one vector
	typedef KT kvec_t __attribute__((ext_vector_type(KPV)));
	typedef VT vvec_t __attribute__((ext_vector_type(VPV)));
	u64 head = ((16u - (u32)((uintptr_t)keys & 15u)) & 15u) / sizeof(KT);
	if (head > n)
		head = n;
	const u64 nstep = (n - head) / E;
	const bool vec_ok = ((uintptr_t)(vals + head) & 15u) == 0;
	const u64 per = (nstep + gridDim.x - 1) / gridDim.x;
	const u64 lo = (u64)blockIdx.x * per < nstep ? (u64)blockIdx.x * per : nstep, hi = lo + per < nstep ? lo + per : nstep;
	for (u64 s0 = lo; s0 < hi; s0 += REDUCE_THREADS) {   // (the same trips for every lane: the ballots want whole waves)
		const u64 s = s0 + tid;
		const bool valid = s < hi;
		KT k[E];
		VT x[E];
#pragma unroll
		for (u32 e = 0; e < E; ++e) {
			k[e] = 0;
			x[e] = 0;
		}
		if (valid) {
			const KT *kp = keys + head + s * E;
			const VT *vp = vals + head + s * E;
#pragma unroll
			for (u32 i = 0; i < E / KPV; ++i) {
				const kvec_t kvv = ((const kvec_t *)kp)[i];
#pragma unroll
				for (u32 e = 0; e < KPV; ++e)
					k[i * KPV + e] = kvv[e];
			}
			if (vec_ok) {
#pragma unroll
				for (u32 i = 0; i < E / VPV; ++i) {
					const vvec_t vv = ((const vvec_t *)vp)[i];
#pragma unroll
					for (u32 e = 0; e < VPV; ++e)
						x[i * VPV + e] = vv[e];
				}
			} else {
#pragma unroll
				for (u32 e = 0; e < E; ++e)
					x[e] = vp[e];
			}
		}
#pragma unroll
		for (u32 e = 0; e < E; ++e)
			add(k[e], x[e], valid);
	}
	if (blockIdx.x == 0) {
		// fewer than 16 elements in front and fewer than E <= 16 behind: one element per thread of the first wave
		const u64 t0 = head + nstep * E;
		const u64 extra = head + (n - t0);
		if (tid < 64u) {
			const bool valid = tid < extra;
			const u64 i = tid < head ? tid : t0 + (tid - head);
			add(valid ? keys[i] : (KT)0, valid ? vals[i] : (VT)0, valid);
		}
	}
	if (LDS) {
		__syncthreads();
		for (u32 cell = tid; cell < C; cell += REDUCE_THREADS) {
			u32 cnt = 0;
			u64 sum = 0;
			VT mn = (VT)~(VT)0, mx = 0;
			for (u32 r = 0; r < lds.sets; ++r) {
				const unsigned char *const b = s_reduce + r * lds.stride;
				cnt += ((const u32 *)(b + lds.cnt_off))[cell];
				if (flags & REDUCE_SUM)
					sum = reduce_add<FLT>(sum, ((const u64 *)(b + lds.sum_off))[cell]);
				if (flags & REDUCE_MIN) {
					const VT o = ((const VT *)(b + lds.min_off))[cell];
					mn = o < mn ? o : mn;
				}
				if (flags & REDUCE_MAX) {
					const VT o = ((const VT *)(b + lds.max_off))[cell];
					mx = o > mx ? o : mx;
				}
			}
			if (!cnt)
				continue;
			atomicAdd(&g_cnt[cell], (u64)cnt);
			if (flags & REDUCE_SUM) {
				if constexpr (FLT)
					unsafeAtomicAdd((double *)&g_sum[cell], __longlong_as_double((long long)sum));
				else
					atomicAdd(&g_sum[cell], sum);
			}
			if (flags & REDUCE_MIN)
				atomicMin(&g_min[cell], mn);
			if (flags & REDUCE_MAX)
				atomicMax(&g_max[cell], mx);
		}
	}
}

// what one group's results are written with: each output may be nullptr
template <typename VT> struct ReduceOutPtrs {
	void *counts;
	u32 count_bytes;
	u64 *sum;
	VT *mn, *mx;
};
template <typename VT>
__device__ __forceinline__ void reduce_emit(const ReduceOutPtrs<VT> &o, u64 g, u64 cnt, u64 sum, VT mn, VT mx, KdfArgs<VT> kv)
{
	if (o.counts) {
		if (o.count_bytes == 4)
			((u32 *)o.counts)[g] = (u32)cnt;
		else
			((u64 *)o.counts)[g] = cnt;
	}
	if (o.sum)
		o.sum[g] = sum;
	if (o.mn)
		o.mn[g] = kdf_invert<VT>(mn, kv);
	if (o.mx)
		o.mx[g] = kdf_invert<VT>(mx, kv);
}

// The table read out by one workgroup: the 2^cells_log2 cells in packed order, a contiguous stretch per thread; the non-empty
// ones are numbered and written compacted.  A cell's key: the packed value spread back over the varying bits, the other bits
// taken from the first key (`kmask`: the bits the runs cover), kdf_invert -- as rsx_unique_expand_kernel.  *total = their number.
template <typename KT, u32 VB>
__global__ __launch_bounds__(1024) void rsx_reduce_readout_kernel(const u64 *__restrict__ table, u32 cells_log2, const KT *__restrict__ src,
                                                                  KdfArgs<KT> ka, KdfArgs<typename reduce_val<VB>::type> kv, BitRuns runs,
                                                                  KT kmask, KT *__restrict__ out_keys,
                                                                  ReduceOutPtrs<typename reduce_val<VB>::type> out, u64 *__restrict__ total)
{
	typedef typename reduce_val<VB>::type VT;
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 C = 1u << cells_log2;
	const u64 *const g_cnt = table, *const g_sum = table + C;
	const VT *const g_min = (const VT *)(table + 2u * (u64)C), *const g_max = g_min + C;
	const u32 per = (C + 1023u) / 1024u;
	const u32 lo = tid * per < C ? tid * per : C, hi = lo + per < C ? lo + per : C;
	u32 c = 0;
	for (u32 d = lo; d < hi; ++d)
		c += g_cnt[d] != 0;
	const u32 incl = unique_wave_incl_sum<u32>(c, lane);
	__shared__ u32 s_w[16];
	if (lane == 63u)
		s_w[wave] = incl;
	__syncthreads();
	u32 o = incl - c, all = 0;
	for (u32 w = 0; w < 16u; ++w) {
		o += w < wave ? s_w[w] : 0u;
		all += s_w[w];
	}
	const KT kconst = (KT)(kdf_apply(src[0], ka) & (KT)~kmask);
	for (u32 d = lo; d < hi; ++d) {
		const u64 cd = g_cnt[d];
		if (!cd)
			continue;
		if (out_keys)
			out_keys[o] = kdf_invert<KT>((KT)(kconst | unique_unpack<KT>(d, runs)), ka);
		reduce_emit<VT>(out, o, cd, g_sum[d], g_min[d], g_max[d], kv);
		++o;
	}
	if (tid == 0)
		total[0] = all;
}

// ---- the sort route -----------------------------------------------------------------------------------------------------------
// what a tile of the sorted array leaves for the seams (reduce_seam_last): `heads` in it; the elements before its first head
// (all of them where it has none) and those from its last head on
struct ReducePart {
	u64 heads;
	u64 lead_cnt, lead_sum, lead_min, lead_max;
	u64 tail_cnt, tail_sum, tail_min, tail_max;
	u64 pad;
};

// Over the sorted keys `in` and their values `vals`, tiled as rsx_group_heads_kernel (recs: rsx_unique_heads_kernel<KT, 0>'s,
// scanned: the heads before the tile).  A thread folds its 16 bytes of keys' worth of elements in order; what it contributes to
// the run that is open at its end -- everything, or the elements from its last head on -- is scanned over the wave, the waves
// and the sweeps of the tile with the segmented operator (a part with a head forgets what came before it).  At its first head
// a thread closes the run that was open before it: that is group (heads before) - 1 where the run began inside the tile, the
// tile's lead otherwise; runs between two heads of one thread are written as they are.  keys[g] = the key at head g.
template <typename KT, u32 VB, bool FLT>
__global__ __launch_bounds__(UNIQUE_HEADS_THREADS) void rsx_reduce_runs_kernel(const KT *__restrict__ in,
                                                                               const typename reduce_val<VB>::type *__restrict__ vals, u64 n,
                                                                               const UniqueRec *__restrict__ recs,
                                                                               KdfArgs<typename reduce_val<VB>::type> kv, u32 flags,
                                                                               KT *__restrict__ keys,
                                                                               ReduceOutPtrs<typename reduce_val<VB>::type> out,
                                                                               ReducePart *__restrict__ parts)
{
	typedef typename reduce_val<VB>::type VT;
	typedef ReduceAgg<VT> Agg;
	constexpr u32 V = 16 / sizeof(KT);
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const bool aligned = ((uintptr_t)in & 15u) == 0;
	const u64 base = (u64)blockIdx.x * unique_heads_tile<KT>();
	constexpr u32 WAVES = UNIQUE_HEADS_THREADS / 64;
	constexpr u32 VALIGN = V * sizeof(VT) < 16 ? V * (u32)sizeof(VT) : 16u;
	__shared__ u32 s_c[WAVES], s_f[WAVES], s_cnt[WAVES];
	__shared__ u64 s_sum[WAVES];
	__shared__ VT s_mn[WAVES], s_mx[WAVES];
	const u64 rec_c = recs[blockIdx.x].cnt;
	u32 carry_c = 0;        // heads in the sweeps before this one
	u32 carry_f = 0;        // ... whether there was one: then carry_a is the run open since the last of them
	Agg carry_a = reduce_none<VT>();
	auto elem = [&](VT raw) { return Agg{1u, (flags & REDUCE_SUM) ? reduce_addend<VB, FLT>(raw, flags) : 0ull, kdf_apply(raw, kv), kdf_apply(raw, kv)}; };
	for (u32 j = 0; j < UNIQUE_HEADS_ITER; ++j) {
		const u32 r0 = (j * UNIQUE_HEADS_THREADS + tid) * V;
		const u64 i0 = base + r0;
		KT x[V];
		VT y[V];
		KT prev = 0;
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			x[e] = 0;
			y[e] = 0;
		}
		if (i0 < n) {
			if (aligned && i0 + V <= n) {
				const kvec_t xv = *(const kvec_t *)(in + i0);
#pragma unroll
				for (u32 e = 0; e < V; ++e)
					x[e] = xv[e];
			} else {
#pragma unroll
				for (u32 e = 0; e < V; ++e)
					x[e] = i0 + e < n ? in[i0 + e] : (KT)0;
			}
			if (i0 + V <= n && ((uintptr_t)(vals + i0) & (VALIGN - 1u)) == 0) {
				// (V values: 8 to 128 bytes, read as whole vectors of at most 16 bytes where they are aligned for them)
				__builtin_memcpy(y, __builtin_assume_aligned(vals + i0, VALIGN), V * sizeof(VT));
			} else {
#pragma unroll
				for (u32 e = 0; e < V; ++e)
					y[e] = i0 + e < n ? vals[i0 + e] : (VT)0;
			}
			if (i0)
				prev = in[i0 - 1];
		}
		u32 f = 0;
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			const bool h = i0 + e < n && (i0 + e == 0 || x[e] != (e ? x[e - 1] : prev));
			f |= (h ? 1u : 0u) << e;
		}
		const u32 c = (u32)__popc(f);
		// the thread's lead (before its first head; everything where it has none) and what it leaves open
		Agg lead = reduce_none<VT>(), cur = reduce_none<VT>();
#pragma unroll
		for (u32 e = 0; e < V; ++e) {
			if (i0 + e < n) {
				if (f >> e & 1u) {
					if (!(f & ((1u << e) - 1u)))
						lead = cur;
					cur = reduce_none<VT>();
				}
				cur = reduce_join<VT, FLT>(cur, elem(y[e]), flags);
			}
		}
		// inclusive scans over the wave: the heads, and the open run with its flag
		const u32 incl_c = unique_wave_incl_sum<u32>(c, lane);
		u32 sf = f ? 1u : 0u;
		Agg sa = cur;
#pragma unroll
		for (u32 off = 1; off < 64; off <<= 1) {
			const u32 of = __shfl_up(sf, off);
			const Agg oa = reduce_shfl_up<VT>(sa, off, flags);
			if (lane >= off) {
				if (!sf)
					sa = reduce_join<VT, FLT>(oa, sa, flags);
				sf |= of;
			}
		}
		if (lane == 63u) {
			s_c[wave] = incl_c;
			s_f[wave] = sf;
			s_cnt[wave] = sa.cnt;
			s_sum[wave] = sa.sum;
			s_mn[wave] = sa.mn;
			s_mx[wave] = sa.mx;
		}
		__syncthreads();
		// what is open before this wave (pf, pa) and behind the sweep (tf, ta), from what was open before the sweep
		u32 wb_c = 0, tot_c = 0, pf = carry_f, tf = carry_f;
		Agg pa = carry_a, ta = carry_a;
#pragma unroll
		for (u32 w = 0; w < WAVES; ++w) {
			const u32 wf = s_f[w];
			const Agg wa = Agg{s_cnt[w], s_sum[w], s_mn[w], s_mx[w]};
			if (w < wave) {
				wb_c += s_c[w];
				pa = wf ? wa : reduce_join<VT, FLT>(pa, wa, flags);
				pf |= wf;
			}
			tot_c += s_c[w];
			ta = wf ? wa : reduce_join<VT, FLT>(ta, wa, flags);
			tf |= wf;
		}
		// ... and before this thread: the wave's inclusive scan one lane up (every lane takes part in the shuffles)
		u32 xf = __shfl_up(sf, 1u);
		Agg xa = reduce_shfl_up<VT>(sa, 1u, flags);
		if (!lane) {
			xf = pf;
			xa = pa;
		} else {
			xa = xf ? xa : reduce_join<VT, FLT>(pa, xa, flags);
			xf |= pf;
		}
		if (f) {
			const u64 hb = rec_c + carry_c + wb_c + incl_c - c;   // heads before this thread's elements: its first head is group hb
			const Agg closed = reduce_join<VT, FLT>(xa, lead, flags);
			if (xf) {
				reduce_emit<VT>(out, hb - 1u, closed.cnt, closed.sum, closed.mn, closed.mx, kv);
			} else {
				ReducePart *const p = parts + blockIdx.x;
				p->lead_cnt = closed.cnt;
				p->lead_sum = closed.sum;
				p->lead_min = closed.mn;
				p->lead_max = closed.mx;
			}
			// the keys at the heads, and the runs between two heads of this thread
			Agg run = reduce_none<VT>();
			u32 h = 0;
#pragma unroll
			for (u32 e = 0; e < V; ++e) {
				if (i0 + e < n) {
					if (f >> e & 1u) {
						if (h)
							reduce_emit<VT>(out, hb + h - 1u, run.cnt, run.sum, run.mn, run.mx, kv);
						if (keys)
							keys[hb + h] = x[e];
						++h;
						run = reduce_none<VT>();
					}
					run = reduce_join<VT, FLT>(run, elem(y[e]), flags);
				}
			}
		}
		carry_c += tot_c;
		carry_f = tf;
		carry_a = ta;
		__syncthreads();
	}
	if (tid == 0) {
		ReducePart *const p = parts + blockIdx.x;
		p->heads = carry_c;
		if (carry_f) {
			p->tail_cnt = carry_a.cnt;
			p->tail_sum = carry_a.sum;
			p->tail_min = carry_a.mn;
			p->tail_max = carry_a.mx;
		} else {
			p->lead_cnt = carry_a.cnt;
			p->lead_sum = carry_a.sum;
			p->lead_min = carry_a.mn;
			p->lead_max = carry_a.mx;
		}
	}
}

// One thread per tile that has a head: the run open at its end -- group (heads before the tile) + (its heads) - 1 -- is its tail
// and the leads of the tiles behind it up to reduce_seam_last, joined left to right and written once.  No atomics: float sums on
// this route come out the same from run to run.
template <u32 VB, bool FLT>
__global__ __launch_bounds__(256) void rsx_reduce_seams_kernel(const ReducePart *__restrict__ parts, const UniqueRec *__restrict__ recs,
                                                               u64 tiles, KdfArgs<typename reduce_val<VB>::type> kv, u32 flags,
                                                               ReduceOutPtrs<typename reduce_val<VB>::type> out)
{
	typedef typename reduce_val<VB>::type VT;
	const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
	if (t >= tiles || !parts[t].heads)
		return;
	u64 cnt = parts[t].tail_cnt, sum = parts[t].tail_sum;
	VT mn = (VT)parts[t].tail_min, mx = (VT)parts[t].tail_max;
	const u64 last = reduce_seam_last(t, tiles, [&](u64 e) { return parts[e].heads != 0; });
	for (u64 e = t + 1; e <= last; ++e) {
		const ReducePart p = parts[e];
		cnt += p.lead_cnt;
		if (flags & REDUCE_SUM)
			sum = reduce_add<FLT>(sum, p.lead_sum);
		mn = (VT)p.lead_min < mn ? (VT)p.lead_min : mn;
		mx = (VT)p.lead_max > mx ? (VT)p.lead_max : mx;
	}
	reduce_emit<VT>(out, recs[t].cnt + parts[t].heads - 1u, cnt, sum, mn, mx, kv);
}

}  // namespace rsx
