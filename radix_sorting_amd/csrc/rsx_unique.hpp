// rsx_unique.hpp -- the kernels of rsx_sort_unique_device: the distinct keys of an array in order of kdf(key), and
// optionally how many of each (README.md "Uniquely sorting with bitmaps", bitmap_sort_16.c: Listing 7).
//
// Where few bits of the derived keys vary, one bit per possible value replaces the sort: the varying bits are packed
// together (BitRuns, the "key compaction" of README.md:716-758 -- order-preserving, all other bits are the same in every
// key), every key sets its bit, and the set bits read out in ascending order ARE the sorted distinct keys.
//
//   rsx_unique_sample_kernel   OR and AND of a few thousand derived keys: a lower bound of the varying bits (existential,
//                              hence sound) that sends evenly spread keys to the sort before any histogram is made
//   rsx_unique_mark_kernel     every key sets its bit -- in a bitmap in LDS per workgroup (64 Ki / 256 Ki / 1 Mi bits), ORed
//                              into the one in device memory at the end, or in the one in device memory directly
//   rsx_unique_expand_kernel   the bitmap read out: set bits per chunk, (scan,) one key per set bit
//   rsx_unique_table_kernel    a count table that exists already (one kept column's 256 counts, the 65536 counts of
//                              rsx_joint16_kernel) read out: keys and counts of the non-empty bins
//   rsx_unique_heads_kernel    the sorted array compacted: head flags i == 0 || a[i] != a[i-1] on raw bits, counted per
//                              tile, (scan,) keys written and counts as differences of head positions
//   rsx_unique_scan_kernel     the exclusive scan of the per-chunk / per-tile records between the two phases
#pragma once

#include "rsx_kernels.hpp"

namespace rsx {

// what a chunk of the bitmap / a tile of the sorted array holds: set bits / heads, and the position + 1 of its last head
// (0: none); after the scan: the number of heads before the tile, and the position + 1 of the last head before it
struct UniqueRec {
	u64 cnt;
	u64 last;
};

enum : u32 { UNIQUE_CHUNK_WORDS = 1024, UNIQUE_SAMPLE = 4096 };

template <typename KT> __device__ __forceinline__ u32 unique_pack(KT k, const BitRuns &runs)
{
	KT o = 0;
	for (u32 r = 0; r < runs.n; ++r)   // (uniform: the runs are kernel arguments)
		o |= (KT)((KT)((k >> runs.src[r]) & (KT)(((KT)1 << runs.len[r]) - 1)) << runs.dst[r]);
	return (u32)o;
}

template <typename KT> __device__ __forceinline__ KT unique_unpack(u32 p, const BitRuns &runs)
{
	KT k = 0;
	for (u32 r = 0; r < runs.n; ++r)
		k |= (KT)((KT)(((KT)p >> runs.dst[r]) & (KT)(((KT)1 << runs.len[r]) - 1)) << runs.src[r]);
	return k;
}

template <typename T> __device__ __forceinline__ T unique_wave_incl_sum(T v, u32 lane)
{
#pragma unroll
	for (u32 off = 1; off < 64; off <<= 1) {
		const T o = __shfl_up(v, off);
		if (lane >= off)
			v += o;
	}
	return v;
}

__device__ __forceinline__ u32 unique_wave_incl_max(u32 v, u32 lane)
{
#pragma unroll
	for (u32 off = 1; off < 64; off <<= 1) {
		const u32 o = __shfl_up(v, off);
		if (lane >= off && o > v)
			v = o;
	}
	return v;
}

// out[0] |= kdf(key), out[1] &= kdf(key) over UNIQUE_SAMPLE keys spread evenly over the array (out: {0, ~0} on entry)
template <typename KT>
__global__ __launch_bounds__(1024) void rsx_unique_sample_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, u64 *__restrict__ out)
{
	const u32 tid = threadIdx.x, lane = tid & 63u;
	u64 o = 0, a = ~0ull;
	const u64 step = n / UNIQUE_SAMPLE ? n / UNIQUE_SAMPLE : 1;
	for (u32 s = tid; s < (u32)UNIQUE_SAMPLE; s += 1024u) {
		const u64 i = (u64)s * step;
		if (i < n) {
			const u64 k = (u64)kdf_apply(src[i], ka);
			o |= k;
			a &= k;
		}
	}
#pragma unroll
	for (u32 off = 32; off; off >>= 1) {
		o |= __shfl_xor(o, off);
		a &= __shfl_xor(a, off);
	}
	if (lane == 0) {
		atomicOr(&out[0], o);
		atomicAnd(&out[1], a);
	}
}

// Every key sets bit pack(kdf(key)).  A workgroup owns a contiguous share of the keys and reads it with 16-byte loads (the
// elements before the first 16-byte boundary and behind the last whole vector are workgroup 0's).  The word is TESTED
// first and the atomic issued only if the bit is still clear: duplicates and sorted inputs cost reads, not atomics that
// serialise on one address.
//   LDS_LOG2 = 16 / 18 / 20: the workgroup's own bitmap of 2^LDS_LOG2 bits in LDS (8 / 32 / 128 KiB), its non-zero words
//     ORed into the bitmap in device memory at the end;
//   LDS_LOG2 = 0: the bitmap in device memory directly, device-scope atomicOr.  The test reads the word without any
//     ordering, so it may see a STALE value -- which can only show a bit as still clear: bits are never cleared after the
//     stream-ordered memset in front of this kernel, so staleness costs a redundant atomic, never a wrong result.
template <typename KT, u32 LDS_LOG2>
__global__ __launch_bounds__(1024) void rsx_unique_mark_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, BitRuns runs,
                                                               u32 *__restrict__ bitmap)
{
	constexpr u32 WORDS = LDS_LOG2 ? (1u << LDS_LOG2) / 32u : 1u;
	__shared__ u32 bm[WORDS];
	const u32 tid = threadIdx.x;
	if (LDS_LOG2) {
		for (u32 i = tid; i < WORDS; i += 1024u)
			bm[i] = 0;
		__syncthreads();
	}
	auto mark = [&](const KT raw) {
		const u32 p = unique_pack<KT>(kdf_apply(raw, ka), runs);
		const u32 w = p >> 5, bit = 1u << (p & 31u);
		if (LDS_LOG2) {
			if (!(bm[w] & bit))
				atomicOr(&bm[w], bit);
		} else {
			if (!(__atomic_load_n(&bitmap[w], __ATOMIC_RELAXED) & bit))
				atomicOr(&bitmap[w], bit);
		}
	};
	constexpr u32 V = 16 / sizeof(KT);
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	u64 head = ((16u - (u32)((uintptr_t)src & 15u)) & 15u) / sizeof(KT);
	if (head > n)
		head = n;
	const u64 nvec = (n - head) / V;
	const kvec_t *vsrc = (const kvec_t *)(src + head);
	const u64 per = (nvec + gridDim.x - 1) / gridDim.x;
	const u64 lo = (u64)blockIdx.x * per, hi = lo + per < nvec ? lo + per : nvec;
	constexpr u32 U = 4;
	for (u64 v = lo + tid; v < hi; v += 1024u * U) {
		kvec_t x[U];
#pragma unroll
		for (u32 u = 0; u < U; ++u)
			if (v + u * 1024u < hi)
				x[u] = vsrc[v + u * 1024u];
#pragma unroll
		for (u32 u = 0; u < U; ++u)
			if (v + u * 1024u < hi) {
#pragma unroll
				for (u32 e = 0; e < V; ++e)
					mark(x[u][e]);
			}
	}
	if (blockIdx.x == 0) {
		if (tid < head)
			mark(src[tid]);
		const u64 t0 = head + nvec * V;
		if (t0 + tid < n)
			mark(src[t0 + tid]);
	}
	if (LDS_LOG2) {
		__syncthreads();
		for (u32 i = tid; i < WORDS; i += 1024u) {
			const u32 w = bm[i];   // (a non-zero word lies below 2^(varying bits) / 32: inside the bitmap in device memory)
			if (w && (__atomic_load_n(&bitmap[i], __ATOMIC_RELAXED) & w) != w)
				atomicOr(&bitmap[i], w);
		}
	}
}

// The exclusive scan of `count` records by one workgroup: cnt by sum, last by maximum; *total = {sum, maximum} of all.
__global__ __launch_bounds__(1024) void rsx_unique_scan_kernel(UniqueRec *__restrict__ recs, u64 count, u64 *__restrict__ total)
{
	__shared__ u64 s_sum[2][1024];
	__shared__ u64 s_max[2][1024];
	const u32 tid = threadIdx.x;
	const u64 per = (count + 1023) / 1024;
	const u64 lo = (u64)tid * per < count ? (u64)tid * per : count, hi = lo + per < count ? lo + per : count;
	u64 sum = 0, mx = 0;
	for (u64 i = lo; i < hi; ++i) {
		sum += recs[i].cnt;
		mx = recs[i].last > mx ? recs[i].last : mx;
	}
	u32 cur = 0;
	s_sum[0][tid] = sum;
	s_max[0][tid] = mx;
	__syncthreads();
	for (u32 off = 1; off < 1024u; off <<= 1) {
		u64 a = s_sum[cur][tid], m = s_max[cur][tid];
		if (tid >= off) {
			a += s_sum[cur][tid - off];
			const u64 o = s_max[cur][tid - off];
			m = o > m ? o : m;
		}
		s_sum[cur ^ 1u][tid] = a;
		s_max[cur ^ 1u][tid] = m;
		cur ^= 1u;
		__syncthreads();
	}
	u64 run = s_sum[cur][tid] - sum, runmax = tid ? s_max[cur][tid - 1] : 0;
	for (u64 i = lo; i < hi; ++i) {
		const UniqueRec r = recs[i];
		recs[i].cnt = run;
		recs[i].last = runmax;
		run += r.cnt;
		runmax = r.last > runmax ? r.last : runmax;
	}
	if (tid == 1023u) {
		total[0] = s_sum[cur][1023];
		total[1] = s_max[cur][1023];
	}
}

// The bitmap read out, a chunk of UNIQUE_CHUNK_WORDS words (four per thread) per workgroup.
//   PHASE 0: recs[chunk] = {set bits, 0};
//   PHASE 1 (after the scan): Listing 7's loop per word -- isolate the lowest set bit, count the zeros below it, clear it --
//     and for every bit the key: the packed value spread back over the varying bits (the inverse of the BitRuns), the
//     constant bits taken from the first key, kdf_invert.
template <typename KT, int PHASE>
__global__ __launch_bounds__(256) void rsx_unique_expand_kernel(const u32 *__restrict__ bitmap, UniqueRec *__restrict__ recs,
                                                                KT *__restrict__ out, const KT *__restrict__ src, KdfArgs<KT> ka,
                                                                BitRuns runs, KT vary)
{
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u64 w0 = (u64)blockIdx.x * UNIQUE_CHUNK_WORDS + 4u * tid;
	const u32x4 x = *(const u32x4 *)(bitmap + w0);
	const u32 c = (u32)__popc(x.x) + (u32)__popc(x.y) + (u32)__popc(x.z) + (u32)__popc(x.w);
	const u32 incl = unique_wave_incl_sum<u32>(c, lane);
	__shared__ u32 s_w[4];
	if (lane == 63u)
		s_w[wave] = incl;
	__syncthreads();
	if (PHASE == 0) {
		if (tid == 0) {
			recs[blockIdx.x].cnt = (u64)s_w[0] + s_w[1] + s_w[2] + s_w[3];
			recs[blockIdx.x].last = 0;
		}
		return;
	}
	u32 before = incl - c;
	for (u32 w = 0; w < wave; ++w)
		before += s_w[w];
	if (!c)
		return;
	const KT kconst = (KT)(kdf_apply(src[0], ka) & (KT)~vary);
	u64 o = recs[blockIdx.x].cnt + before;
	const u32 words[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
	for (u32 j = 0; j < 4; ++j) {
		u32 w = words[j];
		while (w) {
			const u32 b = (u32)__builtin_ctz(w);
			w &= w - 1u;
			const u32 p = (u32)((w0 + j) << 5) | b;
			out[o++] = kdf_invert<KT>((KT)(kconst | unique_unpack<KT>(p, runs)), ka);
		}
	}
}

// A count table read out by one workgroup: `entries` bins (256: one column's EXCLUSIVE OFFSETS in `offs`, the last bin ends
// at n; 65536: rsx_joint16_kernel's counts in `cnts`), bin d standing for the derived key kconst | d << shift, where kconst
// are the bits of kdf(src[0]) outside the bins' (every key has them: that is what a skipped column means,
// radix_sort.hpp:64-70).  Keys and counts of the non-empty bins, ascending; *total = their number.  The keys are not read.
template <typename KT>
__global__ __launch_bounds__(1024) void rsx_unique_table_kernel(const u64 *__restrict__ offs, const u32 *__restrict__ cnts, u32 entries,
                                                                u64 n, u32 shift, const KT *__restrict__ src, KdfArgs<KT> ka,
                                                                KT *__restrict__ out, void *__restrict__ counts, u32 count_bytes,
                                                                u64 *__restrict__ total)
{
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 per = entries >= 1024u ? entries / 1024u : 1u;
	const u32 lo = tid * per < entries ? tid * per : entries, hi = lo + per < entries ? lo + per : entries;
	auto count_of = [&](u32 d) -> u64 {
		if (cnts)
			return cnts[d];
		return (d + 1u < entries ? offs[d + 1u] : n) - offs[d];
	};
	u32 c = 0;
	for (u32 d = lo; d < hi; ++d)
		c += count_of(d) != 0;
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
	const KT binmask = (KT)((KT)(entries - 1u) << shift);
	const KT kconst = (KT)(kdf_apply(src[0], ka) & (KT)~binmask);
	for (u32 d = lo; d < hi; ++d) {
		const u64 cd = count_of(d);
		if (!cd)
			continue;
		out[o] = kdf_invert<KT>((KT)(kconst | (KT)((KT)d << shift)), ka);
		if (counts) {
			if (count_bytes == 4)
				((u32 *)counts)[o] = (u32)cd;
			else
				((u64 *)counts)[o] = cd;
		}
		++o;
	}
	if (tid == 0)
		total[0] = all;
}

// The sorted array `in` compacted into `out` (the other buffer).  A tile is UNIQUE_HEADS_ITER sweeps of UNIQUE_HEADS_THREADS threads x one
// 16-byte vector; element i is a head iff i == 0 or its bits differ from element i - 1's.
//   PHASE 0: recs[tile] = {heads, position + 1 of the last head (0: none)};
//   PHASE 1 (after the scan: heads before the tile, last head before the tile): out[j] = the j-th head, and
//     counts[j - 1] = its position minus the position of the head before it -- the last count, n minus the last head's
//     position, is the last tile's to write.
enum : u32 { UNIQUE_HEADS_ITER = 4, UNIQUE_HEADS_THREADS = 512 };
template <typename KT> constexpr u32 unique_heads_tile() { return UNIQUE_HEADS_ITER * UNIQUE_HEADS_THREADS * (16u / (u32)sizeof(KT)); }

template <typename KT, int PHASE>
__global__ __launch_bounds__(UNIQUE_HEADS_THREADS) void rsx_unique_heads_kernel(const KT *__restrict__ in, u64 n, UniqueRec *__restrict__ recs,
                                                                KT *__restrict__ out, void *__restrict__ counts, u32 count_bytes)
{
	constexpr u32 V = 16 / sizeof(KT);
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const bool aligned = ((uintptr_t)in & 15u) == 0;
	const u64 base = (u64)blockIdx.x * unique_heads_tile<KT>();
	constexpr u32 WAVES = UNIQUE_HEADS_THREADS / 64;
	__shared__ u32 s_c[WAVES], s_l[WAVES];
	// inside the tile heads are counted and positions kept in 32 bits, relative to the tile (position + 1; 0: none)
	u32 carry_c = 0, carry_l = 0;
	u64 rec_c = 0, rec_l = 0;
	if (PHASE == 1) {
		rec_c = recs[blockIdx.x].cnt;
		rec_l = recs[blockIdx.x].last;
	}
	for (u32 j = 0; j < UNIQUE_HEADS_ITER; ++j) {
		const u32 r0 = (j * UNIQUE_HEADS_THREADS + tid) * V;
		const u64 i0 = base + r0;
		KT x[V];
		KT prev = 0;
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
		const u32 l = f ? r0 + (31u - (u32)__builtin_clz(f)) + 1u : 0u;
		const u32 incl_c = unique_wave_incl_sum<u32>(c, lane);
		const u32 incl_l = unique_wave_incl_max(l, lane);
		if (lane == 63u) {
			s_c[wave] = incl_c;
			s_l[wave] = incl_l;
		}
		__syncthreads();
		u32 wb_c = 0, wb_l = 0, tot_c = 0, tot_l = 0;
#pragma unroll
		for (u32 w = 0; w < WAVES; ++w) {
			const u32 sc = s_c[w], sl = s_l[w];
			if (w < wave) {
				wb_c += sc;
				wb_l = sl > wb_l ? sl : wb_l;
			}
			tot_c += sc;
			tot_l = sl > tot_l ? sl : tot_l;
		}
		u32 plr = __shfl_up(incl_l, 1u);   // the last head before this lane's elements (every lane takes part in the shuffle)
		plr = lane ? plr : 0u;
		plr = plr > wb_l ? plr : wb_l;
		plr = plr > carry_l ? plr : carry_l;
		if (PHASE == 1 && f) {
			u64 o = rec_c + carry_c + wb_c + incl_c - c;
			u64 pl = plr ? base + plr : rec_l;
			while (f) {
				const u32 e = (u32)__builtin_ctz(f);
				f &= f - 1u;
				KT xe = x[0];
#pragma unroll
				for (u32 q = 1; q < V; ++q)
					xe = q == e ? x[q] : xe;
				out[o] = xe;
				if (counts && o) {
					const u64 cnt = i0 + e + 1 - pl;
					if (count_bytes == 4)
						((u32 *)counts)[o - 1] = (u32)cnt;
					else
						((u64 *)counts)[o - 1] = cnt;
				}
				pl = i0 + e + 1;
				++o;
			}
		}
		carry_c += tot_c;
		carry_l = tot_l > carry_l ? tot_l : carry_l;
		__syncthreads();
	}
	if (PHASE == 0) {
		if (tid == 0) {
			recs[blockIdx.x].cnt = carry_c;
			recs[blockIdx.x].last = carry_l ? base + carry_l : 0;
		}
	} else if (counts && blockIdx.x == gridDim.x - 1 && tid == 0) {
		const u64 total = rec_c + carry_c, last = carry_l ? base + carry_l : rec_l;
		const u64 cnt = n + 1 - last;
		if (total) {
			if (count_bytes == 4)
				((u32 *)counts)[total - 1] = (u32)cnt;
			else
				((u64 *)counts)[total - 1] = cnt;
		}
	}
}

}  // namespace rsx
