// rsx_group.hpp -- the kernels of rsx_sort_group_device: for every key the index of its group among the distinct keys in
// order of kdf(key) -- the inverse of rsx_sort_unique -- and optionally the distinct keys, how many of each and where
// each occurs first (README.md "Uniquely sorting with bitmaps" taken one step further: a rank directory over the bitmap).
//
// Where few bits of the derived keys vary, rsx_unique_mark_kernel's bitmap says which packed values occur; the number of
// set bits below a key's bit IS its group.  One 8-byte cell per bitmap word holds the word and the set bits below it, so
// the group of a key costs one load and one popcount:
//
//   rsx_group_cells_kernel    cells[w] = {bitmap[w], set bits below word w} (after the scan of the per-chunk counts)
//   rsx_group_table_kernel    the same from one kept column's 256 scanned counts (no key is read for it), with the
//                             groups' keys and counts read off the table
//   rsx_group_lookup_kernel   every key's group, the cells in LDS (2^16 or 2^18 bits' worth) or in device memory
//   rsx_group_heads_kernel    the sort route: over the sorted keys and the stable permutation that sorted them, the
//                             running count of head flags is the group -- scattered through the permutation; keys, counts
//                             and first indices are written at the heads
#pragma once

#include "rsx_unique.hpp"

namespace rsx {

// a word of the bitmap and the number of set bits in all words before it
struct __attribute__((aligned(8))) GroupCell {
	u32 bits;
	u32 below;
};

// A chunk of UNIQUE_CHUNK_WORDS words (four per thread) per workgroup, as rsx_unique_expand_kernel reads it; recs[chunk].cnt
// is the number of set bits before the chunk (rsx_unique_scan_kernel).
__global__ __launch_bounds__(256) void rsx_group_cells_kernel(const u32 *__restrict__ bitmap, const UniqueRec *__restrict__ recs,
                                                              GroupCell *__restrict__ cells)
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
	u32 below = (u32)recs[blockIdx.x].cnt + incl - c;
	for (u32 w = 0; w < wave; ++w)
		below += s_w[w];
	const u32 words[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
	for (u32 j = 0; j < 4; ++j) {
		cells[w0 + j] = GroupCell{words[j], below};
		below += (u32)__popc(words[j]);
	}
}

// One kept column: bin d of its 256 EXCLUSIVE OFFSETS `offs` (the last bin ends at n) stands for the derived key
// kconst | d << shift, as in rsx_unique_table_kernel.  The eight cells of the 256-bit bitmap of the non-empty bins, the keys
// and counts of those bins (each where wanted), *total = their number.  One workgroup of 256 threads; no key but the first
// is read.
template <typename KT>
__global__ __launch_bounds__(256) void rsx_group_table_kernel(const u64 *__restrict__ offs, u64 n, u32 shift, const KT *__restrict__ src,
                                                              KdfArgs<KT> ka, GroupCell *__restrict__ cells, KT *__restrict__ out_keys,
                                                              void *__restrict__ counts, u32 count_bytes, u64 *__restrict__ total)
{
	const u32 d = threadIdx.x;
	const u64 cd = (d + 1u < 256u ? offs[d + 1u] : n) - offs[d];
	__shared__ u32 s_flag[256];
	__shared__ u32 s_word[8], s_below[9];
	s_flag[d] = cd != 0;
	__syncthreads();
	if (d < 8u) {
		u32 w = 0;
		for (u32 b = 0; b < 32u; ++b)
			w |= s_flag[32u * d + b] << b;
		s_word[d] = w;
	}
	__syncthreads();
	if (d == 0) {
		u32 below = 0;
		for (u32 w = 0; w < 8u; ++w) {
			s_below[w] = below;
			cells[w] = GroupCell{s_word[w], below};
			below += (u32)__popc(s_word[w]);
		}
		s_below[8] = below;
		total[0] = below;
	}
	__syncthreads();
	if (!cd)
		return;
	const u32 o = s_below[d >> 5] + (u32)__popc(s_word[d >> 5] & ((1u << (d & 31u)) - 1u));
	if (out_keys) {
		const KT binmask = (KT)((KT)0xFFu << shift);
		const KT kconst = (KT)(kdf_apply(src[0], ka) & (KT)~binmask);
		out_keys[o] = kdf_invert<KT>((KT)(kconst | (KT)((KT)d << shift)), ka);
	}
	if (counts) {
		if (count_bytes == 4)
			((u32 *)counts)[o] = (u32)cd;
		else
			((u64 *)counts)[o] = cd;
	}
}

// inverse[i] = the number of set bits below bit pack(kdf(src[i])).  A workgroup owns a contiguous share of the keys and reads
// it with 16-byte loads (the elements before the first 16-byte boundary of src and behind the last whole vector are
// workgroup 0's, as in rsx_unique_mark_kernel); the groups of a vector's keys are written as whole vectors of at most 16
// bytes where out_inverse + head is aligned for them, element by element otherwise.
//   LDS_LOG2 = 16 / 18: the first min(ncells, 2^LDS_LOG2 / 32) cells are copied into LDS (16 / 64 KiB) -- the caller takes
//     these only where every packed value lies below 2^LDS_LOG2;
//   LDS_LOG2 = 0: the cells are read from device memory.
template <typename KT, typename IT, u32 LDS_LOG2>
__global__ __launch_bounds__(1024) void rsx_group_lookup_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, BitRuns runs,
                                                                const GroupCell *__restrict__ cells, u32 ncells, IT *__restrict__ inverse)
{
	constexpr u32 LCELLS = LDS_LOG2 ? (1u << LDS_LOG2) / 32u : 1u;
	__shared__ GroupCell s_cells[LCELLS];
	const u32 tid = threadIdx.x;
	if (LDS_LOG2) {
		const u32 m = ncells < LCELLS ? ncells : LCELLS;
		for (u32 i = tid; i < m; i += 1024u)
			s_cells[i] = cells[i];
		__syncthreads();
	}
	auto group_of = [&](const KT raw) -> IT {
		const u32 p = unique_pack<KT>(kdf_apply(raw, ka), runs);
		const GroupCell c = LDS_LOG2 ? s_cells[p >> 5] : cells[p >> 5];
		return (IT)(c.below + (u32)__popc(c.bits & ((1u << (p & 31u)) - 1u)));
	};
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 OV = V * sizeof(IT) >= 16 ? 16 / sizeof(IT) : V;   // elements of one store
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	typedef IT ovec_t __attribute__((ext_vector_type(OV)));
	u64 head = ((16u - (u32)((uintptr_t)src & 15u)) & 15u) / sizeof(KT);
	if (head > n)
		head = n;
	const u64 nvec = (n - head) / V;
	const kvec_t *vsrc = (const kvec_t *)(src + head);
	IT *vout = inverse + head;
	const bool vec_ok = ((uintptr_t)vout & (OV * sizeof(IT) - 1u)) == 0;
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
				IT g[V];
#pragma unroll
				for (u32 e = 0; e < V; ++e)
					g[e] = group_of(x[u][e]);
				IT *o = vout + (v + u * 1024u) * V;
				if (vec_ok) {
#pragma unroll
					for (u32 s = 0; s < V / OV; ++s) {
						ovec_t ov;
#pragma unroll
						for (u32 e = 0; e < OV; ++e)
							ov[e] = g[s * OV + e];
						((ovec_t *)o)[s] = ov;
					}
				} else {
#pragma unroll
					for (u32 e = 0; e < V; ++e)
						o[e] = g[e];
				}
			}
	}
	if (blockIdx.x == 0) {
		if (tid < head)
			inverse[tid] = group_of(src[tid]);
		const u64 t0 = head + nvec * V;
		if (t0 + tid < n)
			inverse[t0 + tid] = group_of(src[t0 + tid]);
	}
}

// The sort route's last pass over the sorted keys `in` and the stable permutation `perm` that sorted them (nullptr: the
// identity -- the input was sorted), tiled as rsx_unique_heads_kernel<KT, 1> (whose PHASE 0 and scan made recs: heads
// before the tile, position + 1 of the last head before it).  Element i's group is the number of heads in [0, i] minus one:
//   inverse[perm[i]] = group (a scatter); and at a head of group g: keys[g] = in[i], first[g] = perm[i] (the sort is stable:
//   the smallest index of the group), counts[g - 1] = i minus the position of the head before -- the last count is the last
//   tile's to write.  Every output may be nullptr.
template <typename KT, typename IT>
__global__ __launch_bounds__(UNIQUE_HEADS_THREADS) void rsx_group_heads_kernel(const KT *__restrict__ in, const IT *__restrict__ perm, u64 n,
                                                                               const UniqueRec *__restrict__ recs, IT *__restrict__ inverse,
                                                                               KT *__restrict__ keys, IT *__restrict__ counts,
                                                                               IT *__restrict__ first)
{
	constexpr u32 V = 16 / sizeof(KT);
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const bool aligned = ((uintptr_t)in & 15u) == 0;
	const u64 base = (u64)blockIdx.x * unique_heads_tile<KT>();
	constexpr u32 WAVES = UNIQUE_HEADS_THREADS / 64;
	__shared__ u32 s_c[WAVES], s_l[WAVES];
	u32 carry_c = 0, carry_l = 0;
	const u64 rec_c = recs[blockIdx.x].cnt, rec_l = recs[blockIdx.x].last;
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
		if (i0 < n) {
			// heads before this lane's elements; the first element of the array is a head, so `before` + the heads up to an
			// element is at least one
			const u64 before = rec_c + carry_c + wb_c + incl_c - c;
			u64 pl = plr ? base + plr : rec_l;
#pragma unroll
			for (u32 e = 0; e < V; ++e) {
				const u64 i = i0 + e;
				if (i < n) {
					const u64 g = before + (u32)__popc(f & ((2u << e) - 1u)) - 1u;
					const IT src_i = perm ? perm[i] : (IT)i;
					if (inverse)
						inverse[src_i] = (IT)g;
					if (f >> e & 1u) {
						if (keys)
							keys[g] = x[e];
						if (first)
							first[g] = src_i;
						if (counts && g)
							counts[g - 1] = (IT)(i + 1 - pl);
						pl = i + 1;
					}
				}
			}
		}
		carry_c += tot_c;
		carry_l = tot_l > carry_l ? tot_l : carry_l;
		__syncthreads();
	}
	if (counts && blockIdx.x == gridDim.x - 1 && tid == 0) {
		const u64 total = rec_c + carry_c, last = carry_l ? base + carry_l : rec_l;
		if (total)
			counts[total - 1] = (IT)(n + 1 - last);
	}
}

}  // namespace rsx
