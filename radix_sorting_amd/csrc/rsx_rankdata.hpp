// rsx_rankdata.hpp -- the kernels of rsx_sort_rankdata_device: for every element its place in the stable sorted order (the
// inverse of rsx_sort_rank's permutation), the number of elements with a smaller derived key and the number with an equal one
// (README.md "Counting sort": the prefix sums of the counts ARE the ranks -- read per key instead of used for a scatter).
//
//   rsx_rankdata_lookup_kernel    less / equal of every key from a table of exclusive offsets: one kept column's 256 (copied
//                                 into LDS), or the 65537 of the packed varying bits (read from device memory: 512 KiB, L2)
//   rsx_rankdata_digits_kernel    one kept column, the place, launch 1 of 3: the 256 digit counts of a workgroup's share
//   rsx_rankdata_bases_kernel     ... 2 of 3: the workgroups x 256 counts scanned by digit across the workgroups, on top of the
//                                 column's offsets: where each workgroup's first element of each digit stands
//   rsx_rankdata_place_kernel     ... 3 of 3: the share walked again, place = running base of the digit + elements of the same
//                                 digit earlier in the round -- what a counting sort's scatter would use as the address
//   rsx_rankdata_count16_kernel   rsx_joint16_kernel's scheme on the packed varying bits of keys of any width
//   rsx_rankdata_scan16_kernel    rsx_joint16_scan_kernel without its gate on the plan of a 2-byte sort
//   rsx_rankdata_runs_kernel      the sort route: over the sorted keys, the positions of the heads and the stable permutation,
//                                 place / less / equal of a run [s, e) scattered through the permutation
//   rsx_rankdata_inverse_kernel   the sort route, place alone: place[perm[j]] = j
//   rsx_rankdata_fill_kernel      every key equal: equal = n
//
// The three launches of the place are ordinary ones: no workgroup waits for another (no look-back chain, no spin), and the
// order of equal digits inside a round comes from ballots -- never from the value a returning LDS atomic hands back, whose
// lane order is not a documented guarantee on gfx950 (rsx_scatter2.hpp) and would here BE the result.
#pragma once

#include "rsx_group.hpp"

namespace rsx {

// the place of one kept column: a round is one key per thread, a tile the rounds whose keys are loaded together, a share (what
// one workgroup owns) a whole number of tiles, and there are at most RANKDATA_PLACE_MAX_WGS shares
enum : u32 { RANKDATA_PLACE_THREADS = 256, RANKDATA_PLACE_ROUNDS = 8, RANKDATA_PLACE_TILE = RANKDATA_PLACE_THREADS * RANKDATA_PLACE_ROUNDS,
             RANKDATA_PLACE_MAX_WGS = 1024 };

// `o[0 .. V)` = g, as whole vectors of at most 16 bytes where the caller found `o` aligned for them
template <typename IT, u32 V> __device__ __forceinline__ void rankdata_store(IT *__restrict__ o, const IT (&g)[V], bool vec_ok)
{
	constexpr u32 OV = V * sizeof(IT) >= 16 ? 16 / sizeof(IT) : V;   // elements of one store
	typedef IT ovec_t __attribute__((ext_vector_type(OV)));
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

// less[i] = offs[p], equal[i] = offs[p + 1] - offs[p] for p = pack(kdf(src[i])); each output may be nullptr.  The keys are
// read and the results written as in rsx_group_lookup_kernel: a workgroup owns a contiguous share of the 16-byte vectors,
// workgroup 0 the elements before the first boundary and behind the last whole vector.
//   IN_LDS: `offs` are the 256 exclusive offsets of one kept column (the last bin ends at n), copied into LDS;
//   else: the 65537 of rsx_rankdata_scan16_kernel, read from device memory.
template <typename KT, typename IT, bool IN_LDS>
__global__ __launch_bounds__(1024) void rsx_rankdata_lookup_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, BitRuns runs,
                                                                   const u64 *__restrict__ offs, IT *__restrict__ less,
                                                                   IT *__restrict__ equal)
{
	__shared__ u64 s_offs[IN_LDS ? 257 : 1];
	const u32 tid = threadIdx.x;
	if (IN_LDS) {
		if (tid < 256u)
			s_offs[tid] = offs[tid];
		if (tid == 256u)
			s_offs[256] = n;
		__syncthreads();
	}
	auto look = [&](const KT raw, IT &lo, IT &cnt) {
		const u32 p = unique_pack<KT>(kdf_apply(raw, ka), runs);
		const u64 a = IN_LDS ? s_offs[p] : offs[p], b = IN_LDS ? s_offs[p + 1u] : offs[p + 1u];
		lo = (IT)a;
		cnt = (IT)(b - a);
	};
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 C = V < 4 ? V : 4;   // keys looked up and stored together (a vector of 1-byte keys at once would spill)
	constexpr u32 OV = C * sizeof(IT) >= 16 ? 16 / sizeof(IT) : C;
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	u64 head = ((16u - (u32)((uintptr_t)src & 15u)) & 15u) / sizeof(KT);
	if (head > n)
		head = n;
	const u64 nvec = (n - head) / V;
	const kvec_t *vsrc = (const kvec_t *)(src + head);
	const bool less_ok = (((uintptr_t)(less + head)) & (OV * sizeof(IT) - 1u)) == 0;
	const bool equal_ok = (((uintptr_t)(equal + head)) & (OV * sizeof(IT) - 1u)) == 0;
	const u64 per = (nvec + gridDim.x - 1) / gridDim.x;
	const u64 lo = (u64)blockIdx.x * per, hi = lo + per < nvec ? lo + per : nvec;
	constexpr u32 U = 2;
	for (u64 v = lo + tid; v < hi; v += 1024u * U) {
		kvec_t x[U];
#pragma unroll
		for (u32 u = 0; u < U; ++u)
			if (v + u * 1024u < hi)
				x[u] = vsrc[v + u * 1024u];
#pragma unroll
		for (u32 u = 0; u < U; ++u)
			if (v + u * 1024u < hi) {
				const u64 at = head + (v + u * 1024u) * V;
#pragma unroll
				for (u32 s = 0; s < V; s += C) {
					IT a[C], c[C];
#pragma unroll
					for (u32 e = 0; e < C; ++e)
						look(x[u][s + e], a[e], c[e]);
					if (less)
						rankdata_store<IT, C>(less + at + s, a, less_ok);
					if (equal)
						rankdata_store<IT, C>(equal + at + s, c, equal_ok);
				}
			}
	}
	if (blockIdx.x == 0) {
		auto one = [&](u64 i) {
			IT a, c;
			look(src[i], a, c);
			if (less)
				less[i] = a;
			if (equal)
				equal[i] = c;
		};
		if (tid < head)
			one(tid);
		const u64 t0 = head + nvec * V;
		if (t0 + tid < n)
			one(t0 + tid);
	}
}

// Workgroup w owns the keys [w * share, min((w + 1) * share, n)); tab[w * 256 + d] = how many of them have digit d of the
// kept column (bits shift .. shift + 7 of the derived key).  The counters are LDS atomics whose return value nobody reads.
// (A share holds fewer than 2^32 keys: n / RANKDATA_PLACE_MAX_WGS, rounded up to a tile.)
template <typename KT>
__global__ __launch_bounds__(RANKDATA_PLACE_THREADS) void rsx_rankdata_digits_kernel(const KT *__restrict__ src, u64 n, u64 share, u32 shift,
                                                                                     KdfArgs<KT> ka, u64 *__restrict__ tab)
{
	__shared__ u32 s_cnt[256];
	const u32 tid = threadIdx.x;
	s_cnt[tid] = 0;
	__syncthreads();
	const u64 lo = (u64)blockIdx.x * share, hi = lo + share < n ? lo + share : n;
	for (u64 t0 = lo; t0 < hi; t0 += RANKDATA_PLACE_TILE) {
		KT k[RANKDATA_PLACE_ROUNDS];
#pragma unroll
		for (u32 r = 0; r < RANKDATA_PLACE_ROUNDS; ++r) {
			const u64 i = t0 + r * RANKDATA_PLACE_THREADS + tid;
			k[r] = i < hi ? src[i] : (KT)0;
		}
#pragma unroll
		for (u32 r = 0; r < RANKDATA_PLACE_ROUNDS; ++r)
			if (t0 + r * RANKDATA_PLACE_THREADS + tid < hi)
				atomicAdd(&s_cnt[(u32)(kdf_apply(k[r], ka) >> shift) & 0xFFu], 1u);
	}
	__syncthreads();
	tab[(u64)blockIdx.x * 256u + tid] = s_cnt[tid];
}

// tab[w * 256 + d] (counts) -> offs[d] + the counts of digit d in the workgroups before w: one workgroup, thread (q, d) scans
// a quarter of the workgroups for digit d (the loads of 256 threads with neighbouring d are one contiguous row).
__global__ __launch_bounds__(1024) void rsx_rankdata_bases_kernel(u64 *__restrict__ tab, u32 wgs, const u64 *__restrict__ offs)
{
	__shared__ u64 s_part[4][256];
	const u32 tid = threadIdx.x, d = tid & 255u, q = tid >> 8;
	const u32 per = (wgs + 3u) / 4u;
	const u32 w0 = q * per < wgs ? q * per : wgs, w1 = w0 + per < wgs ? w0 + per : wgs;
	u64 sum = 0;
#pragma unroll 8
	for (u32 w = w0; w < w1; ++w)
		sum += tab[(u64)w * 256u + d];
	s_part[q][d] = sum;
	__syncthreads();
	u64 run = offs[d];
	for (u32 p = 0; p < q; ++p)
		run += s_part[p][d];
#pragma unroll 8
	for (u32 w = w0; w < w1; ++w) {
		const u64 t = tab[(u64)w * 256u + d];
		tab[(u64)w * 256u + d] = run;
		run += t;
	}
}

// place[i] = the position element i takes in a stable counting sort by the kept column.  The workgroup's 256 running bases
// (tab row of the workgroup, rsx_rankdata_bases_kernel) are in LDS; a round is the 256 consecutive keys i = t0 + tid, in which
// the elements of digit d before lane l of wave w are the whole counts of d in the waves before w (s_wcnt, written by the first
// lane of each digit of each wave) plus the lanes of w below l with the same digit (eight ballots).  Two barriers per round:
// the counts of round r + 1 go to the other set, which thread d cleared for digit d when it advanced base[d] in round r - 1.
// Loads and stores are consecutive elements across a wave; a tile's keys are loaded before its first round.
template <typename KT, typename IT>
__global__ __launch_bounds__(RANKDATA_PLACE_THREADS) void rsx_rankdata_place_kernel(const KT *__restrict__ src, u64 n, u64 share, u32 shift,
                                                                                    KdfArgs<KT> ka, const u64 *__restrict__ tab,
                                                                                    IT *__restrict__ place)
{
	constexpr u32 WAVES = RANKDATA_PLACE_THREADS / 64;
	__shared__ u64 s_base[256];
	__shared__ u32 s_wcnt[2][WAVES][256];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	s_base[tid] = tab[(u64)blockIdx.x * 256u + tid];
#pragma unroll
	for (u32 w = 0; w < WAVES; ++w) {
		s_wcnt[0][w][tid] = 0;
		s_wcnt[1][w][tid] = 0;
	}
	__syncthreads();
	const u64 below = ((u64)1 << lane) - 1u;
	const u64 lo = (u64)blockIdx.x * share, hi = lo + share < n ? lo + share : n;
	u32 set = 0;
	for (u64 t0 = lo; t0 < hi; t0 += RANKDATA_PLACE_TILE) {
		KT k[RANKDATA_PLACE_ROUNDS];
#pragma unroll
		for (u32 r = 0; r < RANKDATA_PLACE_ROUNDS; ++r) {
			const u64 i = t0 + r * RANKDATA_PLACE_THREADS + tid;
			k[r] = i < hi ? src[i] : (KT)0;
		}
#pragma unroll
		for (u32 r = 0; r < RANKDATA_PLACE_ROUNDS; ++r) {
			const u64 i = t0 + r * RANKDATA_PLACE_THREADS + tid;
			const bool valid = i < hi;
			const u32 d = (u32)(kdf_apply(k[r], ka) >> shift) & 0xFFu;
			u64 m = __ballot(valid);
#pragma unroll
			for (u32 b = 0; b < 8u; ++b) {
				const bool bit = (d >> b) & 1u;
				const u64 bal = __ballot(bit);
				m &= bit ? bal : ~bal;
			}
			const u32 rank = (u32)__popcll(m & below);
			if (valid && rank == 0)
				s_wcnt[set][wave][d] = (u32)__popcll(m);
			__syncthreads();
			u32 total = 0;   // of digit `tid` in this round
#pragma unroll
			for (u32 w = 0; w < WAVES; ++w)
				total += s_wcnt[set][w][tid];
			if (valid) {
				u64 p = s_base[d] + rank;
				for (u32 w = 0; w < wave; ++w)
					p += s_wcnt[set][w][d];
				place[i] = (IT)p;
			}
			__syncthreads();
			if (total) {
				s_base[tid] += total;
#pragma unroll
				for (u32 w = 0; w < WAVES; ++w)
					s_wcnt[set][w][tid] = 0;
			}
			set ^= 1u;
		}
	}
}

// rsx_joint16_kernel on p = pack(kdf(key)) < 2^16 for keys of any width: a workgroup counts the half of the 65536 bins its
// parity names (p with bit 15 clear / set) in 128 KiB of LDS -- one workgroup per CU -- and skips the other keys; workgroups b
// and b + 8 read the same keys.  One global add per non-empty bin per workgroup.  joint: 65536 counts, zero on entry; fewer
// than 2^32 keys.
template <typename KT>
__global__ __launch_bounds__(1024) void rsx_rankdata_count16_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka, BitRuns runs,
                                                                    u32 *__restrict__ joint)
{
	__shared__ u32 tab[32768];
	const u32 tid = threadIdx.x, half = (blockIdx.x >> 3) & 1u, slot = (blockIdx.x & 7u) | ((blockIdx.x >> 4) << 3),
	          nslots = gridDim.x >> 1;
	for (u32 i = tid; i < 32768u; i += 1024u)
		tab[i] = 0;
	__syncthreads();
	constexpr u32 V = 16 / sizeof(KT);
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	const u64 nvec = n / V;
	const bool aligned = (((uintptr_t)src) & 15) == 0;
	auto count = [&](const KT raw) {
		const u32 p = unique_pack<KT>(kdf_apply(raw, ka), runs);
		if ((p >> 15) == half)
			atomicAdd(&tab[p & 0x7FFFu], 1u);
	};
	if (aligned) {
		for (u64 v = (u64)slot * 1024u + tid; v < nvec; v += (u64)nslots * 1024u) {
			const kvec_t x = *(const kvec_t *)(src + v * V);
#pragma unroll
			for (u32 e = 0; e < V; ++e)
				count(x[e]);
		}
		for (u64 i = nvec * V + (u64)slot * 1024u + tid; i < n; i += (u64)nslots * 1024u)
			count(src[i]);
	} else {
		for (u64 i = (u64)slot * 1024u + tid; i < n; i += (u64)nslots * 1024u)
			count(src[i]);
	}
	__syncthreads();
	for (u32 i = tid; i < 32768u; i += 1024u)
		if (tab[i])
			atomicAdd(&joint[half * 32768u + i], tab[i]);
}

// joint[65536] counts -> offs[65537] exclusive offsets, offs[65536] = n (rsx_joint16_scan_kernel's scan; that kernel does
// nothing unless the device-side plan is a 2-byte sort's with both columns kept, which the keys here need not be)
__global__ __launch_bounds__(1024) void rsx_rankdata_scan16_kernel(const u32 *__restrict__ joint, u64 *__restrict__ offs, u64 n)
{
	__shared__ u64 part[1024];
	const u32 tid = threadIdx.x;
	const u32x4 *j4 = (const u32x4 *)joint + tid * 16;   // this thread's 64 bins
	u64 sum = 0;
#pragma unroll 4
	for (u32 j = 0; j < 16; ++j) {
		const u32x4 v = j4[j];
		sum += (u64)v.x + v.y + v.z + v.w;
	}
	part[tid] = sum;
	__syncthreads();
	for (u32 off = 1; off < 1024; off <<= 1) {
		const u64 add = tid >= off ? part[tid - off] : 0;
		__syncthreads();
		part[tid] += add;
		__syncthreads();
	}
	u64 run = part[tid] - sum;
	u64 *o = offs + tid * 64;
#pragma unroll 4
	for (u32 j = 0; j < 16; ++j) {
		const u32x4 v = j4[j];
		o[4 * j] = run;
		o[4 * j + 1] = run + v.x;
		o[4 * j + 2] = run + v.x + v.y;
		o[4 * j + 3] = run + v.x + v.y + v.z;
		run += (u64)v.x + v.y + v.z + v.w;
	}
	if (tid == 1023)
		offs[65536] = n;
}

// The sort route's last pass over the sorted keys `in` and the stable permutation `perm` that sorted them (nullptr: the
// identity), tiled as rsx_group_heads_kernel (recs: heads before the tile, from rsx_unique_heads_kernel<KT, 0> and the scan).
// start[g] is the position of head g (rsx_group_heads_kernel's `first` over the identity), *total the number of heads G.  The
// element at sorted position j of run g = [start[g], start[g + 1]) -- the last run ends at n: there is no start[G] --
//   place[perm[j]] = j, less[perm[j]] = start[g], equal[perm[j]] = the run's length; each output may be nullptr.
// A thread looks the run up at its first element and again behind every head among its elements; a run that spans tiles is
// the same two loads in each of them.
template <typename KT, typename IT>
__global__ __launch_bounds__(UNIQUE_HEADS_THREADS) void rsx_rankdata_runs_kernel(const KT *__restrict__ in, const IT *__restrict__ perm, u64 n,
                                                                                 const UniqueRec *__restrict__ recs,
                                                                                 const IT *__restrict__ start, const u64 *__restrict__ total,
                                                                                 IT *__restrict__ place, IT *__restrict__ less,
                                                                                 IT *__restrict__ equal)
{
	constexpr u32 V = 16 / sizeof(KT);
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const bool aligned = ((uintptr_t)in & 15u) == 0;
	const u64 base = (u64)blockIdx.x * unique_heads_tile<KT>();
	constexpr u32 WAVES = UNIQUE_HEADS_THREADS / 64;
	__shared__ u32 s_c[WAVES];
	u32 carry_c = 0;
	const u64 rec_c = recs[blockIdx.x].cnt, groups = total[0];
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
		const u32 incl_c = unique_wave_incl_sum<u32>(c, lane);
		if (lane == 63u)
			s_c[wave] = incl_c;
		__syncthreads();
		u32 wb_c = 0, tot_c = 0;
#pragma unroll
		for (u32 w = 0; w < WAVES; ++w) {
			const u32 sc = s_c[w];
			wb_c += w < wave ? sc : 0u;
			tot_c += sc;
		}
		if (i0 < n) {
			// heads before this lane's elements: at least one once the first element (a head: element 0 is one) is counted
			u64 heads = rec_c + carry_c + wb_c + incl_c - c;
			u64 s = 0, len = 0;
			bool have = false;
#pragma unroll
			for (u32 e = 0; e < V; ++e) {
				const u64 i = i0 + e;
				if (i < n) {
					if (f >> e & 1u) {
						++heads;
						have = false;
					}
					if (!have) {
						const u64 g = heads - 1u;
						s = (u64)start[g];
						len = (g + 1u < groups ? (u64)start[g + 1u] : n) - s;
						have = true;
					}
					const IT at = perm ? perm[i] : (IT)i;
					if (place)
						place[at] = (IT)i;
					if (less)
						less[at] = (IT)s;
					if (equal)
						equal[at] = (IT)len;
				}
			}
		}
		carry_c += tot_c;
		__syncthreads();
	}
}

// place[perm[j]] = j: the permutation of a stable argsort inverted
template <typename IT> __global__ __launch_bounds__(256) void rsx_rankdata_inverse_kernel(const IT *__restrict__ perm, u64 n, IT *__restrict__ place)
{
	const u64 stride = (u64)gridDim.x * 256u;
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < n; j += stride)
		place[perm[j]] = (IT)j;
}

template <typename IT> __global__ __launch_bounds__(256) void rsx_rankdata_fill_kernel(IT *__restrict__ dst, u64 n, IT value)
{
	const u64 stride = (u64)gridDim.x * 256u;
	for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += stride)
		dst[i] = value;
}

}  // namespace rsx
