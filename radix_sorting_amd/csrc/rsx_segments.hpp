// rsx_segments.hpp -- the kernels of rsx_sort_segments_device: many independent arrays (CSR style segments of one key array) sorted
// in one call.  The classes, caps, LDS sizes and grids are rsx_segments_shape.hpp's.
//
//   rsx_segments_plan_kernel<IT, PLACE = false>  the count: a workgroup owns a contiguous share of the segment numbers, checks its
//                                 offsets (non-decreasing, offsets[0] == 0, offsets[m] == n) and stores one row: the segments of every
//                                 class, the longest segment, whether an offset was bad
//   rsx_segments_scan_kernel      one workgroup: class-major over the rows -- where every (class, share) starts in the list --, the
//                                 totals, and the plan record, also into the context's pinned memory
//   rsx_segments_plan_kernel<IT, PLACE = true>   the placement: the same shares again; every segment number goes to its class's part
//                                 of the list, in ascending order (ballots inside a wave, the waves' counts summed in LDS); the first
//                                 SEGMENTS_MAX_LONG_LISTED long segments also leave (start, length) for the host's loop
//   rsx_segments_copy_kernel      class COPY: segments of one key
//   rsx_segments_sort_kernel<KT, IDX, NW>  classes WAVE (NW = 1, four teams to a workgroup), GROUP (4) and BLOCK (16): a team of NW
//                                 waves loads one segment into LDS, finds which byte columns vary IN THIS SEGMENT and whether it is
//                                 in order already, runs one stable LDS-to-LDS counting pass per varying column and writes the result
//   rsx_segments_ids_kernel       the composed route: the segment number of every key, for rsx_sort_lex_device
//   rsx_segments_gather_kernel    ... and its keys and indices through the permutation
//   rsx_segments_long_kernel      MIXED: one long segment's keys and indices through its rank sort
//
// No kernel here adds to device memory atomically and none waits for another workgroup.  The ranking inside a team is
// rsx_small.hpp's: a wave owns a contiguous slice of the segment, counts its digits into its own row of cells, the rows become run
// starts by a prefix over digits and waves, and a returning LDS atomic on the cell is the key's position -- it rests on returning
// LDS atomics resolving same-address lanes in lane order, which the host verifies before it takes this route (lds_order_selfcheck).
// The byte histograms of rs_sort_main serve two questions only -- does column j vary, is the array in order --, and a segment
// answers the first with the OR of (key XOR first key) over its keys: column j has a single non-empty bin exactly when byte j of
// that OR is zero.  So a team keeps no histogram, and a dozen keys cost no 2 KiB of zeroing per key byte.
#pragma once

#include "rsx_kernels.hpp"
#include "rsx_segments_shape.hpp"

namespace rsx {

// what the plan kernels leave for the host (device memory and, copied by the scan kernel, pinned host memory)
struct SegmentsPlan {
	u64 max_len;                       // the longest segment
	u64 count[SEGMENTS_CLASSES];       // segments per class (COPY: empty ones included)
	u64 listed[SEGMENTS_CLASSES];      // ... of which the list holds this many (COPY: those of one key)
	u64 list_start[SEGMENTS_CLASSES];  // where the class's part of the list starts
	u32 bad;                           // an offset out of order, offsets[0] != 0 or offsets[m] != n
	u32 pad;
};

// where segment s starts: offsets[s], or s * row_len for uniform rows (offsets == nullptr)
template <typename IT> __device__ __forceinline__ u64 segments_start(const IT *__restrict__ offsets, u64 row_len, u64 s)
{
	return offsets ? (u64)offsets[s] : s * row_len;
}

// one row of the count per workgroup: [0 .. 4] listed segments per class, [5] empty segments, [6] longest, [7] bad
enum : u32 { SEGMENTS_ROW = 8 };

template <typename IT, bool PLACE>
__global__ __launch_bounds__(SEGMENTS_PLAN_THREADS) void rsx_segments_plan_kernel(const IT *__restrict__ offsets, u64 m, u64 n, u32 cap,
                                                                                  SegmentsPlanGrid grid, u64 *__restrict__ rows,
                                                                                  const u64 *__restrict__ starts, u32 *__restrict__ list,
                                                                                  u64 *__restrict__ longtab)
{
	constexpr u32 NWV = SEGMENTS_PLAN_THREADS / 64;
	__shared__ u64 wcnt[NWV][SEGMENTS_ROW];
	__shared__ u64 cursor[SEGMENTS_CLASSES];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u64 lo = (u64)blockIdx.x * grid.share, hi = lo + grid.share < m ? lo + grid.share : m;
	u64 cnt[SEGMENTS_CLASSES] = {0, 0, 0, 0, 0}, empty = 0, longest = 0, bad = 0;
	if (PLACE) {
		if (tid < SEGMENTS_CLASSES)
			cursor[tid] = starts[(u64)blockIdx.x * SEGMENTS_ROW + tid];
		__syncthreads();
	}
	for (u64 base = lo; base < hi; base += SEGMENTS_PLAN_THREADS) {
		const u64 s = base + tid;
		const bool have = s < hi;
		u64 a = 0, b = 0;
		if (have) {
			a = (u64)offsets[s];
			b = (u64)offsets[s + 1];
			if (b < a || (s == 0 && a != 0) || (s + 1 == m && b != n))
				bad = 1;
		}
		const u64 len = b >= a ? b - a : 0;
		const u32 cls = have && len > 0 ? segments_class(len, cap) : 0xFFu;   // (0xFF: nothing to list)
		if (have && len == 0)
			++empty;
		if (len > longest)
			longest = len;
		if (!PLACE) {
			if (cls < SEGMENTS_CLASSES)
				++cnt[cls];
			continue;
		}
		// the placement of one tile: inside a wave by ballots, the waves in order behind the workgroup's cursors
		u32 before = 0, mine = 0;
#pragma unroll
		for (u32 c = 0; c < SEGMENTS_CLASSES; ++c) {
			const u64 bal = __ballot(cls == c);
			if (cls == c)
				before = mbcnt64(bal);
			if (lane == c)
				mine = (u32)__popcll(bal);
		}
		if (lane < SEGMENTS_CLASSES)
			wcnt[wave][lane] = mine;
		__syncthreads();
		if (cls < SEGMENTS_CLASSES) {
			u64 at = cursor[cls] + before;
			for (u32 w = 0; w < wave; ++w)
				at += wcnt[w][cls];
			list[at] = (u32)s;
			if (cls == SEGMENTS_LONG) {
				const u64 k = at - starts[(u64)gridDim.x * SEGMENTS_ROW + SEGMENTS_LONG];   // (behind the rows: where every class's part starts)
				if (k < SEGMENTS_MAX_LONG_LISTED) {
					longtab[2 * k] = a;
					longtab[2 * k + 1] = len;
				}
			}
		}
		__syncthreads();
		if (tid < SEGMENTS_CLASSES) {
			u64 add = 0;
			for (u32 w = 0; w < NWV; ++w)
				add += wcnt[w][tid];
			cursor[tid] += add;
		}
		__syncthreads();
	}
	if (PLACE)
		return;
	// the count: summed over the lanes by shuffles, over the waves in LDS
	u64 v[SEGMENTS_ROW] = {cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], empty, longest, bad};
#pragma unroll
	for (u32 j = 0; j < SEGMENTS_ROW; ++j) {
		for (int off = 32; off > 0; off >>= 1) {
			const u64 y = __shfl_xor(v[j], off);
			v[j] = j == 6 ? (y > v[j] ? y : v[j]) : v[j] + y;
		}
		if (lane == 0)
			wcnt[wave][j] = v[j];
	}
	__syncthreads();
	if (tid < SEGMENTS_ROW) {
		u64 r = 0;
		for (u32 w = 0; w < NWV; ++w)
			r = tid == 6 ? (wcnt[w][tid] > r ? wcnt[w][tid] : r) : r + wcnt[w][tid];
		rows[(u64)blockIdx.x * SEGMENTS_ROW + tid] = r;
	}
}

// starts[w][c], and behind the wgs rows one more: where class c's part of the list starts
__global__ __launch_bounds__(64) void rsx_segments_scan_kernel(const u64 *__restrict__ rows, u64 *__restrict__ starts, u32 wgs,
                                                               SegmentsPlan *__restrict__ plan, SegmentsPlan *__restrict__ host_plan)
{
	if (threadIdx.x != 0)
		return;
	SegmentsPlan p;
	p.max_len = 0;
	p.bad = 0;
	p.pad = 0;
	u64 empty = 0, run = 0;
	for (u32 c = 0; c < SEGMENTS_CLASSES; ++c) {
		p.list_start[c] = run;
		starts[(u64)wgs * SEGMENTS_ROW + c] = run;
		for (u32 w = 0; w < wgs; ++w) {
			starts[(u64)w * SEGMENTS_ROW + c] = run;
			run += rows[(u64)w * SEGMENTS_ROW + c];
		}
		p.listed[c] = p.count[c] = run - p.list_start[c];
	}
	for (u32 w = 0; w < wgs; ++w) {
		empty += rows[(u64)w * SEGMENTS_ROW + 5];
		const u64 l = rows[(u64)w * SEGMENTS_ROW + 6];
		p.max_len = l > p.max_len ? l : p.max_len;
		p.bad |= rows[(u64)w * SEGMENTS_ROW + 7] ? 1u : 0u;
	}
	p.count[SEGMENTS_COPY] += empty;
	*plan = p;
	*host_plan = p;
}

// the index an output position gets: the position in the segment, or in the whole array
__device__ __forceinline__ void segments_store_idx(void *__restrict__ out_idx, bool idx64, u64 at, u64 v)
{
	if (idx64)
		((u64 *)out_idx)[at] = v;
	else
		((u32 *)out_idx)[at] = (u32)v;
}

// list == nullptr: the segments 0 .. count - 1 themselves (uniform rows)
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_segments_copy_kernel(const KT *__restrict__ src, const IT *__restrict__ offsets, u64 row_len,
                                                                const u32 *__restrict__ list, u64 count, KT *__restrict__ out_keys,
                                                                void *__restrict__ out_idx, bool idx64, bool local)
{
	const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count)
		return;
	const u64 at = segments_start<IT>(offsets, row_len, list ? (u64)list[i] : i);
	if (out_keys)
		out_keys[at] = src[at];
	if (out_idx)
		segments_store_idx(out_idx, idx64, at, local ? 0 : at);
}

// a team's barrier: the workgroup's where the team is the workgroup; where it is one wave, whose LDS operations complete in order,
// only the compiler is held (the four teams of such a workgroup run loops of different lengths: no workgroup barrier may lie in them)
template <u32 NW> __device__ __forceinline__ void segments_team_barrier()
{
	if constexpr (NW == 1) {
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
	} else {
		__syncthreads();
	}
}

template <typename KT, typename IT, bool IDX, u32 NW>
__global__ __launch_bounds__(NW == 16 ? 1024 : 256) void rsx_segments_sort_kernel(const KT *__restrict__ src, const IT *__restrict__ offsets,
                                                                                  u64 row_len, const u32 *__restrict__ list, u64 count,
                                                                                  KdfArgs<KT> ka, u32 stride, KT *__restrict__ out_keys,
                                                                                  void *__restrict__ out_idx, bool idx64, bool local)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char s_segments[];
	constexpr u32 T = NW * 64u, TEAMS = NW == 1 ? 4u : 1u;
	const u32 tid = threadIdx.x % T, lane = threadIdx.x & 63u, wid = tid >> 6, team = threadIdx.x / T;
	const u64 item = (u64)blockIdx.x * TEAMS + team;
	if (item >= count)   // (a whole team: a wave, or the workgroup)
		return;
	// the team's LDS: [cells NW x 256][words the waves exchange][keys 2 x stride][positions 2 x stride]
	unsigned char *base = s_segments + (size_t)team * segments_team_bytes(NW, (u32)sizeof(KT), IDX, stride);
	u32 *cell = (u32 *)base;
	u64 *wor = (u64 *)(base + NW * 1024u);           // [NW] the waves' ORs
	u32 *wflag = (u32 *)(base + NW * 1024u + 128u);  // [NW] the waves' descents, [16 .. 19] the digit sums of four waves
	KT *kbuf = (KT *)(base + NW * 1024u + SEGMENTS_TEAM_FIXED);
	uint16_t *vbuf = (uint16_t *)(kbuf + 2 * (size_t)stride);

	const u64 seg = list ? (u64)list[item] : item;
	const u64 start = segments_start<IT>(offsets, row_len, seg);
	const u64 len64 = segments_start<IT>(offsets, row_len, seg + 1) - start;   // 2 .. stride: the class's
	if (len64 > stride)   // (never: the plan put the segment into this class by its length; nothing is written past a team's LDS)
		return;
	const u32 len = (u32)len64;

	for (u32 i = tid; i < len; i += T) {
		kbuf[i] = src[start + i];
		if (IDX)
			vbuf[i] = (uint16_t)i;
	}
	segments_team_barrier<NW>();

	// which columns vary, and is the segment in order already (radix_sort.hpp:47-70 on this segment alone)
	const KT k0 = kdf_apply(kbuf[0], ka);
	u64 diff = 0;
	bool descent = false;
	for (u32 i = tid; i < len; i += T) {
		const KT k = kdf_apply(kbuf[i], ka);
		diff |= (u64)(KT)(k ^ k0);
		if (i + 1 < len && k > kdf_apply(kbuf[i + 1], ka))
			descent = true;
	}
	for (int off = 32; off > 0; off >>= 1)
		diff |= __shfl_xor(diff, off);
	descent = __any(descent) != 0;
	if constexpr (NW > 1) {
		if (lane == 0) {
			wor[wid] = diff;
			wflag[wid] = descent ? 1u : 0u;
		}
		__syncthreads();
		diff = 0;
		descent = false;
#pragma unroll
		for (u32 w = 0; w < NW; ++w) {
			diff |= wor[w];
			descent = descent || wflag[w] != 0;
		}
	}

	u32 cur = 0;
	if (descent) {
		// one stable scatter per varying column, LDS to LDS.  Wave w owns [w * per, (w + 1) * per) of the segment (per a multiple of
		// 64); round r of a lane is element w * per + 64 r + lane.
		const u32 per = ((len + T - 1) / T) * 64;
		const u32 wbeg = wid * per, wend = wbeg + per < len ? wbeg + per : len;
		u32 *row = cell + wid * 256u;
		for (u32 col = 0; col < (u32)sizeof(KT); ++col) {
			if (((diff >> (8 * col)) & 0xFFu) == 0)
				continue;
			const u32 shift = 8 * col;
			const KT *kin = kbuf + (size_t)cur * stride;
			KT *kout = kbuf + (size_t)(cur ^ 1u) * stride;
			const uint16_t *vin = vbuf + (size_t)cur * stride;
			uint16_t *vout = vbuf + (size_t)(cur ^ 1u) * stride;
#pragma unroll
			for (int k = 0; k < 4; ++k)
				row[lane + 64 * k] = 0;
			if constexpr (NW == 1)
				segments_team_barrier<NW>();
			// (a wave's DS operations execute in order: no barrier between zeroing and counting its own row)
			for (u32 i = wbeg + lane; i < wend; i += 64)
				atomicAdd(&row[(u32)(kdf_apply(kin[i], ka) >> shift) & 0xFFu], 1u);
			segments_team_barrier<NW>();
			if constexpr (NW == 1) {
				// the exclusive scan over the digits: four neighbouring digits to a lane
				const u32 c0 = row[4 * lane], c1 = row[4 * lane + 1], c2 = row[4 * lane + 2], c3 = row[4 * lane + 3];
				const u32 tot = c0 + c1 + c2 + c3;
				u32 x = tot;
#pragma unroll
				for (int off = 1; off < 64; off <<= 1) {
					const u32 y = __shfl_up(x, off);
					if (lane >= (u32)off)
						x += y;
				}
				const u32 ex = x - tot;
				segments_team_barrier<NW>();
				row[4 * lane] = ex;
				row[4 * lane + 1] = ex + c0;
				row[4 * lane + 2] = ex + c0 + c1;
				row[4 * lane + 3] = ex + c0 + c1 + c2;
			} else {
				u32 tot = 0, incl = 0;
				if (tid < 256) {
#pragma unroll
					for (u32 w = 0; w < NW; ++w)
						tot += cell[w * 256u + tid];
					u32 x = tot;
#pragma unroll
					for (int off = 1; off < 64; off <<= 1) {
						const u32 y = __shfl_up(x, off);
						if (lane >= (u32)off)
							x += y;
					}
					incl = x;
					if (lane == 63)
						wflag[16 + wid] = x;
				}
				__syncthreads();
				if (tid < 256) {
					u32 acc = incl - tot;
					for (u32 w = 0; w < wid; ++w)
						acc += wflag[16 + w];
#pragma unroll
					for (u32 w = 0; w < NW; ++w) {
						const u32 c = cell[w * 256u + tid];
						cell[w * 256u + tid] = acc;
						acc += c;
					}
				}
			}
			segments_team_barrier<NW>();
			for (u32 i = wbeg + lane; i < wend; i += 64) {
				const KT key = kin[i];
				const u32 pos = __hip_atomic_fetch_add(&row[(u32)(kdf_apply(key, ka) >> shift) & 0xFFu], 1u, __ATOMIC_RELAXED,
				                                       __HIP_MEMORY_SCOPE_WORKGROUP);
				kout[pos] = key;
				if (IDX)
					vout[pos] = vin[i];
			}
			segments_team_barrier<NW>();
			cur ^= 1u;
		}
	}
	const KT *kres = kbuf + (size_t)cur * stride;
	const uint16_t *vres = vbuf + (size_t)cur * stride;
	const u64 add = local ? 0 : start;
	for (u32 i = tid; i < len; i += T) {
		if (out_keys)
			out_keys[start + i] = kres[i];
		if (IDX)
			segments_store_idx(out_idx, idx64, start + i, add + vres[i]);
	}
}

// ---- the composed route -------------------------------------------------------------------------------------------------------
// ids[i] = the segment key i lies in: the last s with offsets[s] <= i (empty segments hold no key)
template <typename IT, typename DT>
__global__ __launch_bounds__(256) void rsx_segments_ids_kernel(const IT *__restrict__ offsets, u64 row_len, u64 m, u64 n, DT *__restrict__ ids)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		u64 s;
		if (!offsets) {
			s = i / row_len;
		} else {
			u64 lo = 0, hi = m;   // the first s in 0 .. m with offsets[s] > i, minus one
			while (lo < hi) {
				const u64 mid = (lo + hi) / 2;
				if ((u64)offsets[mid] <= i)
					lo = mid + 1;
				else
					hi = mid;
			}
			s = lo - 1;
		}
		ids[i] = (DT)s;
	}
}

// out position j lies in the segment input position j lies in: ids[j]
template <typename KT, typename IT, typename DT>
__global__ __launch_bounds__(256) void rsx_segments_gather_kernel(const KT *__restrict__ src, const IT *__restrict__ perm, const DT *__restrict__ ids,
                                                                  const IT *__restrict__ offsets, u64 row_len, u64 n, KT *__restrict__ out_keys,
                                                                  IT *__restrict__ out_idx, bool local)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
		const u64 p = (u64)perm[j];
		if (out_keys)
			out_keys[j] = src[p];
		if (out_idx)
			out_idx[j] = (IT)(local ? p - segments_start<IT>(offsets, row_len, (u64)ids[j]) : p);
	}
}

// MIXED: ranks[0 .. len) of the segment at `start` (positions in the segment) -> its keys and indices
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_segments_long_kernel(const KT *__restrict__ src, const IT *__restrict__ ranks, u64 start, u64 len,
                                                                KT *__restrict__ out_keys, IT *__restrict__ out_idx, bool local)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < len; j += stride) {
		const u64 p = (u64)ranks[j];
		if (out_keys)
			out_keys[start + j] = src[start + p];
		if (out_idx)
			out_idx[start + j] = (IT)(local ? p : start + p);
	}
}

}  // namespace rsx
