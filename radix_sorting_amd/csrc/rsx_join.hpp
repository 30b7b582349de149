// rsx_join.hpp -- the kernels of rsx_sort_join_device and rsx_join_pairs_device: the matching rows of two key columns (README.md
// "Counting sort": the prefix sums of the RIGHT keys' counts are every left row's range into the sorted right side).  The
// arithmetic is rsx_join_shape.hpp's.
//
//   rsx_join_probe_kernel      the table route's one read of the left keys: a key that differs from the right keys in a bit that
//                              does not vary among them matches nothing; every other key's packed value reads two neighbouring
//                              offsets of the right keys' count table.  A workgroup ends by storing the sum of its counts and the
//                              number of its rows without a match
//   rsx_join_scatter_kernel    the merge route: start / count found in the order of the sorted left keys go back through the left
//                              permutation
//   rsx_join_rowsums_kernel    the pairs of every tile of JOIN_ROW_TILE rows ...
//   rsx_join_scan_kernel       ... scanned by one workgroup: excl[0 .. T], excl[T] = the number of pairs
//   rsx_join_expand_kernel     the expansion, one workgroup per output tile of JOIN_EXPAND_TILE consecutive pairs: a binary search
//                              of `excl` finds the row tile of the tile's first pair, the row tile's counts are scanned in LDS,
//                              every thread finds the row of its pair positions by a search of that scan and writes
//                              out_left / out_right as consecutive elements across the wave
//
// No kernel here adds to device memory atomically, none waits for another workgroup (no look-back chain, no spin), and nothing
// depends on the lane order of a returning LDS atomic: there is no LDS atomic.  What a workgroup of the expansion costs depends
// on its output tile alone -- 4096 pairs and the row tiles they touch -- never on how the pairs are spread over the rows.
#pragma once

#include "rsx_join_shape.hpp"
#include "rsx_rankdata.hpp"

namespace rsx {

// the sum of `v` over the workgroup (JOIN_THREADS or 1024 threads), valid in every thread
template <u32 THREADS> __device__ __forceinline__ u64 join_block_sum(u64 v, u64 *s_w)
{
	constexpr u32 WAVES = THREADS / 64;
	const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const u64 incl = unique_wave_incl_sum<u64>(v, lane);
	__syncthreads();   // (s_w may still be read from the call before)
	if (lane == 63u)
		s_w[wave] = incl;
	__syncthreads();
	u64 sum = 0;
#pragma unroll
	for (u32 w = 0; w < WAVES; ++w)
		sum += s_w[w];
	return sum;
}

// start[i] = offs[p], count[i] = offs[p + 1] - offs[p] for p = pack(k), k = kdf(left[i]), where (k & ~vary) == (kdf(right[0]) &
// ~vary); else count[i] = 0 (and start[i] = 0).  Each output may be nullptr.  The keys are read and the results written as in
// rsx_rankdata_lookup_kernel: a workgroup owns a contiguous share of the 16-byte vectors, workgroup 0 the elements before the
// first boundary and behind the last whole vector.  parts[2 b] = the sum of workgroup b's counts, parts[2 b + 1] = the number of
// its rows with count 0.
//   IN_LDS: `offs` are the 257 exclusive offsets of one-byte keys, copied into LDS; else the 65537 of rsx_rankdata_scan16_kernel,
//   read from device memory.
template <typename KT, typename IT, bool IN_LDS>
__global__ __launch_bounds__(1024) void rsx_join_probe_kernel(const KT *__restrict__ left, u64 n, KdfArgs<KT> ka, BitRuns runs, KT vary,
                                                              const KT *__restrict__ right, const u64 *__restrict__ offs,
                                                              IT *__restrict__ start, IT *__restrict__ count, u64 *__restrict__ parts)
{
	__shared__ u64 s_offs[IN_LDS ? 257 : 1];
	__shared__ u64 s_w[16];
	const u32 tid = threadIdx.x;
	if (IN_LDS) {
		if (tid < 257u)
			s_offs[tid] = offs[tid];
		__syncthreads();
	}
	const KT fixed = (KT)(kdf_apply(right[0], ka) & (KT)~vary);
	u64 sum = 0, zeros = 0;
	auto look = [&](const KT raw, IT &lo, IT &cnt) {
		const KT k = kdf_apply(raw, ka);
		const u32 p = unique_pack<KT>(k, runs);
		const u64 a = IN_LDS ? s_offs[p] : offs[p], b = IN_LDS ? s_offs[p + 1u] : offs[p + 1u];
		const bool hit = (KT)(k & (KT)~vary) == fixed;
		const u64 c = hit ? b - a : 0;
		lo = (IT)(hit ? a : 0);
		cnt = (IT)c;
		sum += c;
		zeros += c ? 0u : 1u;
	};
	constexpr u32 V = 16 / sizeof(KT);
	constexpr u32 C = V < 4 ? V : 4;   // keys looked up and stored together
	constexpr u32 OV = C * sizeof(IT) >= 16 ? 16 / sizeof(IT) : C;
	typedef KT kvec_t __attribute__((ext_vector_type(V)));
	u64 head = ((16u - (u32)((uintptr_t)left & 15u)) & 15u) / sizeof(KT);
	if (head > n)
		head = n;
	const u64 nvec = (n - head) / V;
	const kvec_t *vsrc = (const kvec_t *)(left + head);
	const bool start_ok = (((uintptr_t)(start + head)) & (OV * sizeof(IT) - 1u)) == 0;
	const bool count_ok = (((uintptr_t)(count + head)) & (OV * sizeof(IT) - 1u)) == 0;
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
					if (start)
						rankdata_store<IT, C>(start + at + s, a, start_ok);
					if (count)
						rankdata_store<IT, C>(count + at + s, c, count_ok);
				}
			}
	}
	if (blockIdx.x == 0) {
		auto one = [&](u64 i) {
			IT a, c;
			look(left[i], a, c);
			if (start)
				start[i] = a;
			if (count)
				count[i] = c;
		};
		if (tid < head)
			one(tid);
		const u64 t0 = head + nvec * V;
		if (t0 + tid < n)
			one(t0 + tid);
	}
	const u64 wg_sum = join_block_sum<1024>(sum, s_w), wg_zeros = join_block_sum<1024>(zeros, s_w);
	if (tid == 0) {
		parts[2u * blockIdx.x] = wg_sum;
		parts[2u * blockIdx.x + 1u] = wg_zeros;
	}
}

// start[perm[j]] = sorted_start[j], count[perm[j]] = sorted_count[j]: what the search found for the j-th of the SORTED left keys
// belongs to the row that key came from.  Each output may be nullptr.
template <typename IT>
__global__ __launch_bounds__(256) void rsx_join_scatter_kernel(const IT *__restrict__ perm, u64 n, const IT *__restrict__ sorted_start,
                                                               const IT *__restrict__ sorted_count, IT *__restrict__ start,
                                                               IT *__restrict__ count)
{
	const u64 stride = (u64)gridDim.x * 256u;
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < n; j += stride) {
		const u64 i = (u64)perm[j];
		if (start)
			start[i] = sorted_start[j];
		if (count)
			count[i] = sorted_count[j];
	}
}

// excl[t] = the pairs of the rows [t * JOIN_ROW_TILE, (t + 1) * JOIN_ROW_TILE) (join_row_pairs), not yet scanned
template <typename IT>
__global__ __launch_bounds__(JOIN_THREADS) void rsx_join_rowsums_kernel(const IT *__restrict__ count, u64 n, u32 left, u64 *__restrict__ excl)
{
	__shared__ u64 s_w[JOIN_THREADS / 64];
	const u64 T = join_tiles(n, JOIN_ROW_TILE);
	for (u64 t = blockIdx.x; t < T; t += gridDim.x) {
		u64 sum = 0;
#pragma unroll
		for (u32 j = 0; j < JOIN_ROW_TILE / JOIN_THREADS; ++j) {
			const u64 i = t * JOIN_ROW_TILE + j * JOIN_THREADS + threadIdx.x;
			if (i < n)
				sum += join_row_pairs((u64)count[i], left != 0);
		}
		const u64 total = join_block_sum<JOIN_THREADS>(sum, s_w);
		if (threadIdx.x == 0)
			excl[t] = total;
	}
}

// excl[0 .. T) (sums) -> their exclusive scan in place, excl[T] = the total.  One workgroup; thread x owns the entries
// [x * per, (x + 1) * per).
__global__ __launch_bounds__(1024) void rsx_join_scan_kernel(u64 *__restrict__ excl, u64 T)
{
	__shared__ u64 s_part[1024];
	const u32 tid = threadIdx.x;
	const u64 per = (T + 1023u) / 1024u;
	const u64 lo = (u64)tid * per < T ? (u64)tid * per : T, hi = lo + per < T ? lo + per : T;
	u64 sum = 0;
	for (u64 t = lo; t < hi; ++t)
		sum += excl[t];
	s_part[tid] = sum;
	__syncthreads();
	for (u32 off = 1; off < 1024; off <<= 1) {
		const u64 add = tid >= off ? s_part[tid - off] : 0;
		__syncthreads();
		s_part[tid] += add;
		__syncthreads();
	}
	u64 run = s_part[tid] - sum;
	for (u64 t = lo; t < hi; ++t) {
		const u64 own = excl[t];
		excl[t] = run;
		run += own;
	}
	if (tid == 1023u)
		excl[T] = s_part[1023];
}

// The expansion.  Workgroup b writes the output tiles b, b + gridDim.x, ...; the output tile o is the pairs [o * JOIN_EXPAND_TILE,
// min((o + 1) * JOIN_EXPAND_TILE, n_pairs)), written segment by segment (join_segment: the part of it inside one row tile).  For a
// segment the row tile's pairs per row are scanned into s_incl (thread x owns JOIN_ROW_TILE / JOIN_THREADS neighbouring rows);
// pair q of the segment then belongs to row r = join_find_row(q - first), is that row's t-th (t = what is left of q - first
// behind the rows before r), and
//   out_left[q] = i, out_right[q] = perm[start[i] + t]      for i = tile * JOIN_ROW_TILE + r;
// a row without a match (one pair under `left`, else none) gets out_right = all ones, and so does a position at or behind m, which
// arrays as rsx_sort_join_device writes them never name.  Lanes take consecutive q.  Each output may be nullptr.
template <typename IT>
__global__ __launch_bounds__(JOIN_THREADS) void rsx_join_expand_kernel(const IT *__restrict__ start, const IT *__restrict__ count,
                                                                       const IT *__restrict__ perm, u64 n, u64 m, u32 left,
                                                                       const u64 *__restrict__ excl, u64 n_pairs, IT *__restrict__ out_left,
                                                                       IT *__restrict__ out_right)
{
	constexpr u32 RPT = JOIN_ROW_TILE / JOIN_THREADS, WAVES = JOIN_THREADS / 64;
	__shared__ u64 s_incl[JOIN_ROW_TILE];
	__shared__ u64 s_w[WAVES];
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u64 T = join_tiles(n, JOIN_ROW_TILE), out_tiles = join_tiles(n_pairs, JOIN_EXPAND_TILE);
	for (u64 o = blockIdx.x; o < out_tiles; o += gridDim.x) {
		const u64 p0 = o * JOIN_EXPAND_TILE, p1 = p0 + JOIN_EXPAND_TILE < n_pairs ? p0 + JOIN_EXPAND_TILE : n_pairs;
		u64 p = p0;
		while (p < p1) {
			const JoinSegment seg = join_segment(excl, T, p, p1);
			const u64 row0 = seg.tile * JOIN_ROW_TILE;
			const u32 rows = (u32)(n - row0 < JOIN_ROW_TILE ? n - row0 : (u64)JOIN_ROW_TILE);
			u64 c[RPT], sum = 0;
#pragma unroll
			for (u32 j = 0; j < RPT; ++j) {
				const u32 r = tid * RPT + j;
				c[j] = r < rows ? join_row_pairs((u64)count[row0 + r], left != 0) : 0;
				sum += c[j];
			}
			const u64 incl = unique_wave_incl_sum<u64>(sum, lane);
			if (lane == 63u)
				s_w[wave] = incl;
			__syncthreads();
			u64 run = incl - sum;
#pragma unroll
			for (u32 w = 0; w < WAVES; ++w)
				run += w < wave ? s_w[w] : 0;
#pragma unroll
			for (u32 j = 0; j < RPT; ++j) {
				run += c[j];
				s_incl[tid * RPT + j] = run;
			}
			__syncthreads();
			for (u64 q = p + tid; q < seg.end; q += JOIN_THREADS) {
				const u64 rel = q - seg.first;
				const u32 r = join_find_row(s_incl, rows, rel);
				const u64 before = r ? s_incl[r - 1u] : 0;
				const u64 i = row0 + r;
				if (out_left)
					out_left[q] = (IT)i;
				if (out_right) {
					IT v = (IT)~(IT)0;
					// (a row's single pair under `left` may stand for no match: its count says which)
					if (!left || s_incl[r] - before > 1u || count[i] != 0) {
						const u64 at = (u64)start[i] + (rel - before);
						if (at < m)
							v = perm[at];
					}
					out_right[q] = v;
				}
			}
			p = seg.end;
			__syncthreads();   // (s_incl and s_w are written again for the next segment)
		}
	}
}

}  // namespace rsx
