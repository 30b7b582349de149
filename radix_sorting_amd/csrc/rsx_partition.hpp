// rsx_partition.hpp -- the kernels of rsx_sort_partition_device: the stable multi-way split of the keys by given splitters (README.md
// "Counting sort" with the digit replaced by a search among a few values: count, prefix sum, stable placement).  The edges are
// prepared by rsx_locate.hpp's prepare kernel and searched by rsx_locate_shape.hpp's locate_search, both unchanged; the shares,
// the scan and the read-out of the offsets are rsx_partition_shape.hpp's.
//
//   rsx_partition_pass_kernel<.., PLACE = false>   the count: a workgroup owns a contiguous share of the keys in memory order, searches
//                                 the bin of every key and stores one row of D + 1 counts (every wave counts into its own row
//                                 of LDS cells over the whole share -- no barrier per tile --, the rows are summed at the end)
//   rsx_partition_scan_kernel     bin-major over the rows: the start of every (bin, share), the bin totals and from those the
//                                 caller's m + 2 offsets
//   rsx_partition_pass_kernel<.., PLACE = true>    the placement: the same shares, tile by tile in order.  Per key the bin is searched ONCE
//                                 and kept in a register; the tile is ranked stably by bin, staged in LDS in output order (key,
//                                 position in the tile, bin) and written run by run behind the workgroup's per-bin cursors in LDS;
//                                 the keys of the next tile are requested before this one is ranked
//   (m == 0: out_idx = 0 .. n-1 is rsx_kernels.hpp's rsx_iota_kernel)
//   rsx_partition_gather_kernel   the sort route: keys and indices through the rank sort of the bins
//   rsx_partition_ends_kernel     the sort route: offsets[0] = 0, offsets[m + 1] = n, BELOW: offsets[1 + j] += equal[j]
//
// No kernel here waits for another workgroup and none adds to device memory atomically; no LDS atomic is used either.  A tile is
// ranked inside each wave in one of two forms (FORM, rsx_partition_shape.hpp's partition_rank_form): 1, one ballot and mbcnt per
// bin, the running counts in scalar registers; 2, the lanes of a key's bin found by one ballot per bit of the bin number, the
// running count of the bin in a cell of the wave's own row in LDS, read by all of them and advanced by the lowest of them
// (plain loads and stores: a wave's LDS accesses complete in order, and no other wave touches its row before the barrier).
#pragma once

#include "rsx_partition_shape.hpp"
#include "rsx_locate.hpp"

namespace rsx {

template <typename KT, bool PLACE> struct PartitionLds {
	KT E[PARTITION_MAX_EDGES + 1];
	u32 start[LOCATE_START_ENTRIES + 3];
	u32 wcnt[PARTITION_WAVES][PARTITION_MAX_BINS];   // per wave and bin: the keys of the tile; then those of the waves below
	u32 tot[PARTITION_MAX_BINS];                     // per bin: the keys of the tile
	u32 bstart[PARTITION_MAX_BINS];                  // ... and of the bins below it
	u64 cursor[PLACE ? PARTITION_MAX_BINS : 1];      // per bin: where the workgroup's next key of it goes
	KT keys[PLACE ? PARTITION_TILE : 1];             // the tile in output order
	uint16_t pos[PLACE ? PARTITION_TILE : 1];        // ... the position in the tile each came from
	uint8_t bin[PLACE ? PARTITION_TILE : 1];         // ... and its bin
};

// rows: PLACE = false: out, the counts of this share [wgs][bins]; PLACE = true: in, the starts of this share's keys of every bin.
// Position p of a tile is held by wave p / 512, round (p % 512) / 64, lane p % 64: a wave's rounds read 64 neighbouring keys each.
template <typename KT, typename IT, bool PLACE, u32 FORM>
__global__ __launch_bounds__(PARTITION_THREADS) void rsx_partition_pass_kernel(const KT *__restrict__ src, u64 n, KdfArgs<KT> ka,
                                                                               const KT *__restrict__ gE, const u32 *__restrict__ gstart, u32 D,
                                                                               u32 shift, u32 steps, u32 below, PartitionGrid grid,
                                                                               u64 *__restrict__ rows, KT *__restrict__ out_keys,
                                                                               IT *__restrict__ out_idx)
{
	__shared__ PartitionLds<KT, PLACE> s;
	constexpr u32 KPT = PARTITION_KPT, NONE = 0xFFFFFFFFu;
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, bins = D + 1u;
	const u32 nbits = partition_bin_bits(bins);
	for (u32 i = tid; i < D; i += PARTITION_THREADS)
		s.E[i] = gE[i];
	if (tid < LOCATE_START_ENTRIES)
		s.start[tid] = gstart[tid];
	u64 *const row = rows + (u64)blockIdx.x * bins;
	if (PLACE && tid < bins)
		s.cursor[tid] = row[tid];
	if (!PLACE)   // (the count: a wave's cells add up over the whole share and are summed once, at the end)
		for (u32 i = tid; i < PARTITION_WAVES * PARTITION_MAX_BINS; i += PARTITION_THREADS)
			(&s.wcnt[0][0])[i] = 0;
	__syncthreads();
	const u64 lo = partition_share_lo(grid, blockIdx.x), hi = partition_share_hi(grid, blockIdx.x, n);
	// the keys of a tile are requested one tile ahead: the loads of the next tile are in flight while this one is ranked and written
	KT ahead[KPT];
#pragma unroll
	for (u32 j = 0; j < KPT; ++j) {
		const u64 i = lo + wave * (64u * KPT) + j * 64u + lane;
		ahead[j] = i < hi ? src[i] : (KT)0;
	}
	for (u64 base = lo; base < hi; base += PARTITION_TILE) {
		const u32 cnt = hi - base < PARTITION_TILE ? (u32)(hi - base) : (u32)PARTITION_TILE;
		KT raw[KPT];
		u32 bin[KPT], rank[KPT];
#pragma unroll
		for (u32 j = 0; j < KPT; ++j) {
			raw[j] = ahead[j];
			const u64 i = base + PARTITION_TILE + wave * (64u * KPT) + j * 64u + lane;
			ahead[j] = i < hi ? src[i] : (KT)0;
		}
#pragma unroll
		for (u32 j = 0; j < KPT; ++j) {
			const u32 p = wave * (64u * KPT) + j * 64u + lane;
			u32 eq;
			const u32 b = locate_search<KT, u32>(s.E, D, s.start, shift, steps, kdf_apply(raw[j], ka), &eq);
			bin[j] = p < cnt ? locate_bin_entry(b, eq, below != 0) : NONE;
			rank[j] = 0;
		}
		if (FORM == 1) {
			for (u32 b = 0; b < bins; ++b) {
				u32 c = 0;
#pragma unroll
				for (u32 j = 0; j < KPT; ++j) {
					const u64 bal = __ballot(bin[j] == b);
					if (PLACE && bin[j] == b)
						rank[j] = c + mbcnt64(bal);
					c += (u32)__popcll(bal);
				}
				if (lane == 0)
					s.wcnt[wave][b] = PLACE ? c : s.wcnt[wave][b] + c;
			}
		} else {
			if (PLACE)
				for (u32 b = lane; b < bins; b += 64u)
					s.wcnt[wave][b] = 0;
			__builtin_amdgcn_wave_barrier();
#pragma unroll
			for (u32 j = 0; j < KPT; ++j) {
				const bool valid = bin[j] != NONE;
				u64 peers = __ballot(valid);
				for (u32 bit = 0; bit < nbits; ++bit) {
					const bool one = (bin[j] >> bit & 1u) != 0;
					const u64 bal = __ballot(one);
					peers &= one ? bal : ~bal;
				}
				const u32 before = mbcnt64(peers);
				const u32 cell = valid ? bin[j] : 0u;
				const u32 prev = s.wcnt[wave][cell];
				rank[j] = prev + before;
				__builtin_amdgcn_wave_barrier();
				if (valid && before == 0)
					s.wcnt[wave][cell] = prev + (u32)__popcll(peers);
				__builtin_amdgcn_wave_barrier();
			}
		}
		if (!PLACE)
			continue;
		__syncthreads();
		if (tid < bins) {
			u32 run = 0;
#pragma unroll
			for (u32 w = 0; w < PARTITION_WAVES; ++w) {
				const u32 c = s.wcnt[w][tid];
				s.wcnt[w][tid] = run;
				run += c;
			}
			s.tot[tid] = run;
		}
		if (PLACE) {
			__syncthreads();
			if (wave == 0) {
				// the exclusive scan of the tile's bin totals: four bins per lane
				u32 t[4], sum = 0;
#pragma unroll
				for (u32 e = 0; e < 4u; ++e) {
					t[e] = lane * 4u + e < bins ? s.tot[lane * 4u + e] : 0u;
					sum += t[e];
				}
				u32 incl = sum;
#pragma unroll
				for (u32 off = 1; off < 64u; off <<= 1) {
					const u32 up = __shfl_up(incl, off);
					incl += lane >= off ? up : 0u;
				}
				u32 run = incl - sum;
#pragma unroll
				for (u32 e = 0; e < 4u; ++e) {
					s.bstart[lane * 4u + e] = run;
					run += t[e];
				}
			}
			__syncthreads();
#pragma unroll
			for (u32 j = 0; j < KPT; ++j)
				if (bin[j] != NONE) {
					const u32 q = s.bstart[bin[j]] + s.wcnt[wave][bin[j]] + rank[j];
					if (q < PARTITION_TILE) {
						s.keys[q] = raw[j];
						s.pos[q] = (uint16_t)(wave * (64u * KPT) + j * 64u + lane);
						s.bin[q] = (uint8_t)bin[j];
					}
				}
			__syncthreads();
			for (u32 q = tid; q < cnt; q += PARTITION_THREADS) {
				const u32 b = s.bin[q];
				const u64 at = s.cursor[b] + (q - s.bstart[b]);
				if (at < n) {
					if (out_keys)
						out_keys[at] = s.keys[q];
					if (out_idx)
						out_idx[at] = (IT)(base + s.pos[q]);
				}
			}
			__syncthreads();
			if (tid < bins)
				s.cursor[tid] += s.tot[tid];
		}
		__syncthreads();
	}
	if (!PLACE) {
		__syncthreads();
		if (tid < bins) {
			u64 sum = 0;
#pragma unroll
			for (u32 w = 0; w < PARTITION_WAVES; ++w)
				sum += s.wcnt[w][tid];
			row[tid] = sum;
		}
	}
}

// rows[wgs][bins] -> starts[wgs][bins] (partition_bin_starts) and, where wanted, offsets[0 .. m + 2) (partition_offset_entry); one
// workgroup, thread b < bins owns bin b
template <typename IT>
__global__ __launch_bounds__(1024) void rsx_partition_scan_kernel(const u64 *__restrict__ rows, u64 *__restrict__ starts, u32 wgs, u32 D,
                                                                  const u64 *__restrict__ cum, u64 m, u64 n, IT *__restrict__ offsets)
{
	__shared__ u64 s_incl[PARTITION_MAX_BINS], s_excl[PARTITION_MAX_BINS + 1], s_cum[PARTITION_MAX_BINS];
	const u32 tid = threadIdx.x, bins = D + 1u;
	u64 own = 0;
	if (tid < PARTITION_MAX_BINS) {
		own = tid < bins ? partition_bin_total(rows, wgs, bins, tid) : 0;
		s_incl[tid] = own;
		s_cum[tid] = tid < bins ? cum[tid] : ~(u64)0;
	}
	__syncthreads();
	for (u32 off = 1; off < PARTITION_MAX_BINS; off <<= 1) {
		const u64 add = (tid < PARTITION_MAX_BINS && tid >= off) ? s_incl[tid - off] : 0;
		__syncthreads();
		if (tid < PARTITION_MAX_BINS)
			s_incl[tid] += add;
		__syncthreads();
	}
	if (tid < bins) {
		const u64 base = s_incl[tid] - own;
		s_excl[tid] = base;
		partition_bin_starts(rows, wgs, bins, tid, base, starts);
	}
	if (tid == 0)
		s_excl[bins] = n;
	__syncthreads();
	if (offsets)
		for (u64 j = tid; j < m + 2u; j += 1024u)
			offsets[j] = (IT)s_excl[partition_offset_entry(s_cum, D, j)];
}

// out_keys[j] = src[ranks[j]], out_idx[j] = ranks[j]; each may be nullptr (out_idx may BE ranks)
template <typename KT, typename IT>
__global__ __launch_bounds__(256) void rsx_partition_gather_kernel(const KT *__restrict__ src, const IT *ranks, u64 n, KT *__restrict__ out_keys,
                                                                    IT *out_idx)
{
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < n; j += (u64)gridDim.x * 256u) {
		const IT r = ranks[j];
		if (out_keys)
			out_keys[j] = src[r];
		if (out_idx)
			out_idx[j] = r;
	}
}

// offsets[1 + j] holds `less` of the j-th sorted edge already
template <typename IT>
__global__ __launch_bounds__(256) void rsx_partition_ends_kernel(IT *__restrict__ offsets, const IT *__restrict__ equal, u64 m, u64 n)
{
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < m + 2u; j += (u64)gridDim.x * 256u) {
		if (j == 0)
			offsets[0] = 0;
		else if (j == m + 1u)
			offsets[j] = (IT)n;
		else if (equal)
			offsets[j] += equal[j - 1u];
	}
}

}  // namespace rsx
