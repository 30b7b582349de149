// rsx_lex.hpp -- the one kernel of rsx_sort_lex_device: the keys of one GROUP of columns derived, packed and (from the second
// group on) gathered through the permutation found so far.
//
// An ordering by several columns is the reference's own argument one level up: "this is only possible because the sort is
// stable" makes one LSD pass per byte column a sort, and one stable sort per key column -- least significant first -- an
// ORDER BY.  The host (rsx.hip, sort_lex_device) groups neighbouring columns whose widths add up to at most the packing limit;
// this kernel turns a group into ONE unsigned key per row,
//
//     key[i] = kdf_a(col_a[r]) << shift_a | kdf_b(col_b[r]) << shift_b | ...      r = i (pack form) or perm[i] (gather form)
//
// with the group's most significant column in the highest bits used and every unused high byte zero, so that the ordinary
// ascending sort of OT orders the rows by the tuple (and skips the unused bytes as constant columns).
//
//   pack form    a thread takes four consecutive rows per grid-stride step: one vector load of 4 x width bytes per column (4, 8,
//                16 or 2 x 16 bytes) where the column's base is aligned to that (LexCol::vec, decided on the host: the caller's
//                pointers are only element-aligned), four element loads otherwise; one vector store of 4 x sizeof(OT)
//   gather form  the permutation quad is one vector load (two for 8-byte indices) where its base is 16-byte aligned
//                (LexArgs::perm_vec); the column elements are single loads at perm[i].  Element-granular gathers are uncoalesced
//                by nature: that is the price of an LSD ordering by several columns, not something this kernel can remove.
//
// Bounds: whole quads cover rows 0 .. 4 * (n / 4) - 1; the last n % 4 rows are taken element by element by the first threads
// of workgroup 0.  Every index read from `perm` is below n because the inner sorts produce permutations of 0 .. n-1.  `out` is
// the library's buffer (256-byte aligned, n keys); no store goes past row n - 1.
//
// The column descriptors travel by value in the kernel arguments and are indexed by a wave-uniform loop counter only: scalar
// loads, no scratch.
#pragma once

#include "rsx_kernels.hpp"

namespace rsx {

enum : u32 { LEX_THREADS = 256, LEX_GROUP_COLS = 8, LEX_MAX_GRID = 4096 };

struct LexCol {
	const void *p;
	u32 wlog2;               // log2 of the element width in bytes
	u32 shift;               // bit position of this column in the packed key
	u32 vec;                 // pack form: the base is aligned to 4 x width, a quad is one vector load
	u32 pad;
	u64 fmask, sflip, desc;  // KdfArgs of the column's type, zero-extended
};
struct LexArgs {
	LexCol col[LEX_GROUP_COLS];
	u32 ncols;
	u32 perm_vec;            // gather form: `perm` is 16-byte aligned
};

template <typename KT> __device__ __forceinline__ u64 lex_kdf(KT raw, const LexCol &d)
{
	return (u64)kdf_apply<KT>(raw, KdfArgs<KT>{(KT)d.fmask, (KT)d.sflip, (KT)d.desc});
}

// the derived keys of rows i0 .. i0 + 3 of one column (all four rows exist)
__device__ __forceinline__ void lex_quad(const LexCol &d, u64 i0, u64 (&k)[4])
{
	switch (d.wlog2) {
	case 0: {
		const uint8_t *p = (const uint8_t *)d.p + i0;
		u32 w;
		if (d.vec)
			w = *(const u32 *)p;
		else
			w = (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
#pragma unroll
		for (u32 j = 0; j < 4; ++j)
			k[j] = lex_kdf<uint8_t>((uint8_t)(w >> (8 * j)), d);
		break;
	}
	case 1: {
		const uint16_t *p = (const uint16_t *)d.p + i0;
		u32x2 w;
		if (d.vec) {
			w = *(const u32x2 *)p;
		} else {
			w.x = (u32)p[0] | ((u32)p[1] << 16);
			w.y = (u32)p[2] | ((u32)p[3] << 16);
		}
		k[0] = lex_kdf<uint16_t>((uint16_t)w.x, d);
		k[1] = lex_kdf<uint16_t>((uint16_t)(w.x >> 16), d);
		k[2] = lex_kdf<uint16_t>((uint16_t)w.y, d);
		k[3] = lex_kdf<uint16_t>((uint16_t)(w.y >> 16), d);
		break;
	}
	case 2: {
		const u32 *p = (const u32 *)d.p + i0;
		u32x4 w;
		if (d.vec) {
			w = *(const u32x4 *)p;
		} else {
			w.x = p[0];
			w.y = p[1];
			w.z = p[2];
			w.w = p[3];
		}
		k[0] = lex_kdf<u32>(w.x, d);
		k[1] = lex_kdf<u32>(w.y, d);
		k[2] = lex_kdf<u32>(w.z, d);
		k[3] = lex_kdf<u32>(w.w, d);
		break;
	}
	default: {
		const u64 *p = (const u64 *)d.p + i0;
		u64 x[4];
		if (d.vec) {
			const u32x4 a = *(const u32x4 *)p, b = *(const u32x4 *)(p + 2);
			x[0] = (u64)a.x | ((u64)a.y << 32);
			x[1] = (u64)a.z | ((u64)a.w << 32);
			x[2] = (u64)b.x | ((u64)b.y << 32);
			x[3] = (u64)b.z | ((u64)b.w << 32);
		} else {
#pragma unroll
			for (u32 j = 0; j < 4; ++j)
				x[j] = p[j];
		}
#pragma unroll
		for (u32 j = 0; j < 4; ++j)
			k[j] = lex_kdf<u64>(x[j], d);
		break;
	}
	}
}

// the derived key of row r of one column
__device__ __forceinline__ u64 lex_one(const LexCol &d, u64 r)
{
	switch (d.wlog2) {
	case 0: return lex_kdf<uint8_t>(((const uint8_t *)d.p)[r], d);
	case 1: return lex_kdf<uint16_t>(((const uint16_t *)d.p)[r], d);
	case 2: return lex_kdf<u32>(((const u32 *)d.p)[r], d);
	default: return lex_kdf<u64>(((const u64 *)d.p)[r], d);
	}
}

// four packed keys to out[i0 .. i0 + 3]: one store of 4 x sizeof(OT) bytes (two 16-byte ones for 8-byte keys)
template <typename OT> __device__ __forceinline__ void lex_store_quad(OT *out, u64 i0, const u64 (&key)[4])
{
	if constexpr (sizeof(OT) == 2) {
		u32x2 v;
		v.x = (u32)key[0] | ((u32)key[1] << 16);
		v.y = (u32)key[2] | ((u32)key[3] << 16);
		*(u32x2 *)(out + i0) = v;
	} else if constexpr (sizeof(OT) == 4) {
		u32x4 v;
		v.x = (u32)key[0];
		v.y = (u32)key[1];
		v.z = (u32)key[2];
		v.w = (u32)key[3];
		*(u32x4 *)(out + i0) = v;
	} else {
		u32x4 a, b;
		a.x = (u32)key[0];
		a.y = (u32)(key[0] >> 32);
		a.z = (u32)key[1];
		a.w = (u32)(key[1] >> 32);
		b.x = (u32)key[2];
		b.y = (u32)(key[2] >> 32);
		b.z = (u32)key[3];
		b.w = (u32)(key[3] >> 32);
		*(u32x4 *)(out + i0) = a;
		*(u32x4 *)(out + i0 + 2) = b;
	}
}

template <typename IT> __device__ __forceinline__ void lex_perm_quad(const IT *perm, u64 i0, bool vec, u64 (&r)[4])
{
	if (!vec) {
#pragma unroll
		for (u32 j = 0; j < 4; ++j)
			r[j] = (u64)perm[i0 + j];
	} else if constexpr (sizeof(IT) == 4) {
		const u32x4 v = *(const u32x4 *)(perm + i0);
		r[0] = v.x;
		r[1] = v.y;
		r[2] = v.z;
		r[3] = v.w;
	} else {
		const u32x4 a = *(const u32x4 *)(perm + i0), b = *(const u32x4 *)(perm + i0 + 2);
		r[0] = (u64)a.x | ((u64)a.y << 32);
		r[1] = (u64)a.z | ((u64)a.w << 32);
		r[2] = (u64)b.x | ((u64)b.y << 32);
		r[3] = (u64)b.z | ((u64)b.w << 32);
	}
}

// out[i] = the packed key of row i (GATHER: of row perm[i]), i < n.  OT: u16 / u32 / u64, the smallest that holds the group.
template <typename OT, typename IT, bool GATHER>
__global__ __launch_bounds__(LEX_THREADS) void rsx_lex_pack_kernel(const LexArgs a, const IT *__restrict__ perm, OT *__restrict__ out, u64 n)
{
	const u64 quads = n / 4;
	const u64 stride = (u64)gridDim.x * LEX_THREADS;
	for (u64 q = (u64)blockIdx.x * LEX_THREADS + threadIdx.x; q < quads; q += stride) {
		const u64 i0 = 4 * q;
		u64 key[4] = {0, 0, 0, 0};
		u64 r[4] = {i0, i0 + 1, i0 + 2, i0 + 3};
		if constexpr (GATHER)
			lex_perm_quad<IT>(perm, i0, a.perm_vec != 0, r);
		for (u32 c = 0; c < a.ncols; ++c) {   // (wave-uniform: the descriptor comes by scalar loads)
			const LexCol d = a.col[c];
			u64 k[4];
			if constexpr (GATHER) {
#pragma unroll
				for (u32 j = 0; j < 4; ++j)
					k[j] = lex_one(d, r[j]);
			} else {
				lex_quad(d, i0, k);
			}
#pragma unroll
			for (u32 j = 0; j < 4; ++j)
				key[j] |= k[j] << d.shift;
		}
		lex_store_quad<OT>(out, i0, key);
	}
	// the last n % 4 rows, element by element
	const u64 i = 4 * quads + threadIdx.x;
	if (blockIdx.x == 0 && i < n) {
		const u64 r = GATHER ? (u64)perm[i] : i;
		u64 key = 0;
		for (u32 c = 0; c < a.ncols; ++c) {
			const LexCol d = a.col[c];
			key |= lex_one(d, r) << d.shift;
		}
		out[i] = (OT)key;
	}
}

}  // namespace rsx
