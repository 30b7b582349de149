// rsx_keybits.hpp: the host arithmetic over the varying bits of the keys that rsx_sort_unique*, rsx_sort_group* and
// rsx_sort_rankdata* share -- the runs of the mask (BitRuns, a kernel argument), the shape of the bitmap over the packed values and
// the grid of a sweep over the keys.  Included by rsx_kernels.hpp.  Nothing of HIP and nothing of Ctx is used here:
// tests/cpp/keybits_check.cpp includes this file alone and checks it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rsx {

typedef unsigned long long u64;
typedef unsigned int u32;

// README.md:716-758 "key compaction": the varying bits of a KDF key packed together (a software bit extract over at most 8 runs
// of contiguous mask bits).  All other bits are the same in every key, so the packed values order exactly as the keys do.
struct BitRuns {
	uint8_t n;            // runs
	uint8_t src[8];       // first bit of the run in the key
	uint8_t len[8];       // bits
	uint8_t dst[8];       // first bit of the run in the packed value
};

// the runs of contiguous set bits of `mask`, lowest first, packed towards bit 0; false if there are more than eight
inline bool bit_runs(u64 mask, BitRuns *out)
{
	out->n = 0;
	u32 dst = 0;
	for (u32 b = 0; b < 64;) {
		if (!((mask >> b) & 1)) {
			++b;
			continue;
		}
		u32 e = b;
		while (e < 64 && ((mask >> e) & 1))
			++e;
		if (out->n == 8)
			return false;
		out->src[out->n] = (uint8_t)b;
		out->len[out->n] = (uint8_t)(e - b);
		out->dst[out->n] = (uint8_t)dst;
		dst += e - b;
		++out->n;
		b = e;
	}
	return true;
}

// one kept column: the byte `col` of the key is the packed value
inline BitRuns column_runs(u32 col)
{
	BitRuns runs{};
	runs.n = 1;
	runs.src[0] = (uint8_t)(8 * col);
	runs.len[0] = 8;
	runs.dst[0] = 0;
	return runs;
}

// The bitmap over packed values below 2^vbits: a multiple of the read-out's chunk (UNIQUE_CHUNK_WORDS, rsx_unique.hpp).  The mark
// kernel keeps a bitmap of 2^16, 2^18 or 2^20 bits in LDS (`lds_bits`; 0: it sets the bits in device memory).  Two workgroups of
// 1024 threads fill a CU (2048 threads; 2 x 8 or 2 x 32 KiB of its 160 KiB of LDS); the 128 KiB form leaves room for one.
constexpr u32 KEYBITS_CHUNK_WORDS = 1024;
struct BitmapShape {
	u64 words;      // 32 bits each
	u64 chunks;     // the grid of the read-out and the records of its scan
	size_t bytes;
	u32 lds_bits;   // 16, 18, 20 or 0
	u32 full;       // the largest grid of the mark kernel
};
inline BitmapShape bitmap_shape(u32 vbits)
{
	BitmapShape s;
	s.words = ((u64)1 << vbits) / 32 > KEYBITS_CHUNK_WORDS ? ((u64)1 << vbits) / 32 : KEYBITS_CHUNK_WORDS;
	s.chunks = s.words / KEYBITS_CHUNK_WORDS;
	s.bytes = (size_t)s.words * sizeof(u32);
	s.lds_bits = vbits <= 16 ? 16u : vbits <= 18 ? 18u : vbits <= 20 ? 20u : 0u;
	s.full = s.lds_bits == 20 ? 256u : 512u;
	return s;
}

// The grid of a sweep of workgroups of 1024 threads over n keys read as 16-byte vectors: a workgroup should have a few sweeps of
// its own (16 vectors per thread) to pay for zeroing and merging -- or copying -- its table in LDS.
inline unsigned sweep_grid(u64 n, size_t key_bytes, u32 full = 512)
{
	const u64 nvec = n * key_bytes / 16;
	const u64 wgs = nvec / 16384;
	return (unsigned)(wgs < 1 ? 1 : wgs > full ? full : wgs);
}

}  // namespace rsx
