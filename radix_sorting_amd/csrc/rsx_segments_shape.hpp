// rsx_segments_shape.hpp: the arithmetic of rsx_sort_segments*'s LDS route (rsx_segments.hpp) -- the size classes of
// the segments, the longest segment a class and the route take (`cap`), the LDS a launch of a class declares, its grid, and the
// shares of the plan kernels.  Nothing of HIP and nothing of Ctx is used here: every function is __host__ __device__ under hipcc
// and plain C++ otherwise; tests/cpp/segments_shape_check.cpp includes this file alone and checks it on the CPU, and
// tests/segments_lib.py restates it.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RSX_SEGMENTS_HD __host__ __device__ inline
#else
#define RSX_SEGMENTS_HD inline
#endif

namespace rsx {

typedef unsigned long long u64;
typedef unsigned int u32;

// A TEAM of waves sorts one segment in LDS.  The classes, by the length of a segment:
//   COPY   0 .. 1           nothing to sort: a segment of one key is copied by one thread, an empty one is not even listed
//   WAVE   2 .. 256         a team is ONE wave; a workgroup of 256 threads holds four teams, each with LDS of its own
//   GROUP  257 .. 2048      a team is a workgroup of 256 threads
//   BLOCK  2049 .. cap      a team is a workgroup of 1024 threads; the launch declares the LDS its LONGEST segment needs, at most all
//                           160 KiB of a CU
//   LONG   cap + 1 ..       does not fit LDS: another route's
enum : u32 { SEGMENTS_COPY = 0, SEGMENTS_WAVE = 1, SEGMENTS_GROUP = 2, SEGMENTS_BLOCK = 3, SEGMENTS_LONG = 4, SEGMENTS_CLASSES = 5 };
enum : u32 { SEGMENTS_COPY_MAX = 1, SEGMENTS_WAVE_MAX = 256, SEGMENTS_GROUP_MAX = 2048 };
enum : u32 { SEGMENTS_LDS_BYTES = 163840, SEGMENTS_TEAM_FIXED = 256, SEGMENTS_IDX_BYTES = 2, SEGMENTS_CAP_STEP = 256 };
// the plan kernels: a workgroup of SEGMENTS_PLAN_THREADS threads owns a contiguous share of whole tiles of as many segments
enum : u32 { SEGMENTS_PLAN_THREADS = 256, SEGMENTS_PLAN_MAX_WGS = 256, SEGMENTS_MAX_LONG_LISTED = 4096 };

// the waves of a team, the teams and the threads of a workgroup of a class (COPY: one thread per segment)
RSX_SEGMENTS_HD u32 segments_team_waves(u32 cls) { return cls == SEGMENTS_WAVE ? 1u : cls == SEGMENTS_GROUP ? 4u : cls == SEGMENTS_BLOCK ? 16u : 0u; }
RSX_SEGMENTS_HD u32 segments_wg_teams(u32 cls) { return cls == SEGMENTS_WAVE ? 4u : cls == SEGMENTS_COPY ? 256u : 1u; }
RSX_SEGMENTS_HD u32 segments_wg_threads(u32 cls) { return cls == SEGMENTS_BLOCK ? 1024u : 256u; }

// What a team keeps in LDS: one row of 256 digit cells per wave, SEGMENTS_TEAM_FIXED bytes of words the waves exchange, and two
// buffers of `stride` elements -- a key and, where indices are wanted, its position in the segment as a u16 (SEGMENTS_IDX_BYTES:
// cap never exceeds 65536 where indices travel).  `with_idx`: out_idx is wanted (with or without out_keys: the keys travel anyway).
RSX_SEGMENTS_HD u32 segments_elem_bytes(u32 key_bytes, bool with_idx) { return key_bytes + (with_idx ? (u32)SEGMENTS_IDX_BYTES : 0u); }
RSX_SEGMENTS_HD u32 segments_team_bytes(u32 waves, u32 key_bytes, bool with_idx, u32 stride)
{
	return waves * 1024u + SEGMENTS_TEAM_FIXED + 2u * stride * segments_elem_bytes(key_bytes, with_idx);
}

// cap: the longest segment the LDS route takes -- what fits a BLOCK team's LDS, in steps of SEGMENTS_CAP_STEP, at most 65536
RSX_SEGMENTS_HD u32 segments_cap(u32 key_bytes, bool with_idx)
{
	const u32 room = SEGMENTS_LDS_BYTES - 16u * 1024u - SEGMENTS_TEAM_FIXED;
	u32 cap = room / (2u * segments_elem_bytes(key_bytes, with_idx)) / SEGMENTS_CAP_STEP * SEGMENTS_CAP_STEP;
	return cap > 65536u ? 65536u : cap;
}

// the class of a segment of `len` keys
RSX_SEGMENTS_HD u32 segments_class(u64 len, u32 cap)
{
	return len <= SEGMENTS_COPY_MAX ? (u32)SEGMENTS_COPY
	     : len > cap ? (u32)SEGMENTS_LONG
	     : len <= SEGMENTS_WAVE_MAX ? (u32)SEGMENTS_WAVE
	     : len <= SEGMENTS_GROUP_MAX ? (u32)SEGMENTS_GROUP : (u32)SEGMENTS_BLOCK;
}

// the elements of a team's buffers in a launch of class `cls` whose longest segment has max_len keys (WAVE, GROUP: the class's
// own longest; BLOCK: max_len rounded up to SEGMENTS_CAP_STEP, so that shorter segments leave room for a second workgroup on the CU)
RSX_SEGMENTS_HD u32 segments_stride(u32 cls, u64 max_len, u32 cap)
{
	if (cls == SEGMENTS_WAVE)
		return SEGMENTS_WAVE_MAX < cap ? (u32)SEGMENTS_WAVE_MAX : cap;
	if (cls == SEGMENTS_GROUP)
		return SEGMENTS_GROUP_MAX < cap ? (u32)SEGMENTS_GROUP_MAX : cap;
	if (cls != SEGMENTS_BLOCK)
		return 0;
	const u64 up = (max_len + SEGMENTS_CAP_STEP - 1u) / SEGMENTS_CAP_STEP * SEGMENTS_CAP_STEP;
	return up > cap ? cap : (u32)up;
}
// the LDS bytes a workgroup of the class declares
RSX_SEGMENTS_HD u32 segments_lds_bytes(u32 cls, u32 key_bytes, bool with_idx, u64 max_len)
{
	const u32 waves = segments_team_waves(cls);
	if (!waves)
		return 0;
	return segments_wg_teams(cls) * segments_team_bytes(waves, key_bytes, with_idx, segments_stride(cls, max_len, segments_cap(key_bytes, with_idx)));
}
// the workgroups of a launch over the `count` listed segments of a class: one team each
RSX_SEGMENTS_HD u64 segments_grid(u32 cls, u64 count)
{
	const u32 teams = segments_wg_teams(cls);
	return (count + teams - 1u) / teams;
}

// ---- the plan kernels' shares: workgroup w owns the segments [w * share, (w + 1) * share) below m, share a multiple of the tile ----
struct SegmentsPlanGrid {
	u64 share;   // segments per workgroup
	u32 wgs;
};
RSX_SEGMENTS_HD SegmentsPlanGrid segments_plan_grid(u64 m)
{
	SegmentsPlanGrid g;
	const u64 tiles = (m + SEGMENTS_PLAN_THREADS - 1u) / SEGMENTS_PLAN_THREADS;
	const u64 per = (tiles + SEGMENTS_PLAN_MAX_WGS - 1u) / SEGMENTS_PLAN_MAX_WGS;
	g.share = (per ? per : 1u) * SEGMENTS_PLAN_THREADS;
	const u64 wgs = (m + g.share - 1u) / g.share;
	g.wgs = (u32)(wgs ? wgs : 1u);
	return g;
}

// the narrowest unsigned type that holds the segment numbers 0 .. m - 1 (the composed route's id column): its bytes
RSX_SEGMENTS_HD u32 segments_id_bytes(u64 m) { return m <= 256u ? 1u : m <= 65536u ? 2u : 4u; }

}  // namespace rsx
