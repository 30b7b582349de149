// segments_shape_check.cpp -- the arithmetic of rsx_sort_segments*'s LDS route (radix_sorting_amd/csrc/rsx_segments_shape.hpp) on
// the CPU: every class's LDS fits a CU, cap is monotone in the key width, every length lands in exactly one class, a class's grid
// covers its list, the plan kernels' shares cover the segments.  No GPU and no library: the header alone.
// Built by `make cpp`, run by tests/test_segments_shape_cpu.py (which reads the printed table too).
// Prints one "cap <key bytes> <with idx> <cap> <lds of a full BLOCK>" line per shape, "segments_shape_check OK" and returns 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../radix_sorting_amd/csrc/rsx_segments_shape.hpp"

using namespace rsx;

static int failures = 0;
#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			if (failures < 20)                                              \
				std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			++failures;                                                     \
		}                                                                   \
	} while (0)

// the one class whose range of lengths holds len, from the ranges as the header's comment states them
static u32 class_by_ranges(u64 len, u32 cap, int *hits)
{
	const u64 lo[SEGMENTS_CLASSES] = {0, 2, 257, 2049, (u64)cap + 1};
	const u64 hi[SEGMENTS_CLASSES] = {1, 256, 2048, cap, ~(u64)0};
	u32 cls = 0;
	*hits = 0;
	for (u32 c = 0; c < SEGMENTS_CLASSES; ++c)
		if (len >= lo[c] && len <= hi[c]) {
			cls = c;
			++*hits;
		}
	return cls;
}

static void check_shape(u32 kb, bool with_idx)
{
	const u32 cap = segments_cap(kb, with_idx);
	CHECK(cap > SEGMENTS_GROUP_MAX && cap <= 65536 && cap % SEGMENTS_CAP_STEP == 0);
	if (with_idx)
		CHECK(cap <= 65536);   // positions travel as u16
	for (u64 len = 0; len <= (u64)cap + 1; ++len) {
		int hits = 0;
		const u32 want = class_by_ranges(len, cap, &hits);
		CHECK(hits == 1);
		const u32 cls = segments_class(len, cap);
		CHECK(cls == want);
		if (cls >= SEGMENTS_WAVE && cls <= SEGMENTS_BLOCK) {
			// the segment fits its team's buffers, and the launch whose longest segment it is fits a CU
			CHECK(segments_stride(cls, len, cap) >= len);
			CHECK(segments_stride(cls, cap, cap) >= len);
			const u32 lds = segments_lds_bytes(cls, kb, with_idx, len);
			CHECK(lds > 0 && lds <= SEGMENTS_LDS_BYTES && lds % 16 == 0);
			CHECK(lds == segments_wg_teams(cls) * segments_team_bytes(segments_team_waves(cls), kb, with_idx, segments_stride(cls, len, cap)));
			CHECK(segments_team_waves(cls) * 64 * segments_wg_teams(cls) == segments_wg_threads(cls));
		} else {
			CHECK(segments_lds_bytes(cls, kb, with_idx, len) == 0);
		}
	}
	CHECK(segments_class((u64)1 << 40, cap) == SEGMENTS_LONG);
	// one step more would not fit
	CHECK(segments_team_bytes(16, kb, with_idx, cap + SEGMENTS_CAP_STEP) > SEGMENTS_LDS_BYTES || cap == 65536);
	for (u32 cls = 0; cls < SEGMENTS_CLASSES; ++cls)
		CHECK(segments_lds_bytes(cls, kb, with_idx, cap) <= SEGMENTS_LDS_BYTES);
	std::printf("cap %u %d %u %u\n", kb, with_idx ? 1 : 0, cap, segments_lds_bytes(SEGMENTS_BLOCK, kb, with_idx, cap));
}

static void check_grids()
{
	for (u32 cls = SEGMENTS_COPY; cls <= SEGMENTS_BLOCK; ++cls)
		for (u64 count : {(u64)0, (u64)1, (u64)3, (u64)4, (u64)5, (u64)255, (u64)256, (u64)257, (u64)1000003, ((u64)1 << 32) + 1}) {
			const u64 g = segments_grid(cls, count), teams = segments_wg_teams(cls);
			CHECK(g * teams >= count);                     // covers the list
			CHECK(count == 0 ? g == 0 : (g - 1) * teams < count);   // ... with no workgroup to spare
		}
	for (u64 m : {(u64)1, (u64)2, (u64)255, (u64)256, (u64)257, (u64)65535, (u64)65536, (u64)65537, (u64)1000003, (u64)0xFFFFFFFEull}) {
		const SegmentsPlanGrid g = segments_plan_grid(m);
		CHECK(g.wgs >= 1 && g.wgs <= SEGMENTS_PLAN_MAX_WGS && g.share % SEGMENTS_PLAN_THREADS == 0);
		CHECK((u64)g.wgs * g.share >= m && (u64)(g.wgs - 1) * g.share < m);
	}
	CHECK(segments_id_bytes(1) == 1 && segments_id_bytes(256) == 1 && segments_id_bytes(257) == 2 && segments_id_bytes(65536) == 2 &&
	      segments_id_bytes(65537) == 4);
}

int main()
{
	for (bool with_idx : {false, true}) {
		u32 before = ~0u;
		for (u32 kb : {1u, 2u, 4u, 8u}) {
			check_shape(kb, with_idx);
			CHECK(segments_cap(kb, with_idx) <= before);   // monotone in the key width
			before = segments_cap(kb, with_idx);
		}
	}
	for (u32 kb : {1u, 2u, 4u, 8u})
		CHECK(segments_cap(kb, true) <= segments_cap(kb, false));
	check_grids();
	CHECK(SEGMENTS_COPY_MAX < SEGMENTS_WAVE_MAX && SEGMENTS_WAVE_MAX < SEGMENTS_GROUP_MAX && SEGMENTS_LDS_BYTES == 160 * 1024);
	if (failures) {
		std::printf("segments_shape_check: %d FAILED\n", failures);
		return 1;
	}
	std::printf("segments_shape_check OK\n");
	return 0;
}
