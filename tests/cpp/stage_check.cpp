// stage_check: stage_layout (radix_sorting_amd/csrc/rsx_stage.hpp) on the CPU -- where the arrays of a blocking call on host buffers
// lie in the one staging buffer of the context.  Every combination of five arrays, each absent or of 0, 1, 255, 256 or 257 bytes
// (either side of a multiple of the alignment): every slot is 256-aligned, no two slots overlap, an absent array takes no room and
// has no offset, the total is the end of the last slot.  No GPU and no library: the program includes the header alone; exits
// non-zero at the first mismatch.
#include "../../radix_sorting_amd/csrc/rsx_stage.hpp"

#include <cstdio>

#define CHECK(cond, ...)                                 \
	do {                                                 \
		if (!(cond)) {                                   \
			fprintf(stderr, "stage_check: %s: ", #cond); \
			fprintf(stderr, __VA_ARGS__);                \
			fprintf(stderr, "\n");                       \
			return 1;                                    \
		}                                                \
	} while (0)

static int check_layout(const size_t *bytes, size_t count)
{
	size_t off[8];
	for (size_t i = 0; i < 8; ++i)
		off[i] = 12345;   // (every entry is written, those of absent arrays too)
	const size_t total = stage_layout(bytes, count, off);
	size_t end = 0, room = 0;   // the end of the last slot; the padded room of the slots before the one looked at
	for (size_t i = 0; i < count; ++i) {
		if (bytes[i] == STAGE_ABSENT) {
			CHECK(off[i] == STAGE_ABSENT, "array %zu is absent, yet lies at %zu", i, off[i]);
			continue;
		}
		CHECK(off[i] % 256 == 0, "array %zu of %zu bytes at %zu", i, bytes[i], off[i]);
		// behind every slot before it, and no further than their padded sizes: an absent array took no room
		CHECK(off[i] >= end && off[i] == room, "array %zu of %zu bytes at %zu: the slots before it end at %zu and take %zu", i, bytes[i], off[i], end, room);
		for (size_t j = 0; j < i; ++j)
			if (bytes[j] != STAGE_ABSENT)
				CHECK(off[j] + bytes[j] <= off[i], "arrays %zu and %zu overlap: %zu + %zu > %zu", j, i, off[j], bytes[j], off[i]);
		end = off[i] + bytes[i];
		room = off[i] + (bytes[i] + 255) / 256 * 256;
	}
	CHECK(total == end, "total %zu, the last slot ends at %zu", total, end);
	return 0;
}

int main()
{
	static_assert(STAGE_ALIGN == 256, "the slots start on 256-byte boundaries");
	static const size_t sizes[6] = {STAGE_ABSENT, 0, 1, 255, 256, 257};
	size_t bytes[5];
	for (size_t count = 0; count <= 5; ++count) {
		size_t combos = 1;
		for (size_t i = 0; i < count; ++i)
			combos *= 6;
		for (size_t k = 0; k < combos; ++k) {
			size_t r = k;
			for (size_t i = 0; i < count; ++i, r /= 6)
				bytes[i] = sizes[r % 6];
			if (check_layout(bytes, count))
				return 1;
		}
	}
	// in numbers, once: [1][absent][257][256][0] lie at 0, -, 256, 768, 1024 and end at 1024; nothing at all takes nothing
	static const size_t one[5] = {1, STAGE_ABSENT, 257, 256, 0};
	size_t off[5];
	CHECK(stage_layout(one, 5, off) == 1024 && off[0] == 0 && off[1] == STAGE_ABSENT && off[2] == 256 && off[3] == 768 && off[4] == 1024,
	      "offsets %zu %zu %zu %zu %zu", off[0], off[1], off[2], off[3], off[4]);
	CHECK(stage_layout(one, 0, off) == 0, "no arrays take room");
	// sizes of real calls: n = 4099 indices of 4 and of 8 bytes and keys of 1 byte
	static const size_t real[3] = {4099 * 4, 4099 * 8, 4099};
	CHECK(stage_layout(real, 3, off) == 49664 + 4099 && off[1] == 16640 && off[2] == 49664, "offsets %zu %zu", off[1], off[2]);
	printf("stage_check OK\n");
	return 0;
}
