// rsx_stage.hpp: where the arrays of a blocking call on host buffers lie in the one staging buffer of the context (Ctx::stage) --
// a slot per array, each on a 256-byte boundary, each as large as its own array (staged_call, rsx_api.hpp; rsx_sort_lex).
// Part of librsx.so's host side, included by rsx.hip (one translation unit).
// Nothing of HIP and nothing of Ctx is used here: tests/cpp/stage_check.cpp includes this file alone and checks it on the CPU.
#pragma once

#include <cstddef>

namespace {

constexpr size_t STAGE_ALIGN = 256;
// as a size: the array is not there and takes no room; as an offset: it has no slot (nothing may be added to it)
constexpr size_t STAGE_ABSENT = ~(size_t)0;

// off[i] = where the slot of bytes[i] bytes begins; the total = where the last slot ends
inline size_t stage_layout(const size_t *bytes, size_t count, size_t *off)
{
	size_t end = 0;
	for (size_t i = 0; i < count; ++i) {
		off[i] = STAGE_ABSENT;
		if (bytes[i] == STAGE_ABSENT)
			continue;
		off[i] = (end + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1);
		end = off[i] + bytes[i];
	}
	return end;
}

}   // namespace
