// rsx_api.hpp: what the extern "C" entry points share -- dispatch by type, the refusal of a capturing stream, argument checks,
// host staging; part of librsx.so's host side, included by rsx.hip behind the routes (rsx_ctx.hpp: the context type, the error convention).
#pragma once

// (CALL may hold a launch: its commas lie bare once hipLaunchKernelGGL is expanded, hence the ...)
#define RSX_DISPATCH_KT(dtype, ...)                                \
	switch (dtype_size(dtype)) {                                   \
	case 1: { typedef uint8_t KT; __VA_ARGS__; } break;            \
	case 2: { typedef uint16_t KT; __VA_ARGS__; } break;           \
	case 4: { typedef uint32_t KT; __VA_ARGS__; } break;           \
	case 8: { typedef u64 KT; __VA_ARGS__; } break;                \
	default: return fail(RSX_EINVAL, "unknown dtype %d", (int)(dtype)); \
	}

// ... and a second type WT of `bytes` = 4 or 8 (checked by the caller): an index, a payload
#define RSX_DISPATCH_KT_W(dtype, bytes, WT, CALL)                  \
	if ((bytes) == 4) {                                            \
		typedef u32 WT;                                            \
		RSX_DISPATCH_KT(dtype, CALL)                               \
	} else {                                                       \
		typedef u64 WT;                                            \
		RSX_DISPATCH_KT(dtype, CALL)                               \
	}

// the (device, stream) context of a call, created at its first use and held to the end of the scope: calls that share a context
// share its workspace (Ctx::mu)
#define RSX_LOCKED_CTX(c, stream)     \
	Ctx *c;                           \
	RSX_TRY(get_ctx(stream, &c));     \
	std::lock_guard<std::recursive_mutex> ctx_lock(c->mu)

// ... of a device-scheduled entry point (enqueue only; the stream may be capturing): marked as such to the end of the scope
// (AsyncScope), on the set of flags that is the device-scheduled sorts' own (AsyncSetScope)
#define RSX_ASYNC_CTX(c, stream)                    \
	RSX_LOCKED_CTX(c, stream);                      \
	AsyncScope async_scope((hipStream_t)(stream));  \
	AsyncSetScope set_scope(*c)

namespace {

// what every plain sort refuses: an unknown dtype, a second array (payloads, indices) of other than 4- or 8-byte elements,
// a buffer that is missing where there are keys (`bufs`: all of them are there)
int sort_args(const char *who, rsx_dtype dtype, size_t n, bool bufs, size_t second_bytes = 4)
{
	if (!dtype_size(dtype) || (second_bytes != 4 && second_bytes != 8) || (n && !bufs))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	return RSX_OK;
}

// A call that waits for the device cannot be captured (a query that fails is no refusal: the call goes on)
int refuse_capture(void *stream, const char *who, const char *why)
{
	hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess)
		(void)hipGetLastError();
	else if (st != hipStreamCaptureStatusNone)
		return fail(RSX_EINVAL, "%s: the stream is capturing (%s)", who, why);
	return RSX_OK;
}

// the caller's info struct or a local one, cleared
template <typename T> T *info_or(T *info, T *local)
{
	if (!info)
		info = local;
	memset(info, 0, sizeof(*info));
	return info;
}

// the width of the indices a call of n keys writes, and whether the largest of them fits it: n - 1 where they are positions
// (idx_last), n itself where they may be counts
int idx_args(const char *who, size_t idx_bytes, size_t n, size_t largest)
{
	if (idx_bytes != 4 && idx_bytes != 8)
		return fail(RSX_EINVAL, "%s: idx_bytes = %zu (4 or 8)", who, idx_bytes);
	if (idx_bytes == 4 && (uint64_t)largest > 0xFFFFFFFFull)
		return fail(RSX_EINVAL, "%s: n = %zu does not fit a 4-byte index", who, n);
	return RSX_OK;
}
inline size_t idx_last(size_t n) { return n ? n - 1 : 0; }

// rsx_sort_topk*, rsx_sort_nth*: keys of one type in, keys and / or their indices out
int select_args(const char *who, const void *src, size_t n, rsx_dtype dtype, rsx_order order, const void *out_keys, const void *out_idx,
                size_t idx_bytes)
{
	if (!dtype_size(dtype) || (order != RSX_ASCENDING && order != RSX_DESCENDING) || (n && !src))
		return fail(RSX_EINVAL, "%s: bad argument", who);
	if (!out_keys && !out_idx)
		return fail(RSX_EINVAL, "%s: both outputs are NULL", who);
	return idx_args(who, idx_bytes, n, idx_last(n));
}

// ... the host entry point behind its checks.  run(keys, out_keys, out_idx) is the _device entry point: on the caller's buffers where
// they are the device's; else on the keys staged in recs[0] as rsx_sort_rank stages them, and the `count` results are brought back
// through `out` = [keys, padded to 16 bytes][indices]
template <typename F>
int select_run(Ctx &c, const char *who, DevBuf &out, const void *src, size_t n, size_t kb, size_t count, void *out_keys, void *out_idx,
               size_t idx_bytes, F run)
{
	if (is_device_ptr(src)) {
		if ((out_keys && !is_device_ptr(out_keys)) || (out_idx && !is_device_ptr(out_idx)))
			return fail(RSX_EINVAL, "%s: src is a device pointer but an output is not", who);
		RSX_TRY(run(src, out_keys, out_idx));
		HIP_TRY(hipStreamSynchronize(c.stream));
		return RSX_OK;
	}
	const size_t pad = (count * kb + 15) & ~(size_t)15;
	RSX_TRY(c.recs[0].ensure(n * kb));
	RSX_TRY(out.ensure(pad + count * idx_bytes));
	HIP_TRY(hipMemcpyAsync(c.recs[0].p, src, n * kb, hipMemcpyHostToDevice, c.stream));
	char *dk = (char *)out.p, *di = dk + pad;
	RSX_TRY(run(c.recs[0].p, out_keys ? dk : nullptr, out_idx ? di : nullptr));
	if (out_keys)
		HIP_TRY(hipMemcpyAsync(out_keys, dk, count * kb, hipMemcpyDeviceToHost, c.stream));
	if (out_idx)
		HIP_TRY(hipMemcpyAsync(out_idx, di, count * idx_bytes, hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	return RSX_OK;
}

// n == 1 is answered on the host where `p` is the host's: there is no device (asked first: then no device call is made), or
// there is one and `p` is not its memory
bool one_on_host(size_t n, const void *p) { return n == 1 && (rsx_device_count() <= 0 || !is_device_ptr(p)); }

}  // namespace
