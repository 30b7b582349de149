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

// the grid of a small grid-stride kernel: `per` items to a workgroup, `most` workgroups at most
inline unsigned small_grid(u64 count, unsigned per, unsigned most) { return (unsigned)std::min<u64>(most, std::max<u64>(1, (count + per - 1) / per)); }

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

// ---- host staging: what the blocking entry points do around their _device entry point -------------------------------------------
// is every pointer of `ps` that is there the device's, the host's, or are they mixed?
enum PtrKind { PTR_HOST, PTR_DEVICE, PTR_MIXED };
inline PtrKind pointer_kind(const void *const *ps, size_t count)
{
	bool device = false, host = false;
	for (size_t i = 0; i < count; ++i)
		if (ps[i])
			(is_device_ptr(ps[i]) ? device : host) = true;
	return device && host ? PTR_MIXED : device ? PTR_DEVICE : PTR_HOST;
}
inline int mixed_pointers(const char *who) { return fail(RSX_EINVAL, "%s: host and device pointers in one call", who); }

// one array of a blocking call.  Key columns are staged as rsx_sort_rank stages them, the first in recs[0], a second in recs[1]
// (the _device routes leave recs[] alone); every other array in a slot of Ctx::stage (rsx_stage.hpp)
enum StageHome { STAGE_SLOT, STAGE_RECS0, STAGE_RECS1 };
struct StageRow {
	const void *ptr;   // the caller's; nullptr: the array is absent
	size_t up;         // bytes to upload before the call (0: a pure output)
	size_t room;       // bytes to set aside on the device (0: nothing is read or written there, so whose memory it is does not matter)
	StageHome home = STAGE_SLOT;
};

// ... the host entry point behind its checks and shortcuts.  run(d, back) is the _device entry point on d[i] = the caller's own
// pointers where they are the device's; else on the staged arrays, and back[i] bytes -- what run() says -- are brought back into
// each output that is there.  The stream is through when the call returns.
template <size_t N, typename F> int staged_call(Ctx &c, const char *who, const StageRow (&rows)[N], F run)
{
	const void *ps[N];
	size_t bytes[N], off[N], back[N] = {};
	void *d[N];
	for (size_t i = 0; i < N; ++i) {
		ps[i] = rows[i].room ? rows[i].ptr : nullptr;
		bytes[i] = rows[i].ptr && rows[i].home == STAGE_SLOT ? rows[i].room : STAGE_ABSENT;
		d[i] = (void *)rows[i].ptr;
	}
	const PtrKind kind = pointer_kind(ps, N);
	if (kind == PTR_MIXED)
		return mixed_pointers(who);
	if (kind == PTR_HOST) {
		RSX_TRY(c.stage.ensure(stage_layout(bytes, N, off)));
		for (size_t i = 0; i < N; ++i) {
			if (!rows[i].ptr)
				continue;
			if (rows[i].home == STAGE_SLOT) {
				d[i] = (char *)c.stage.p + off[i];
			} else {
				DevBuf &b = c.recs[rows[i].home == STAGE_RECS1];
				RSX_TRY(b.ensure(rows[i].room));
				d[i] = b.p;
			}
			if (rows[i].up)
				HIP_TRY(hipMemcpyAsync(d[i], rows[i].ptr, rows[i].up, hipMemcpyHostToDevice, c.stream));
		}
	}
	RSX_TRY(run(d, back));
	if (kind == PTR_HOST)
		for (size_t i = 0; i < N; ++i)
			if (rows[i].ptr && back[i])
				HIP_TRY(hipMemcpyAsync((void *)rows[i].ptr, d[i], back[i], hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	return RSX_OK;
}

// n == 1 is answered on the host where `p` is the host's: there is no device (asked first: then no device call is made), or
// there is one and `p` is not its memory
bool one_on_host(size_t n, const void *p) { return n == 1 && (rsx_device_count() <= 0 || !is_device_ptr(p)); }

}  // namespace
