// rsx_ws_layout.hpp: where the parts of a caller-owned workspace lie (WsLayout) -- what rsx_workspace_bytes[_fast] promise, what
// borrow_ctx / borrow_blind hand to the context, and where rsx_async_route_ws reads the plan and the attempt's control block back.
// Part of librsx.so's host side, included by rsx.hip (one translation unit).
// Nothing of HIP and nothing of Ctx is used here: tests/cpp/ws_layout_check.cpp includes this file alone and checks it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

// ---- the fixed small state of a context (Ctx::small, one set): [unsorted u32 | hotd 9 u32 | plan_done | pad 64][Plan 64][kept 16 u32 64] ----
constexpr size_t WS_FLAGS_BYTES = 256;       // one set of flags (Ctx::SMALL_BYTES)
constexpr size_t WS_PLAN_OFF = 64;           // the Plan inside a set (Ctx::plan(), Ctx::async_plan())
constexpr size_t WS_HPART_ROWS = 512;        // the histogram kernel's rows: at most 512 workgroups (launch_hist)
constexpr size_t WS_BOUND_PAD = 256;         // what rsx_workspace_bytes adds to its bound; rsx_workspace_bytes_fast twice that

inline size_t ws_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// A sort without a histogram is attempted inside a workspace for these keys only (borrow_blind, rsx_workspace_bytes_fast,
// rsx_async_route_ws): keys of 4 bytes or more, 2^22 <= n < 2^30
inline bool ws_blind_window(size_t key_bytes, size_t n) { return key_bytes >= 4 && n >= ((size_t)1 << 22) && n < ((size_t)1 << 30); }

// bytes of what such an attempt needs (blind_sizes, rsx_route_blind.hpp: each rounded up to 256); all zero: no attempt
struct WsBlind {
	size_t gscan = 0, seg = 0, slack1 = 0, slack = 0;
	size_t total() const { return gscan + seg + slack1 + slack; }
};

// The status words rsx_workspace_bytes sets aside -- an upper bound over the kernels' shapes: quarter tiles (8 Ki elements,
// 4 Ki with an 8-byte element), a region per pass, 64-bit words from 2^30 keys on (a sort's own figure: status_bytes x key bytes)
inline size_t ws_status_bound(size_t n, size_t key_bytes, size_t payload_bytes)
{
	const size_t elem = key_bytes > payload_bytes ? key_bytes : payload_bytes;
	const size_t tile = elem == 8 ? 4096 : 8192;
	const size_t tiles = (n + tile - 1) / tile;
	return (256 + tiles * 256 * (n >= ((size_t)1 << 30) ? 8 : 4)) * key_bytes;
}

// [flags 256][second plan 64 + pad to 512][histogram][status regions, padded][histogram rows] -- `minimal` -- and, 256-aligned
// behind them, what an attempt without a histogram takes: [gscan][seg: SegCtl first][level-1 slots][level-2 slots] -- `fast_total`
struct WsLayout {
	size_t flags_off = 0;        // Ctx::small
	size_t plan_off = 0;         // ... the Plan in it, which the kernels of a device-scheduled sort write
	size_t plan2_off = 0;        // Ctx::dev_host_plan: the kernels' second copy of the plan (nobody reads it on the host)
	size_t hist_off = 0, hist_bytes = 0;       // Ctx::hist: [key bytes][256] u64
	size_t status_off = 0, status_bytes = 0;   // Ctx::status: status_total rounded up to 256
	size_t hpart_off = 0, hpart_bytes = 0;     // Ctx::hpart: [WS_HPART_ROWS][key bytes][256] u32
	size_t minimal = 0;          // what every *_ws sort needs
	size_t gscan_off = 0, seg_off = 0, slack1_off = 0, slack_off = 0;   // Ctx::gscan, seg, slack1, slack (sizes: `blind`)
	WsBlind blind;
	size_t fast_total = 0;       // ... with the attempt's part: borrowed if the workspace holds this much (minimal if there is none)
	bool blind_fits(size_t ws_bytes) const { return blind.total() != 0 && fast_total <= ws_bytes; }
	// what rsx_workspace_bytes / rsx_workspace_bytes_fast return for a layout made from ws_status_bound
	size_t bound() const { return minimal + WS_BOUND_PAD; }
	size_t bound_fast() const { return fast_total + 2 * WS_BOUND_PAD; }
};

inline WsLayout ws_layout_for(size_t key_bytes, size_t status_total, const WsBlind &blind = WsBlind())
{
	WsLayout l;
	l.flags_off = 0;
	l.plan_off = l.flags_off + WS_PLAN_OFF;
	l.plan2_off = l.flags_off + WS_FLAGS_BYTES;
	l.hist_off = 2 * WS_FLAGS_BYTES;
	l.hist_bytes = key_bytes * 256 * sizeof(uint64_t);
	l.status_off = l.hist_off + l.hist_bytes;
	l.status_bytes = ws_align256(status_total);
	l.hpart_off = l.status_off + l.status_bytes;
	l.hpart_bytes = WS_HPART_ROWS * key_bytes * 256 * sizeof(uint32_t);
	l.minimal = l.hpart_off + l.hpart_bytes;
	l.blind = blind;
	l.gscan_off = ws_align256(l.minimal);
	l.seg_off = l.gscan_off + blind.gscan;
	l.slack1_off = l.seg_off + blind.seg;
	l.slack_off = l.slack1_off + blind.slack1;
	l.fast_total = l.slack_off + blind.slack;
	return l;
}

}   // namespace
