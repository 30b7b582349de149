// ws_layout_check: WsLayout (radix_sorting_amd/csrc/rsx_ws_layout.hpp) on the CPU -- the layout of a caller-owned workspace against
// what rsx_workspace_bytes, borrow_ctx, borrow_blind, rsx_workspace_bytes_fast and rsx_async_route_ws each wrote out themselves
// before there was one struct for it.  No GPU and no library: the program includes the header alone; exits non-zero at the
// first mismatch.
#include "../../radix_sorting_amd/csrc/rsx_ws_layout.hpp"

#include <cstdio>

typedef unsigned long long ull;

#define CHECK(cond, ...)                                 \
	do {                                                 \
		if (!(cond)) {                                   \
			fprintf(stderr, "ws_layout_check: %s: ", #cond); \
			fprintf(stderr, __VA_ARGS__);                \
			fprintf(stderr, "\n");                       \
			return 1;                                    \
		}                                                \
	} while (0)

static ull align256(ull b) { return (b + 255) / 256 * 256; }

// One workspace: keys of kb bytes, status words of `status_total` bytes, the parts of an attempt without a histogram of
// g / sg / s1 / s2 bytes (all zero: none).  The expectations are the expressions of the functions named, in numbers.
static int check_layout(size_t kb, ull status_total, ull g, ull sg, ull s1, ull s2)
{
	WsBlind b;
	b.gscan = (size_t)g, b.seg = (size_t)sg, b.slack1 = (size_t)s1, b.slack = (size_t)s2;
	const WsLayout l = ws_layout_for(kb, (size_t)status_total, b);
	// borrow_ctx: [256 flags][plan at +256][512][hist][status, padded][hist rows]; need = their sum
	const ull hist = kb * 256 * 8, hpart = 512ull * kb * 256 * 4, st = align256(status_total);
	CHECK(l.flags_off == 0 && l.plan2_off == 256 && l.hist_off == 512, "%zu-byte keys: flags %zu, second plan %zu, hist %zu", kb, l.flags_off, l.plan2_off, l.hist_off);
	CHECK(l.hist_bytes == hist && l.status_off == 512 + hist, "%zu-byte keys: hist of %zu bytes, status at %zu", kb, l.hist_bytes, l.status_off);
	CHECK(l.status_bytes == st && l.status_bytes >= status_total && l.status_bytes % 256 == 0, "%zu-byte keys: status of %zu bytes for %llu", kb, l.status_bytes, status_total);
	CHECK(l.hpart_off == 512 + hist + st && l.hpart_bytes == hpart, "%zu-byte keys: rows at %zu, %zu bytes", kb, l.hpart_off, l.hpart_bytes);
	CHECK(l.minimal == 512 + hist + st + hpart, "%zu-byte keys: minimal %zu", kb, l.minimal);
	// rsx_async_route_ws: the plan at + 64 -- where Ctx::plan() points in a set of flags
	CHECK(l.plan_off == 64 && WS_PLAN_OFF == 64 && l.plan_off + 64 <= WS_FLAGS_BYTES, "the plan at %zu", l.plan_off);
	// borrow_blind: gscan at the 256-aligned end of borrow_ctx's part, then seg, slack1, slack;
	// rsx_async_route_ws: the control block at align256(minimal) + 256 * sizeof(u64)
	CHECK(l.gscan_off == align256(l.minimal) && l.gscan_off % 256 == 0, "%zu-byte keys: gscan at %zu", kb, l.gscan_off);
	CHECK(l.seg_off == l.gscan_off + g && l.slack1_off == l.seg_off + sg && l.slack_off == l.slack1_off + s1, "%zu-byte keys: seg %zu, slack1 %zu, slack %zu", kb, l.seg_off, l.slack1_off, l.slack_off);
	CHECK(l.fast_total == l.gscan_off + g + sg + s1 + s2, "%zu-byte keys: fast total %zu", kb, l.fast_total);
	if (g) {
		CHECK(g == 256 * 8 && l.seg_off == align256(l.minimal) + 256 * 8, "%zu-byte keys: the control block at %zu", kb, l.seg_off);
		// borrowed by a workspace of exactly the fast total, not by one a byte short of it, nor by the minimal one
		CHECK(l.blind_fits(l.fast_total) && l.blind_fits(l.fast_total + 1), "%zu-byte keys: a workspace of the fast total does not borrow", kb);
		CHECK(!l.blind_fits(l.fast_total - 1) && !l.blind_fits(l.minimal), "%zu-byte keys: a workspace one byte short borrows", kb);
	} else {
		CHECK(l.fast_total == l.minimal && !l.blind_fits(l.fast_total) && !l.blind_fits((size_t)1 << 40), "%zu-byte keys: nothing to borrow, yet borrowed", kb);
	}
	// rsx_workspace_bytes_fast: align256(rsx_workspace_bytes) + 256 + g + sg + s1 + s2, rsx_workspace_bytes = minimal + 256
	CHECK(l.bound() == l.minimal + 256 && l.bound_fast() == align256(l.bound()) + 256 + g + sg + s1 + s2, "%zu-byte keys: bounds %zu, %zu", kb, l.bound(), l.bound_fast());
	CHECK(l.bound_fast() >= l.fast_total, "%zu-byte keys: the fast bound %zu is below the fast total %zu", kb, l.bound_fast(), l.fast_total);
	return 0;
}

int main()
{
	// ---- rsx_workspace_bytes(n, dtype, payload_bytes) for payloads of 0 and 8 bytes, and the status words in it: the four key
	// widths at n = 2, 2^22 - 1, 2^22, 2^30 - 1 and 2^30 (where the status words become 64-bit), from
	//   elem = max(kb, payload); tile = elem == 8 ? 4096 : 8192; status = (256 + ceil(n / tile) * 256 * (n >= 2^30 ? 8 : 4)) * kb
	//   512 + kb * 2048 + align256(status) + 512 * kb * 1024 + 256
	static const ull ns[5] = {2, (1ull << 22) - 1, 1ull << 22, (1ull << 30) - 1, 1ull << 30};
	static const struct { size_t kb; struct { ull bytes0, bytes8, status0; } at[5]; } bounds[4] = {
	    {1, {{528384, 528384, 1280}, {1051648, 1575936, 524544}, {1051648, 1575936, 524544}, {134745088, 268962816, 134217984}, {268962816, 537398272, 268435712}}},
	    {2, {{1056000, 1056000, 2560}, {2102528, 3151104, 1049088}, {2102528, 3151104, 1049088}, {269489408, 537924864, 268435968}, {537924864, 1074795776, 536871424}}},
	    {4, {{2111232, 2111232, 5120}, {4204288, 6301440, 2098176}, {4204288, 6301440, 2098176}, {538978048, 1075848960, 536871936}, {1075848960, 2149590784, 1073742848}}},
	    {8, {{4221696, 4221696, 10240}, {12602112, 12602112, 8390656}, {12602112, 12602112, 8390656}, {2151697152, 2151697152, 2147485696}, {4299180800, 4299180800, 4294969344}}},
	};
	for (const auto &w : bounds)
		for (int i = 0; i < 5; ++i) {
			const size_t n = (size_t)ns[i];
			CHECK(ws_status_bound(n, w.kb, 0) == w.at[i].status0, "%zu-byte keys, n = %llu: status bound %zu", w.kb, ns[i], ws_status_bound(n, w.kb, 0));
			CHECK(ws_layout_for(w.kb, ws_status_bound(n, w.kb, 0)).bound() == w.at[i].bytes0, "%zu-byte keys, n = %llu: rsx_workspace_bytes %zu", w.kb, ns[i],
			      ws_layout_for(w.kb, ws_status_bound(n, w.kb, 0)).bound());
			CHECK(ws_layout_for(w.kb, ws_status_bound(n, w.kb, 8)).bound() == w.at[i].bytes8, "%zu-byte keys, n = %llu, 8-byte payloads: rsx_workspace_bytes %zu", w.kb,
			      ns[i], ws_layout_for(w.kb, ws_status_bound(n, w.kb, 8)).bound());
			// the attempt in a workspace: keys of 4 bytes or more, 2^22 <= n < 2^30
			CHECK(ws_blind_window(w.kb, n) == (w.kb >= 4 && i >= 2 && i <= 3), "%zu-byte keys, n = %llu: the window says %d", w.kb, ns[i], (int)ws_blind_window(w.kb, n));
			// the layout with the bound's status words, with a sort's own (smaller, not a multiple of 256), without and with an
			// attempt's parts (gscan is 256 u64; the others any multiples of 256)
			if (check_layout(w.kb, w.at[i].status0, 0, 0, 0, 0) || check_layout(w.kb, w.at[i].status0 / 2 + 16, 0, 0, 0, 0) ||
			    check_layout(w.kb, w.at[i].status0, 2048, 2896896, 1342177280 + 131072, 134217728 + 65536) ||
			    check_layout(w.kb, w.at[i].status0 / 2 + 16, 2048, 6834432, 256, 256))
				return 1;
		}
	// rsx_workspace_bytes_fast in numbers, once: 4-byte keys, n = 2^22, an attempt of 2048 + 3289856 + 4325376 + 2228224 bytes behind
	// rsx_workspace_bytes = 4204288: 4204288 + 256 + 9845504
	WsBlind b;
	b.gscan = 2048, b.seg = 3289856, b.slack1 = 4325376, b.slack = 2228224;
	const WsLayout l = ws_layout_for(4, ws_status_bound((size_t)1 << 22, 4, 0), b);
	CHECK(l.bound_fast() == 14050048 && l.fast_total == 14049536 && l.seg_off == 4204032 + 2048, "bound_fast %zu, fast_total %zu, seg at %zu", l.bound_fast(), l.fast_total, l.seg_off);
	printf("ws_layout_check OK\n");
	return 0;
}
