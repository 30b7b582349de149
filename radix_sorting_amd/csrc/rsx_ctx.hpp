// rsx_ctx.hpp: what every host function uses -- the error convention (fail, HIP_TRY, RSX_TRY), DevBuf, the per (device, stream) context
// Ctx, profiling, the device checks, get_ctx; part of librsx.so's host side, included by rsx.hip behind rsx_env.hpp, rsx_seg_layout.hpp, rsx_ws_layout.hpp and rsx_stage.hpp, ahead of the routes.
#pragma once

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return code;
}

#define HIP_TRY(expr)                                                                              \
	do {                                                                                           \
		hipError_t e_ = (expr);                                                                    \
		if (e_ != hipSuccess) {                                                                    \
			(void)hipGetLastError();                                                               \
			return fail(e_ == hipErrorOutOfMemory ? RSX_ENOMEM : RSX_EHIP, "%s failed: %s (%s:%d)", #expr, \
			            hipGetErrorString(e_), __FILE__, __LINE__);                                \
		}                                                                                          \
	} while (0)

#define RSX_TRY(expr)          \
	do {                       \
		int rc_ = (expr);      \
		if (rc_ != RSX_OK)     \
			return rc_;        \
	} while (0)

size_t dtype_size(int dtype)
{
	switch (dtype) {
	case RSX_U8: case RSX_I8: return 1;
	case RSX_U16: case RSX_I16: return 2;
	case RSX_U32: case RSX_I32: case RSX_F32: return 4;
	case RSX_U64: case RSX_I64: case RSX_F64: return 8;
	default: return 0;
	}
}

template <typename KT>
KdfArgs<KT> make_kdf(int dtype, int order)
{
	KdfArgs<KT> a;
	const KT high = (KT)((KT)1 << (sizeof(KT) * 8 - 1));
	const bool is_signed = dtype == RSX_I8 || dtype == RSX_I16 || dtype == RSX_I32 || dtype == RSX_I64;
	const bool is_float = dtype == RSX_F32 || dtype == RSX_F64;
	a.fmask = is_float ? (KT)~(KT)0 : (KT)0;
	a.sflip = (is_signed || is_float) ? high : (KT)0;
	a.desc = order == RSX_DESCENDING ? (KT)~(KT)0 : (KT)0;
	return a;
}

// ---- the *_inplace_async entry points (enqueue only; the stream may be capturing a graph) mark their extent ----------------
// What the mark changes: a scratch buffer that would have to grow under a capture is an error instead of a hipFree / hipMalloc
// (DevBuf::ensure), and no slot array is ever released from inside such a call (blind_enqueue, pairs_blind_enqueue): a graph
// captured earlier on this context may still name it.
thread_local bool g_in_async = false;
thread_local hipStream_t g_async_stream = nullptr;
struct AsyncScope {
	bool prev;
	hipStream_t prev_stream;
	explicit AsyncScope(hipStream_t s) : prev(g_in_async), prev_stream(g_async_stream)
	{
		g_in_async = true;
		g_async_stream = s;
	}
	~AsyncScope()
	{
		g_in_async = prev;
		g_async_stream = prev_stream;
	}
	AsyncScope(const AsyncScope &) = delete;
	AsyncScope &operator=(const AsyncScope &) = delete;
};

// ---- a growable device allocation -------------------------------------------
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	bool external = false;   // a slice of a caller-owned workspace (rsx_sort_inplace_async_ws): never grown, never freed
	// Inside a *_inplace_async entry point (AsyncScope) the stream may be capturing: a buffer never grows under a capture -- the
	// graph would keep the old address, and hipFree / hipMalloc are not capturable.
	int ensure(size_t bytes)
	{
		if (bytes <= cap)
			return RSX_OK;
		if (external)
			return fail(RSX_EINVAL, "the caller's workspace is too small: %zu bytes needed where %zu were set aside "
			                        "(size it with rsx_workspace_bytes)", bytes, cap);
		if (g_in_async) {
			hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
			if (hipStreamIsCapturing(g_async_stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
				return fail(RSX_EINVAL, "a scratch buffer would have to grow (%zu -> %zu bytes) while the stream is capturing: run the "
				                        "sort once outside the capture, or use the *_ws entry points with a workspace of your own",
				            cap, bytes);
			(void)hipGetLastError();
		}
		// A buffer that GROWS is rounded up to an eighth of the power of two below its size (buffers of 2 MiB and more; smaller
		// ones get an eighth on top): a sort of slightly more keys than the last one -- the sub-ranges of a distributed sort, a
		// growing table -- finds room instead of paying hipFree + hipMalloc, and hipFree synchronises the device.  At most
		// 12.5 % above the request (round 4 gave GiB-sized slot arrays no headroom at all and re-allocated on every record
		// size).  A buffer's FIRST allocation is what was asked for (to 2 MiB): the four slot arrays of 2^28 pairs, a tile
		// above 1.25 GiB each, took 1.375 -- half a GiB for sorts that never come; sizes that do vary pay one re-allocation.
		size_t want = bytes + bytes / 8;
		if (!p && bytes >= ((size_t)2 << 20)) {
			want = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
		} else if (bytes >= ((size_t)2 << 20)) {
			size_t p2 = (size_t)1 << 21;
			while ((p2 << 1) <= bytes)
				p2 <<= 1;
			const size_t step = p2 / 8;
			want = (bytes + step - 1) / step * step;
		}
		// The new allocation is made BEFORE the old one goes: if it fails the old buffer (which a graph captured earlier may
		// still name) stays where it is; only then the old one is given up to make room.
		void *np = nullptr;
		hipError_t e = hipMalloc(&np, want);
		if (e != hipSuccess) {
			(void)hipGetLastError();
			want = bytes;
			e = hipMalloc(&np, want);
		}
		if (e != hipSuccess && p && !g_in_async) {
			(void)hipGetLastError();
			(void)hipFree(p);
			p = nullptr;
			cap = 0;
			e = hipMalloc(&np, want);
		}
		if (e != hipSuccess) {
			(void)hipGetLastError();
			return fail(RSX_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
		}
		if (p)
			(void)hipFree(p);
		p = np;
		cap = want;
		return RSX_OK;
	}
	void release()
	{
		if (p && !external)
			(void)hipFree(p);
		p = nullptr;
		cap = 0;
	}
	void borrow(void *ptr, size_t bytes)
	{
		p = ptr;
		cap = bytes;
		external = true;
	}
};

// ---- per (device, stream) context --------------------------------------------
struct Ctx {
	int device = -1;
	hipStream_t stream = nullptr;
	// fixed small state: [unsorted u32 | hotd 9 u32 | plan_done | pad 64][Plan 64][kept 16 u32 64]
	DevBuf small;
	DevBuf hist;        // counts, then exclusive offsets [key bytes][256] u64
	DevBuf hpart;       // the histogram kernel's per-workgroup rows [workgroups][key bytes][256] u32
	DevBuf status;      // [ticket u32, pad to 256 B][tiles * 256 status words]
	DevBuf keys[2];     // key ping-pong for rank sorts / host staging
	DevBuf vals[2];     // payload ping-pong for host staging / narrow-index rank
	DevBuf recs[2];     // record gather staging; the key columns of a blocking call on host buffers (staged_call)
	DevBuf stage;       // ... its other arrays, a slot each (rsx_stage.hpp).  One buffer for every entry point: a blocking call holds `mu` and is through before it returns
	DevBuf tkeys;       // keys extracted from records (rsx_sort_records_tagged*)
	DevBuf ckeys;       // rank sorts: the keys' varying bits packed together (RSX_COMPACT_BITS)
	DevBuf joint;       // 2-byte keys: [65536 u32 counts][65537 u64 offsets] of the 16-bit digit (rsx_joint16_kernel)
	DevBuf seg;         // two-level sorts (rsx_hybrid.hpp): [SegCtl][per-bucket digit counts][status regions][leaf segments][tiles]
	SegLayout seg_lay;  // ... where they lie, for the sort being enqueued (seg_layout, rsx_route_levels.hpp; read through SegView)
	SelfPlanArgs pass_sp{nullptr, nullptr, nullptr, nullptr, HybCaps{0, 0, 0, 0}};   // a self-planned pass 0 (SCATTER_SELF_PLAN)
	DevBuf gscan;       // [256] u64: the highest kept column's offsets from a self-planned pass 0 (for the leaves)
	// rsx_sort_inplace_async after an attempt without the histogram: the control block whose `mode` tells the histogram-first
	// kernels enqueued behind it that there is nothing left to do
	const SegCtl *pass_gate = nullptr;
	bool async_tried_blind = false;   // ... whether the last rsx_sort_inplace_async of this context enqueued such an attempt
	bool ws_blind = false;            // a context in a caller's workspace that has room for the slots of a sort without a histogram (borrow_ctx)
	bool boff_forget = false;   // rsx_reload_env since the last attempt: SegCtl::boff_* are zeroed before the next one
	u32 hints = 0;                    // what the caller of the sort being enqueued has said about its keys (rsx_sort_inplace_async_hint)
	bool async_small = false;         // ... or was the one-launch sort of a small array (rsx_async_route: 0, whatever the device's words say)
	const void *pass_alt = nullptr;   // rsx_sort_rank_inplace_async: the second work copy of the keys (SCATTER_RANK_ASYNC passes)
	DevBuf vsum;        // RSX_VERIFY=2: [descents, sum, mix] of the input and of the result
	DevBuf vasync;      // RSX_VERIFY: mismatches found in device-scheduled passes, kept until rsx_verify_poll / the next blocking sort
	DevBuf slack_v;     // ... the payloads' slots (key + payload and rank sorts)
	DevBuf slack;       // two-level sorts, slack attempt: 65536 slots of slack_cap keys (+ a tile of padding)
	u32 slack_cap = 0;
	u32 slack_mean = 0;   // the mean number of keys of a level-2 slot of the sort being enqueued (n / 65536: pass16a_wanted)
	DevBuf slack1_v;    // ... and of as many payloads (pairs_blind)
	DevBuf slack1;      // sorts without a histogram (sort_keys_blind): the level-1 pass's 256 slots of slack1_cap keys
	DevBuf logb;        // rsx_logroute.hpp: [LogCtl][LogTabs][level-2 cursors 2 x 65536][level-2 tiles]
	DevBuf logslots;    // ... the level-2 slots (four bytes per key)
	DevBuf ubits;       // rsx_sort_unique*: the bitmap, one bit per packed value (at most 2^RSX_UNIQUE_MAX_BITS / 8 bytes)
	DevBuf urecs;       // ... [8 u64: sample / totals][UniqueRec per chunk of the bitmap or tile of the sorted array]
	DevBuf gcells;      // rsx_sort_group*: one GroupCell per word of the bitmap in ubits: the word and the set bits below it
	DevBuf rdtab;       // rsx_sort_rankdata*: [workgroups][256] u64 bases of the place, or [65536 u32 counts][65537 u64 offsets] of the packed varying bits
	DevBuf tkctl;       // rsx_sort_topk*: [TopkCtl][rows of the input's ranges][rows of the candidates'][their offsets]
	DevBuf tkpairs;     // ... the k (key, index) pairs and the second buffers of their sort: [keys k][keys k][indices k][indices k]
	DevBuf tkcand;      // ... the selected bucket's (key, index) candidates: [keys cap][indices cap], cap = n / 8 + 1024
	DevBuf nthctl;      // rsx_sort_nth*: [NthCtl][table: 64 buckets x 256 digits u64][counts of the input's ranges u64]
	DevBuf nthcand;     // ... the active buckets' (key, index) candidates and the second buffers of their sort: [keys cap] x 2 [indices cap] x 2
	DevBuf nthio;       // ... [ranks m u64][n_less m u64][n_equal m u64][record of each position m u32]
	DevBuf loctab;      // rsx_sort_locate*: the search route's [header][start table][edges][cum][column totals][one row of counts per workgroup], or the table route's counts and offsets of keys and values
	DevBuf locvals;     // ... [values m][values m]: a copy of the values and the second buffer of its sort
	DevBuf rcells;      // rsx_sort_reduce*: the table of cells [counts][sums][minima][maxima], or a ReducePart per tile of the sorted array
	DevBuf jointab;     // rsx_sort_join*: the table route's counts and offsets of the right keys, behind them two sums per workgroup of the probe
	DevBuf joinkeys;    // ... the merge route: [left keys n][left keys n], a copy of the left keys and the second buffer of its sort
	DevBuf joinidx;     // ... [indices n] x 4: the left permutation, the second buffer of its sort, start and count in sorted order; or n counts nobody asked for
	DevBuf jointiles;   // rsx_sort_join*, rsx_join_pairs*: [row tiles + 1] u64: the pairs of every tile of rows, scanned
	DevBuf lexkeys;     // rsx_sort_lex*: [keys n][keys n] of the widest packed type: a group's keys and the second buffer of their sort
	DevBuf lexidx;      // ... [indices n][indices n][indices n]: the permutation found so far and the second buffer of its sort
	DevBuf parttab;     // rsx_sort_partition*: the scatter route's [header][start table][edges][cum][one row of counts per workgroup][one row of starts per workgroup]
	DevBuf partvals;    // ... [edges m][edges m]: a copy of the edges and the second buffer of its sort
	DevBuf partidx;     // ... the sort route: [bins n][indices n][indices n][equal m]: locate's bins, the two halves of their rank sort, locate's equal
	DevBuf segtab;      // rsx_sort_segments*: [plan record][one row of counts per workgroup][one row of starts][the long segments' (start, length)][the segment numbers m, class by class]
	DevBuf segwork;     // ... the composed route: [segment number of every key n][the permutation n] (its sorts work in lex's buffers, as the long segments' sorts do)
	SegmentsPlan *host_segplan = nullptr, *dev_host_segplan = nullptr;   // pinned, written by rsx_segments_scan_kernel
	LogCtl *host_logctl = nullptr;   // pinned: the control block as the device left it
	hipEvent_t log_ev = nullptr;
	u32 slack1_cap = 0;
	u32 slack1_lo = 0;  // ... of which the first slack1_lo lie in the caller's second buffer (keys-only sorts; 0: all in slack1)
	bool narrow1 = false;   // 8-byte keys: the forms that keep low words in the level-1 slots are enqueued too (SegCtl::narrow == 2 picks them)
	// ... sorts to go before the next attempt, doubled by every attempt that is called off; per kind of sort (4- / 8-byte keys,
	// rank sorts, keys + payload): what one kind's inputs look like says nothing about another's
	u32 blind_skip[4] = {0, 0, 0, 0}, blind_backoff[4] = {0, 0, 0, 0};
	u32 log_skip = 0, log_backoff = 0;       // ... and the same for the attempts by (bit length, mantissa) digits (sort_keys_log): a refused or lost one costs 65 us and more
	bool blind_no_room = false;              // the slots could not be allocated once: not asked for again (until rsx_reload_env)
	u32 env_epoch = 0;                       // ... forgotten when rsx_reload_env() has run since
	SegCtl *host_segctl = nullptr, *dev_host_segctl = nullptr;   // pinned, written by rsx_seg_plan_kernel
	hipEvent_t seg_ev = nullptr;
	Plan *host_plan = nullptr;   // pinned, written by the kernels themselves (dev_host_plan: its device address)
	Plan *dev_host_plan = nullptr;
	hipEvent_t plan_ev = nullptr;   // recorded behind the plan's copy to the host
	u64 *host_hist = nullptr;    // pinned, 256 u64
	// Small sorts of host buffers (rsx_sort, rsx_sort_rank on arrays the one-launch kernels take): pinned, mapped staging the
	// kernel reads and writes over PCIe itself -- one launch and one synchronisation instead of two copies around them.
	char *hstage = nullptr, *hstage_dev = nullptr;
	static constexpr size_t HSTAGE_BYTES = 5 * (size_t)SMALL_SORT_BYTES;   // keys, keys, and two halves of 8-byte indices

	bool fast = false;           // rsx_scatter2_kernel allowed on this device (LDS atomic order verified)
	// The reference is re-entrant (concurrent calls on disjoint buffers are safe); here calls that share a context
	// (same device and stream) share its workspace, so every entry point holds this for its duration.
	std::recursive_mutex mu;

	// The library's own contexts hold TWO sets of flags and histograms and alternate between them (`gen`): small sorts zero
	// the set of the next sort inside this sort's histogram kernel instead of launching a kernel for it (plan_phase).  A
	// context in a caller's workspace (external) has one set.
	// A THIRD set (ASYNC_SET) belongs to the device-scheduled sorts (*_inplace_async, rsx_msd_split_async: AsyncSetScope): a
	// graph captured from one keeps the addresses it was enqueued with and may be replayed between any two blocking sorts
	// without the host seeing it, so it must never count into a set that a blocking sort trusts to be zero.
	u32 gen = 0;
	static constexpr u32 ASYNC_SET = 2, SETS = 3;
	static constexpr size_t SMALL_BYTES = WS_FLAGS_BYTES, HIST_SET_BYTES = 8 * 256 * sizeof(u64);
	char *small_set() const { return (char *)small.p + (small.external ? 0 : gen * SMALL_BYTES); }
	char *small_set_other() const { return (char *)small.p + (gen ^ 1u) * SMALL_BYTES; }
	u64 *ghist() const { return (u64 *)((char *)hist.p + (hist.external ? 0 : gen * HIST_SET_BYTES)); }
	u64 *ghist_other() const { return (u64 *)((char *)hist.p + (gen ^ 1u) * HIST_SET_BYTES); }
	u32 *unsorted() const { return (u32 *)small_set(); }
	u32 *plan_done() const { return (u32 *)(small_set() + 52); }   // blocks of rsx_plan_kernel that are through
	u64 *verify_bad() const { return (u64 *)(small_set() + 56); }  // RSX_VERIFY: mismatches found by rsx_verify_tile_kernel
	u32 *hotd() const { return (u32 *)(small_set() + 16); }   // [8] hot digits per column + [1] valid bits (rsx_plan_kernel)
	Plan *plan() const { return (Plan *)(small_set() + WS_PLAN_OFF); }   // (a caller's workspace: WsLayout::plan_off)
	// ... of the last device-scheduled sort of this context (rsx_async_route), whatever the blocking sorts have done since
	const Plan *async_plan() const { return (const Plan *)((char *)small.p + (small.external ? 0 : ASYNC_SET * SMALL_BYTES) + WS_PLAN_OFF); }
	u32 *kept() const { return (u32 *)(small_set() + 128); }
	u32 *colmax() const { return (u32 *)(small_set() + 192); }   // [8] largest bin per column (rsx_plan_kernel, kept[16..])

	int init()
	{
		RSX_TRY(small.ensure(SETS * SMALL_BYTES));
		RSX_TRY(hist.ensure(SETS * HIST_SET_BYTES));
		RSX_TRY(gscan.ensure(256 * sizeof(u64)));
		HIP_TRY(hipMemset(small.p, 0, SETS * SMALL_BYTES));   // (the alternating sets start out zeroed: see `gen`)
		HIP_TRY(hipMemset(hist.p, 0, SETS * HIST_SET_BYTES));
		if (!host_plan)
		{
			HIP_TRY(hipHostMalloc((void **)&host_plan, sizeof(Plan), hipHostMallocMapped));
			HIP_TRY(hipHostGetDevicePointer((void **)&dev_host_plan, host_plan, 0));
		}
		if (!host_hist)
			HIP_TRY(hipHostMalloc((void **)&host_hist, 256 * sizeof(u64), hipHostMallocDefault));
		if (!host_segctl) {
			HIP_TRY(hipHostMalloc((void **)&host_segctl, sizeof(SegCtl), hipHostMallocMapped));
			HIP_TRY(hipHostGetDevicePointer((void **)&dev_host_segctl, host_segctl, 0));
		}
		return RSX_OK;
	}
	int ensure_hstage()
	{
		if (!hstage) {
			HIP_TRY(hipHostMalloc((void **)&hstage, HSTAGE_BYTES, hipHostMallocMapped));
			HIP_TRY(hipHostGetDevicePointer((void **)&hstage_dev, hstage, 0));
		}
		return RSX_OK;
	}
	int ensure_segplan()
	{
		if (!host_segplan) {
			HIP_TRY(hipHostMalloc((void **)&host_segplan, sizeof(SegmentsPlan), hipHostMallocMapped));
			HIP_TRY(hipHostGetDevicePointer((void **)&dev_host_segplan, host_segplan, 0));
		}
		return RSX_OK;
	}
	void release()
	{
		if (hstage)
			(void)hipHostFree(hstage);
		hstage = hstage_dev = nullptr;
		small.release();
		hist.release();
		hpart.release();
		status.release();
		for (int i = 0; i < 2; ++i) {
			keys[i].release();
			vals[i].release();
			recs[i].release();
		}
		stage.release();
		tkeys.release();
		ckeys.release();
		joint.release();
		seg.release();
		slack.release();
		slack1.release();
		logb.release();
		logslots.release();
		ubits.release();
		urecs.release();
		gcells.release();
		rdtab.release();
		tkctl.release();
		tkpairs.release();
		tkcand.release();
		nthctl.release();
		nthcand.release();
		nthio.release();
		loctab.release();
		locvals.release();
		rcells.release();
		jointab.release();
		joinkeys.release();
		joinidx.release();
		jointiles.release();
		lexkeys.release();
		lexidx.release();
		parttab.release();
		partvals.release();
		partidx.release();
		segtab.release();
		segwork.release();
		if (host_segplan)
			(void)hipHostFree(host_segplan);
		host_segplan = dev_host_segplan = nullptr;
		if (host_logctl)
			(void)hipHostFree(host_logctl);
		host_logctl = nullptr;
		if (log_ev)
			(void)hipEventDestroy(log_ev);
		log_ev = nullptr;
		slack1_v.release();
		slack_v.release();
		vasync.release();
		vsum.release();
		gscan.release();
		if (host_segctl)
			(void)hipHostFree(host_segctl);
		host_segctl = dev_host_segctl = nullptr;
		if (seg_ev)
			(void)hipEventDestroy(seg_ev);
		seg_ev = nullptr;
		if (plan_ev)
			(void)hipEventDestroy(plan_ev);
		plan_ev = nullptr;
		if (host_plan)
			(void)hipHostFree(host_plan);
		if (host_hist)
			(void)hipHostFree(host_hist);
		host_plan = nullptr;
		host_hist = nullptr;
	}
};

// ... for the duration of a device-scheduled entry point on one of the library's own contexts (held under the context's mutex):
// every accessor above then names the third set, and `gen` is what it was when the call returns
struct AsyncSetScope {
	Ctx &c;
	u32 prev;
	explicit AsyncSetScope(Ctx &c_) : c(c_), prev(c_.gen) { c.gen = Ctx::ASYNC_SET; }
	~AsyncSetScope() { c.gen = prev; }
	AsyncSetScope(const AsyncSetScope &) = delete;
	AsyncSetScope &operator=(const AsyncSetScope &) = delete;
};

std::mutex g_mu;
std::map<std::pair<int, void *>, Ctx *> g_ctx;
std::map<int, int> g_lds_order_ok;   // device -> result of lds_order_selfcheck (1 ok, 0 not)

// ---- RSX_HOST_REGISTER=1 (a measurement switch): the caller's host buffers are page-locked (hipHostRegister) FOR THE
// DURATION OF THE CALL, so that the copies go by DMA straight from / to them instead of through the runtime's bounce buffers.
// (Round 2 kept registrations cached per pointer across calls: a buffer freed and reallocated at the same address then
// reused a stale mapping, and evicting an entry could pull the registration from under another thread's copy.  Measured
// gain of keeping buffers registered: 1-2 %; a caller that wants it registers its own buffers with
// hipHostRegister -- the library copies from registered memory as it finds it.)
struct HostRegScope {
	void *p = nullptr;
	HostRegScope(void *ptr, size_t bytes)
	{
		if (!env().host_register || bytes < ((size_t)1 << 20))
			return;
		if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess)
			p = ptr;
		(void)hipGetLastError();   // (a buffer that cannot be registered -- or already is -- is copied as it is)
	}
	~HostRegScope()
	{
		if (p)
			(void)hipHostUnregister(p);
	}
	HostRegScope(const HostRegScope &) = delete;
	HostRegScope &operator=(const HostRegScope &) = delete;
};

// ---- optional HIP-event bracketing of the kernels (rsx_profile_begin/end) ------
struct ProfRec {
	int kind;   // 0 histogram, 1 scatter, 2 leaves (rsx_hybrid.hpp), 3 passes that write narrowed keys into slots
	hipEvent_t start, stop;
	u64 bytes;
	hipStream_t stream;
	bool called_off;   // launches of an attempt the device called off (or of a route the plan did not choose): they returned at
	                   // once or their output was discarded -- their time is booked apart, their bytes are not booked at all
	// device-scheduled sorts (rsx_sort_inplace_async): nobody reads a verdict back while the sort is enqueued, so the record names
	// a pinned word that receives SegCtl::mode behind the attempt (prof_verdict_slot) and which value makes it count:
	// valid_if 1 -- the attempt's own launches: SEG_MODE_LEAVES; 2 -- the gated histogram-first launches behind it: anything else
	const u32 *verdict = nullptr;
	int valid_if = 0;
};
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;

// What a sort books is what the DEVICE chose.  Kernels are enqueued before the host knows the route (a sort without a histogram
// may be called off by its sample; leaves are launched in every shape the plan may ask for); once the host has the verdict it
// takes the records of the launches that did nothing out of the byte count (prof_called_off) or corrects their bytes
// (prof_rebook: 8-byte keys whose level-2 slots the sample narrowed to four bytes).  prof_mark() = where this call's records start.
size_t prof_mark()
{
	if (!g_prof_on)
		return 0;
	std::lock_guard<std::mutex> lock(g_prof_mu);
	return g_prof.size();
}
void prof_called_off(size_t mark, hipStream_t s, int kind = -1)
{
	if (!g_prof_on)
		return;
	std::lock_guard<std::mutex> lock(g_prof_mu);
	for (size_t i = mark; i < g_prof.size(); ++i)
		if (g_prof[i].stream == s && (kind < 0 || g_prof[i].kind == kind))
			g_prof[i].called_off = true;
}
// (the LAST record of `kind` since the mark: a sort's level-1 and level-2 passes are both kind 1, in that order)
void prof_rebook(size_t mark, hipStream_t s, int kind, u64 bytes, int new_kind = -1)
{
	if (!g_prof_on)
		return;
	std::lock_guard<std::mutex> lock(g_prof_mu);
	for (size_t i = g_prof.size(); i > mark; --i)
		if (g_prof[i - 1].stream == s && g_prof[i - 1].kind == kind && !g_prof[i - 1].called_off) {
			g_prof[i - 1].bytes = bytes;
			if (new_kind >= 0)
				g_prof[i - 1].kind = new_kind;
			break;
		}
}

// a pinned word for one device-scheduled sort's verdict (4096 per profile window; none left: the records stay as they are)
u32 *g_prof_vblock = nullptr;
size_t g_prof_vnext = 0;
u32 *prof_verdict_slot()
{
	std::lock_guard<std::mutex> lock(g_prof_mu);
	if (!g_prof_vblock && hipHostMalloc((void **)&g_prof_vblock, 4096 * sizeof(u32), hipHostMallocDefault) != hipSuccess) {
		(void)hipGetLastError();
		g_prof_vblock = nullptr;
		return nullptr;
	}
	if (g_prof_vnext >= 4096)
		return nullptr;
	u32 *p = g_prof_vblock + g_prof_vnext++;
	*p = 0;
	return p;
}
void prof_tag(size_t from, size_t to, hipStream_t s, const u32 *verdict, int valid_if)
{
	std::lock_guard<std::mutex> lock(g_prof_mu);
	for (size_t i = from; i < to && i < g_prof.size(); ++i)
		if (g_prof[i].stream == s) {
			g_prof[i].verdict = verdict;
			g_prof[i].valid_if = valid_if;
		}
}
// ... around the attempt and the gated launches of a device-scheduled sort (`attempted`: an attempt was enqueued at all)
struct ProfAsyncVerdict {
	size_t m0 = 0, m1 = 0;
	u32 *slot = nullptr;
	hipStream_t stream;
	explicit ProfAsyncVerdict(hipStream_t s) : stream(s) { m0 = prof_mark(); }
	void attempt_enqueued(const SegCtl *ctl)
	{
		if (!g_prof_on)
			return;
		slot = prof_verdict_slot();
		if (slot && hipMemcpyAsync(slot, &ctl->mode, sizeof(u32), hipMemcpyDeviceToHost, stream) != hipSuccess) {
			(void)hipGetLastError();
			slot = nullptr;
		}
		m1 = prof_mark();
	}
	void gated_enqueued()
	{
		if (!g_prof_on || !slot)
			return;
		const size_t m2 = prof_mark();
		prof_tag(m0, m1, stream, slot, 1);
		prof_tag(m1, m2, stream, slot, 2);
	}
};

struct ProfScope {
	bool on;
	ProfRec rec;
	hipStream_t stream;
	ProfScope(int kind, u64 bytes, hipStream_t s) : on(g_prof_on), stream(s)
	{
		if (!on)
			return;
		rec.kind = kind;
		rec.bytes = bytes;
		rec.stream = s;
		rec.called_off = false;
		if (hipEventCreate(&rec.start) != hipSuccess || hipEventCreate(&rec.stop) != hipSuccess) {
			on = false;
			return;
		}
		(void)hipEventRecord(rec.start, stream);
	}
	~ProfScope()
	{
		if (!on)
			return;
		(void)hipEventRecord(rec.stop, stream);
		std::lock_guard<std::mutex> lock(g_prof_mu);
		g_prof.push_back(rec);
	}
};
int g_devcount = -2;   // -2: not probed

int probe_devices()
{
	if (g_devcount != -2)
		return g_devcount;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		n = 0;
	}
	int usable = 0;
	for (int d = 0; d < n; ++d) {
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
			++usable;
		else
			(void)hipGetLastError();
	}
	g_devcount = usable;
	return usable;
}

// rsx_scatter2_kernel ranks keys with returning LDS atomics and needs them to resolve same-address lanes
// in lane order.  gfx950 does, but that is an observed property, not a documented one: verify it once
// per device (about a millisecond) and otherwise stay on the table-based ranking of rsx_scatter_kernel.
int lds_order_selfcheck(int dev)
{
	auto it = g_lds_order_ok.find(dev);
	if (it != g_lds_order_ok.end())
		return it->second;
	int ok = 0;
	u64 *d_bad = nullptr;
	if (!env().force_table_rank && hipMalloc((void **)&d_bad, sizeof(u64)) == hipSuccess) {
		u64 bad = ~0ull;
		if (hipMemset(d_bad, 0, sizeof(u64)) == hipSuccess) {
			// two shapes: eight waves of bare atomics on collision-heavy digits, and the production shape of
			// rsx_scatter2_kernel (16 waves, eight atomics in flight, staging stores and 16-byte rows between them)
			hipLaunchKernelGGL(rsx_lds_order_check_kernel, dim3(1024), dim3(512), 0, 0, d_bad, 0x9E3779B9u, 512);
			hipLaunchKernelGGL(rsx_lds_order_check2_kernel, dim3(512), dim3(1024), 0, 0, d_bad, 0x85EBCA6Bu, 256);
			if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
			    hipMemcpy(&bad, d_bad, sizeof(u64), hipMemcpyDeviceToHost) == hipSuccess)
				ok = bad == 0;
		}
		(void)hipFree(d_bad);
	}
	(void)hipGetLastError();
	g_lds_order_ok[dev] = ok;
	return ok;
}

// ---- rsx_capture_histogram: the caller-supplied Hist of rs_sort_main (radix_sort.hpp:28-33) -------------------------
// Armed per thread; the next sort of that thread that runs the histogram kernels writes the raw per-column digit counts
// there (hist[256 j + d]) and disarms.  The counts are recovered from the exclusive offsets the plan kernel leaves in the
// workspace (every column is scanned, kept or not): count[d] = offset[d + 1] - offset[d], the last one n - offset[255].
thread_local u64 *g_capture_dst = nullptr;
thread_local size_t g_capture_entries = 0;

inline bool capture_armed() { return g_capture_dst != nullptr; }

int capture_hist(Ctx &c, size_t n, size_t kb)
{
	if (!g_capture_dst)
		return RSX_OK;
	u64 *dst = g_capture_dst;
	const size_t entries = g_capture_entries;
	g_capture_dst = nullptr;
	g_capture_entries = 0;
	if (entries < 256 * kb)
		return fail(RSX_EINVAL, "rsx_capture_histogram: room for %zu entries, the sort has %zu", entries, 256 * kb);
	std::vector<u64> off(256 * kb);
	HIP_TRY(hipMemcpyAsync(off.data(), c.ghist(), 256 * kb * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
	HIP_TRY(hipStreamSynchronize(c.stream));
	for (size_t j = 0; j < kb; ++j)
		for (size_t d = 0; d < 256; ++d)
			dst[256 * j + d] = (d == 255 ? (u64)n : off[256 * j + d + 1]) - off[256 * j + d];
	return RSX_OK;
}

// RSX_VERIFY=1 (read once per process): after every host-scheduled scatter pass of the fast kernel one pseudo-randomly
// chosen tile is re-ranked without LDS atomics (rsx_verify_tile_kernel) and compared with what the pass wrote; a
// mismatch fails the call with RSX_EVERIFY.  Passes are then serialised by the check's read-back and no pass is
// speculative; the *_inplace_async entry points, which never synchronise, are not verified.
bool verify_mode() { return env().verify; }
u32 g_verify_seq = 0;

int get_ctx(void *stream, Ctx **out)
{
	std::lock_guard<std::mutex> lock(g_mu);
	if (probe_devices() <= 0)
		return fail(RSX_ENODEVICE, "no gfx950 (MI355X) device visible to HIP; this library has no CPU path");
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	auto key = std::make_pair(dev, stream);
	auto it = g_ctx.find(key);
	if (it == g_ctx.end()) {
		Ctx *c = new Ctx();
		c->device = dev;
		c->stream = (hipStream_t)stream;
		c->fast = lds_order_selfcheck(dev) != 0;
		int rc = c->init();
		if (rc != RSX_OK) {
			c->release();
			delete c;
			return rc;
		}
		it = g_ctx.emplace(key, c).first;
	}
	*out = it->second;
	return RSX_OK;
}

void info_clear(rsx_info *info, int dtype)
{
	if (!info)
		return;
	memset(info, 0, sizeof(*info));
	info->key_bytes = (uint32_t)dtype_size(dtype);
}

void info_from_plan(rsx_info *info, const Plan &p)
{
	if (!info)
		return;
	info->ncols = p.ncols;
	for (u32 i = 0; i < p.ncols && i < 8; ++i)
		info->cols[i] = p.cols[i];
}

}  // namespace
