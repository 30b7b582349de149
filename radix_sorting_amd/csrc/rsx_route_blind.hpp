// rsx_route_blind.hpp: the sorts WITHOUT a histogram -- their gates and back-off, their sizes, the attempt for keys alone
// (blind_enqueue, sort_keys_blind) and for (key, payload) and rank sorts (pairs_blind_enqueue, pairs_blind); part of librsx.so's
// host side, included by rsx.hip behind rsx_route_levels.hpp, ahead of the drivers.
#pragma once

namespace {

// ---- two MSB passes and leaves WITHOUT the histogram (rsx_hybrid.hpp, rsx_blind_precheck_kernel) -----------------------------
// For the arrays a two-level sort is for (hybrid_caps: cap2), blocking keys-only sorts.  *done = 1: sorted, *result set.
// *done = 0: called off (the sample did not prove what it has to, or a slot overflowed) -- `src` and `aux` are untouched and
// the caller runs the ordinary path.  A context that has been called off skips the next attempts of its kind (1, 3, 7 ... 31 sorts).
// kinds of sorts that learn separately: 0 / 1 keys only (4- / 8-byte keys), 2 rank sorts, 3 key + payload sorts
template <typename KT> constexpr int blind_kind(size_t payload_bytes, bool rank = false)
{
	return payload_bytes ? (rank ? 2 : 3) : (sizeof(KT) == 8 ? 1 : 0);
}
// may this context try a sort without a histogram at all?  (allow_ws_blind: a context in a caller's workspace may, if the workspace
// was sized for the slots as well -- rsx_workspace_bytes_fast, the device-scheduled keys-only sort)
inline bool blind_gate(const Ctx &c, bool allow_ws_blind = false)
{
	return !(env().no_blind || env().no_slack || !hybrid_enabled() || !c.fast || capture_armed() || verify_mode() ||
	         (c.small.external && !(allow_ws_blind && c.ws_blind)) || env().no_speculation);
}
inline void blind_called_off(Ctx &c, int kind)
{
	c.blind_backoff[kind] = std::min<u32>(2 * c.blind_backoff[kind] + 1, 31);
	c.blind_skip[kind] = c.blind_backoff[kind];
}
// rsx_reload_env() makes every context forget what it has learnt about its inputs (and about its device's memory)
inline void blind_refresh(Ctx &c)
{
	const u32 epoch = g_env_epoch.load();
	if (c.env_epoch != epoch) {
		c.env_epoch = epoch;
		c.blind_no_room = false;
		for (int k = 0; k < 4; ++k)
			c.blind_skip[k] = c.blind_backoff[k] = 0;
		c.log_skip = c.log_backoff = 0;
		c.boff_forget = true;   // (... and the device-side one of the device-scheduled sorts, SegCtl::boff_*: zeroed by the next attempt)
	}
}
// rsx_reload_env: the context forgets the attempts it lost -- the host's counters above, the device's here (in front of the sample kernel)
inline int blind_forget_device_backoff(Ctx &c)
{
	if (c.boff_forget && c.seg.p) {
		HIP_TRY(hipMemsetAsync(&SegView(c).ctl()->boff_skip, 0, 2 * sizeof(u32), c.stream));
		c.boff_forget = false;
	}
	return RSX_OK;
}
// Where the keys-only sorts without a histogram end: 2^30 keys (32-bit offsets in the leaf and tile tables; level-2 slots of more
// than 32 Ki whole keys have no leaf) -- or, 4-byte keys in two-byte slots (rsx_leafc.hpp: slots of up to 40960 values), where the
// mean level-2 slot passes 32 Ki: 2^31 + 65536 keys.  Every offset of such a sort still fits 32 bits: 257 level-1 slots of
// 1.25 x 2^23 keys, 65537 level-2 slots of 40960 values, positions below 2^32.
template <typename KT> size_t blind_keys_end()
{
	if (sizeof(KT) == 4 && dense_cap_max<KT>() >= LEAFC_CAP)
		return (size_t)32769 << 16;
	return (size_t)1 << 30;
}
template <typename KT> bool blind_wanted(Ctx &c, size_t n, size_t payload_bytes = 0, bool rank = false)
{
	if constexpr (sizeof(KT) < 4)
		return false;
	if (!blind_gate(c))
		return false;
	if (n < ((size_t)1 << 22) || n >= (payload_bytes || rank ? (size_t)1 << 30 : blind_keys_end<KT>()))
		return false;
	if (payload_bytes) {
		// 4-byte keys with 4-byte payloads, 16 Mi .. 2^28 pairs.  Round 3: from 96 Mi (one leaf shape, 5120 pairs, whose fixed
		// costs made 16 Mi pairs cost 0.63 ms); with the leaves' three shapes (pairs_blind) -- f32 keys -> ranks / pairs, ms,
		// against one pass per column: 16 Mi 0.271 / 0.273 against 0.271 / 0.299, 32 Mi 0.41 / 0.44 against 0.47 / 0.52, 64 Mi
		// 0.68 / 0.74 against 0.84 / 1.00, 2^27 1.21 / 1.33 (round 3's shape: 1.54 / 1.63)
		// (tools/rank_threshold_probe.py, profiles/r04/rank_threshold_probe.txt); a lower RSX_TWO_LEVEL_MIN_LOG2 (tests) lowers the floor
		// With a wave per leaf for slots of up to 256 / 512 pairs (LeafKCfg<64, 256, 8, 9>, <64, 512, 8, 10>): from 4 Mi pairs -- 8 Mi 0.169 / 0.170 against
		// 0.176 / 0.177 ms, 10 Mi 0.180 / 0.186 against 0.229 / 0.233, 12 Mi 0.194 / 0.201 against 0.240 / 0.248.
		// Round 6: up to 2^29 pairs (slots of 10240 pairs: LeafKCfg<1024, 10240, 4, 13>, fourteen position bits)
		if (sizeof(KT) != 4 || payload_bytes != 4 || n > ((size_t)1 << 29) ||
		    n < std::min((size_t)1 << 22, (size_t)1 << env().two_level_min_log2))   // (4 Mi: 140 against 151 us, 6 Mi 148 against 161)
			return false;
	} else {
		// keys only: without the histogram two levels beat one pass per column earlier than with it.  8-byte keys from 4.5 Mi
		// keys on (a wave per leaf for slots of up to 256 keys, LeafKCfg<64, 256, 8, 9>: 5 Mi 204 against 278 us, 7 Mi 219 against
		// 322, 8 Mi 234 where 128 threads per leaf took 284; five kept columns: 4 Mi 172 against 167, 5 Mi 184 against 207;
		// one level reaches 3-4 Mi keys: tools/u64_small_probe.py), before that from 8 Mi
		// keys on since their leaves come in three shapes (launch_leaves; one shape: from 48 Mi) -- uniform keys 8 Mi 0.287
		// against 0.347 ms, 16 Mi 0.386 against 0.605, 32 Mi 0.58 against 1.18, 64 Mi 0.93 against 2.15; five kept columns: 8 Mi
		// level, 16 Mi 0.337 against 0.404 (tools/u64_threshold_probe.py, profiles/r04/u64_threshold_probe.txt).
		// 4-byte keys, round 4 (their leaves read two-byte slots and are one wave's -- or a row of sixteen lanes' -- work up to
		// 1024 values, rsx_leaf16w_kernel / rsx_leaf16q_kernel): from 7.5 Mi keys (8 Mi 128 against 137 us, tools/size_sweep.py)
		size_t floor_keys = sizeof(KT) == 8 ? (size_t)9 << 19 : (size_t)15 << 19;
		if (env().blind_min_log2)
			floor_keys = (size_t)1 << env().blind_min_log2;
		floor_keys = std::min(floor_keys, (size_t)1 << env().two_level_min_log2);
		if (n < floor_keys)
			return false;
	}
	blind_refresh(c);
	const int kind = blind_kind<KT>(payload_bytes, rank);
	if (c.blind_skip[kind]) {
		--c.blind_skip[kind];
		return false;
	}
	return true;
}

// The device's part: the sample, both passes, the tables and the leaves, enqueued; *enqueued = 0: no room for the slots (or no
// leaf shape for them): nothing was enqueued.  Nothing waits for the host; SegCtl::mode == SEG_MODE_LEAVES (and the pinned
// copy the slack plan writes) says afterwards whether the sort went through.
// ... for a device-scheduled sort (rsx_sort_inplace_async): the same sizes; its back-off lives on the device (SegCtl::boff_skip: nothing is ever read back)
template <typename KT> bool async_blind_ok(Ctx &c, size_t n)
{
	if constexpr (sizeof(KT) < 4)
		return false;
	// (a caller's workspace: only one that was sized for the slots as well, rsx_workspace_bytes_fast)
	if (!blind_gate(c, true))
		return false;
	// (blind_wanted's floors, except that 4-byte keys start at 9 Mi here: at 8 Mi the empty launches of the gated histogram-first
	// kernels behind the attempt make it 153 us against 138 for one pass per column; the blocking sort: 127 against 135-139)
	size_t floor_keys = sizeof(KT) == 8 ? (size_t)1 << 23 : (size_t)9 << 20;
	if (env().blind_min_log2)
		floor_keys = (size_t)1 << env().blind_min_log2;
	floor_keys = std::min(floor_keys, (size_t)1 << env().two_level_min_log2);
	blind_refresh(c);
	return n >= std::max(floor_keys, (size_t)1 << 22) && n < (c.ws_blind ? (size_t)1 << 30 : blind_keys_end<KT>());
}
// ... for key + payload and rank sorts (4-byte keys, 4-byte payloads: blind_wanted's window, without its back-off)
template <typename KT> bool async_pairs_blind_ok(Ctx &c, size_t n, size_t payload_bytes)
{
	if (sizeof(KT) != 4 || payload_bytes != 4)
		return false;
	if (!blind_gate(c))
		return false;
	blind_refresh(c);
	return n >= std::min((size_t)1 << 24, (size_t)1 << env().two_level_min_log2) && n >= ((size_t)1 << 22) && n <= ((size_t)1 << 29);
}

// No room for the slots: the ordinary path, now and for this context's later sorts (a multi-GiB hipMalloc that fails is not worth
// repeating per sort); what was allocated of `bufs` goes back -- unless this is a device-scheduled sort (AsyncScope): a graph
// captured earlier may name the old arrays, so nothing is released and nothing is remembered
template <typename... Bufs> void blind_give_up_room(Ctx &c, Bufs &...bufs)
{
	(void)hipGetLastError();
	c.slack1_cap = c.slack_cap = 0;
	if (!g_in_async) {
		(bufs.release(), ...);
		c.blind_no_room = true;
	}
}

template <typename KT>
int blind_enqueue(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, int *enqueued)
{
	typedef Sc2Cfg<KT, NoVal> C2;
	*enqueued = 0;
	const u32 mean1 = (u32)(n >> 8), mean2 = (u32)(n >> 16);
	const u32 cap1 = level1_slot_cap<KT>(mean1);
	const u32 cap2 = slot_cap_for(mean2);
	if (cap2 > std::max((u32)LeafShapes<KT>::Big::CAP, dense_cap_max<KT>()))
		return RSX_OK;
	if (c.blind_no_room)
		return RSX_OK;
	// Where the level-1 slots lie.  The attempt only writes after its sample has PROVEN the input unsorted and four columns kept
	// -- from then on the caller's second buffer belongs to the sort whatever route finishes it (radix_sort.hpp:60-62 keeps it
	// untouched only on the early exits) -- so the slots that fit there (n / cap1 of them: 204 of 256) lie there and the library
	// allocates the rest only: 0.25 n keys instead of 1.25 n (2^28 u32 keys: 0.25 GiB + 0.63 GiB of two-byte level-2 slots
	// instead of 1.25 + 1.25).  Needs a slot that holds a tile (a lost attempt's runs go over the slot's own beginning there,
	// rsx_scatter2.hpp); RSX_NO_AUX_SLOTS=1: all slots in scratch memory.
	u32 lo = (aux && !env().no_aux_slots && cap1 >= (u32)C2::TILE) ? (u32)std::min<size_t>(n / cap1, 255) : 0u;
	c.slack_cap = cap2;   // (dense_slots asks for it)
	c.slack_mean = mean2;
	const size_t slot2_bytes = dense_slots<KT>(c) ? 2 : sizeof(KT);
	if (c.slack1.ensure(((size_t)(256 - lo) * cap1 + C2::TILE) * sizeof(KT)) != RSX_OK ||
	    c.slack.ensure(((size_t)65536 * cap2 + C2::TILE) * slot2_bytes) != RSX_OK) {
		blind_give_up_room(c, c.slack1, c.slack);
		return RSX_OK;
	}
	// the level-1 pass reaches both parts with 32-bit element offsets from the lower one (rsx_scatter2.hpp, SegArgs): they
	// must lie within 2^32 elements of each other, the dump area behind the last slot included -- else everything in scratch
	if (lo && !SlotParts(aux, c.slack1.p, lo, cap1, sizeof(KT), C2::TILE).fits32()) {
		lo = 0;
		if (c.slack1.ensure(((size_t)256 * cap1 + C2::TILE) * sizeof(KT)) != RSX_OK) {
			blind_give_up_room(c, c.slack1, c.slack);
			return RSX_OK;
		}
	}
	c.slack1_lo = lo;
	RSX_TRY(seg_layout<KT>(c, n));
	RSX_TRY(c.gscan.ensure(256 * sizeof(u64)));
	const SegView sv(c);
	const u64 ntiles0 = sv.L.rows - seg_extra_rows<KT>();   // (the level-1 pass's tiles: no partial ones)
	SegCtl *ctl = sv.ctl();
	SegTile *tiles = sv.tiles();
	LeafSeg *segtab = sv.segtab();
	u32 *btile = sv.btile();
	u64 *off1 = (u64 *)c.gscan.p;
	// (a context in a caller's workspace has neither a pinned control block nor an event: nobody reads a verdict there)
	if (!c.seg_ev && !c.small.external)
		HIP_TRY(hipEventCreateWithFlags(&c.seg_ev, hipEventDisableTiming));
	if (c.host_segctl)
		c.host_segctl->mode = SEG_MODE_NONE;
	c.slack1_cap = cap1;
	c.slack_cap = cap2;
	// 4-byte keys from 64 Mi keys on: the level-1 pass in whole 64-byte atoms (rsx_pass32a_kernel: a workgroup per CU takes a range
	// of tiles and carries what does not fill an atom; a bucket then lies at both ends of its slot)
	const bool atoms = pass16a_wanted<KT>(c);   // (the level-2 pass that writes whole atoms: smaller tiles, two cursors per slot)
	const bool atoms64 = pass64a_narrow_wanted<KT>(c);   // (8-byte keys: the same for the form that writes four-byte slots; the sample decides which form runs)
	typedef Pass32aCfgT<sizeof(KT) == 8 ? 14 : 28> P32;
	const size_t min32 = env().pass32_min_mi ? (size_t)env().pass32_min_mi << 20 : sizeof(KT) == 8 ? (size_t)3 << 23 : (size_t)13 << 22;
	const bool atoms1 = (sizeof(KT) == 4 ? atoms : !env().no_unstable) && !env().no_pass32a && n >= min32 &&
	                    cap1 >= (u32)P32::TILE + 2 * PASS32_BACK;
	// (keys the caller says arrive in order of their top digit, piece by piece: four counters per digit, rsx_pass32.hpp)
	const bool rep4 = (c.hints & 1u) != 0 || (env().probe & 4u) != 0;
	// 8-byte keys in which nothing below the level-1 digit varies above bit 32 (keys below 2^40: BASELINE.json's cfg 3 (ii), (iii)):
	// the level-1 slots can hold low words -- all 256 of them then fit the caller's second buffer -- and the level-2 pass reads four
	// bytes per key.  Both atom passes in both forms are enqueued; the sample decides (SegCtl::narrow == 2).  The 256 slots of cap1
	// four-byte places must fit the caller's n keys (a larger cap1 -- RSX_CAP1_PAD_KIB -- would write past its end).
	c.narrow1 = sizeof(KT) == 8 && atoms1 && atoms64 && lo != 0 && !rep4 && !env().no_narrow1 && (((uintptr_t)aux) & 63) == 0 &&
	            (size_t)256 * cap1 * 4 <= n * sizeof(KT);
	// the sample (workgroup 0: control block, plan) and the zeroing of both passes' status words, one launch
	static_assert(sizeof(SegCtl) <= 256, "the control block is not part of what is zeroed");
	RSX_TRY(blind_forget_device_backoff(c));
	hipLaunchKernelGGL((rsx_blind_precheck_kernel<KT>), dim3(1 + 512), dim3(1024), 0, c.stream, (const KT *)src, (u64)n, ka, ctl,
	                   c.plan(), c.dev_host_plan, (u32x4 *)sv.status(0), (u64)(2 * sv.L.st_bytes / 16),
	                   4u,   // (two levels want four kept columns: two for the passes, two or more for the leaves)
	                   // 4-byte keys whose leaves read two-byte slots (rsx_leaf16.hpp): the MSB digits may lie below constant top bits
	                   (u32)(sizeof(KT) == 4 && dense_slots<KT>(c) && !env().no_leaf16 && !env().no_shift ? 1 : 0),
	                   // 8-byte keys in slots rsx_leafk_kernel takes: four-byte slots where the leaves' columns lie in the low word
	                   (u32)(narrow_slots_ok<KT>(cap2) ? (c.narrow1 ? 2 : 1) : 0), 0u,
	                   // a device-scheduled sort keeps its back-off on the device (SegCtl::boff_skip); the blocking sorts keep theirs on the host
	                   (u32)(g_in_async ? 1 : 0), (u32)((env().probe & 4u) ? 1u : c.hints));
	{
		// 4-byte keys: only in front of rsx_pass16a_kernel (a bucket that lies at both ends of its slot is one tile more: that pass's
		// tile table has room for it); from 52 Mi keys, where that pass starts for good -- as first built (the next tile requested
		// ahead, two LDS atomics per key) it was level with the chained pass at 64-80 Mi and 1 % ahead at 96 Mi
		// (profiles/r05/atoms_threshold_probe.txt); as it is now: 0-4 % ahead at 54 .. 95 Mi keys, never behind
		// (tools/ab_sizes.py RSX_PASS32_MIN_MI 96 40 u32 ...), 2-5 % behind in the 1024-value-slot window around 40 Mi.
		// 8-byte keys (atoms of eight keys, 14 Ki-key tiles): in front of the CHAINED level-2 pass, whose status words have a row
		// more per bucket for that (seg_extra_rows); from 24 Mi keys (1.3-2.5 % ahead at 24 .. 44 Mi, level at 20 Mi:
		// tools/ab_sizes.py RSX_PASS32_MIN_MI 48 16 u64 ...) -- tools/ubench/pass32_probe, 2^28 u64 keys: 0.926 ms against 1.01 for
		// the chained pass, 2^27: 0.447 against 0.50.
		if (atoms1) {
			// one base for the stores, the parts' offsets in the slots' places (as launch_seg_pass does for the chained pass)
			const SlotParts parts(aux, c.slack1.p, lo, cap1, sizeof(KT), C2::TILE);   // (lo == 0: the scratch array, no offsets)
			KT *kbase = (KT *)parts.base;
			const u32 off_lo = parts.off_lo, off_hi = parts.off_hi;
			u32 *cur1 = sv.cursors(1);
			u32 *ovf = &ctl->overflow;
			const bool plain = ka.fmask == 0 && ka.sflip == 0 && ka.desc == 0;
			ProfScope prof(1, (u64)n * 2 * sizeof(KT), c.stream);
			// (probed and not kept: Pass32aCfgT<12> -- 12 Ki-key tiles, 81 KB of LDS, two workgroups per CU, no prefetch: 0.534-0.543 ms
			// for 2^28 keys where this shape takes 0.470-0.477 on the same box, profiles/r05/pass32a_probe.txt)
			// (the next tile's keys requested while this tile is written out: 1 % ahead at 2^27 keys, 2-5 % BEHIND from 2^28 on -- the
			// level-1 pass of 2^28 keys 0.485 -> 0.457 ms without, three rounds alternating in one process, tools/blind_ab.py;
			// 380 M keys 1.975 -> 1.929 ms, 2^30 5.157 -> 5.130: reads and writes in flight together cost more than the gap between tiles)
			// (8-byte keys: never ahead -- 2^27 keys 0.447 against 0.455 ms, 2^28 0.926 against 0.951)
			// (later, with one LDS atomic per key: never ahead at 54 .. 224 Mi keys either -- 54 Mi 0.340 -> 0.330 ms, 192 Mi 0.983 -> 0.961,
			// level at 80 and 128 Mi, tools/ab_sizes.py RSX_PASS32_PREFETCH 1 0 u32 ...: off unless RSX_PASS32_PREFETCH=1 asks for it)
			const bool prefetch = sizeof(KT) == 4 && env().pass32_prefetch > 0;
#define RSX_LAUNCH_P32R(DIGV, PF, REPV)                                                                                      \
			hipLaunchKernelGGL((rsx_pass32a_kernel<KT, DIGV, PF, P32, REPV>), dim3(256), dim3(P32::BLOCK), 0, c.stream,              \
			                   (const KT *)src, (u64)n, kbase, lo, off_lo, off_hi, cap1, (const SegCtl *)ctl, cur1, ovf, ka)
#define RSX_LAUNCH_P32(DIGV, PF)                                                                                             \
			do {                                                                                                                 \
				if (rep4 && !(PF))                                                                                               \
					RSX_LAUNCH_P32R(DIGV, false, 4);                                                                             \
				else                                                                                                             \
					RSX_LAUNCH_P32R(DIGV, PF, 1);                                                                                \
			} while (0)
			if constexpr (sizeof(KT) == 4) {
				if (plain && prefetch)
					RSX_LAUNCH_P32(DIG_PLAIN, true);
				else if (!plain && prefetch)
					RSX_LAUNCH_P32(DIG_GENERIC, true);
			}
			if (plain && !prefetch)
				RSX_LAUNCH_P32(DIG_PLAIN, false);
			else if (!prefetch)
				RSX_LAUNCH_P32(DIG_GENERIC, false);
#undef RSX_LAUNCH_P32
#undef RSX_LAUNCH_P32R
			if constexpr (sizeof(KT) == 8) {
				if (c.narrow1) {
					// ... and the form that writes low words: slot d = cap1 four-byte places at d x cap1 of the caller's second buffer
					if (plain)
						hipLaunchKernelGGL((rsx_pass32a_kernel<KT, DIG_PLAIN, false, P32, 1, u32>), dim3(256), dim3(P32::BLOCK), 0, c.stream,
						                   (const KT *)src, (u64)n, (u32 *)aux, 256u, 0u, 0u, cap1, (const SegCtl *)ctl, cur1, ovf, ka);
					else
						hipLaunchKernelGGL((rsx_pass32a_kernel<KT, DIG_GENERIC, false, P32, 1, u32>), dim3(256), dim3(P32::BLOCK), 0, c.stream,
						                   (const KT *)src, (u64)n, (u32 *)aux, 256u, 0u, 0u, cap1, (const SegCtl *)ctl, cur1, ovf, ka);
				}
			}
			HIP_TRY(hipGetLastError());
		}
	}
	if (!atoms1)
		RSX_TRY(launch_seg_pass<KT>(c, src, lo ? aux : nullptr, n, ka, -2, 1));
	hipLaunchKernelGGL(rsx_seg_tiles_kernel, dim3(32), dim3(256), 0, c.stream, (const u64 *)c.ghist(), (u64)n, (const Plan *)c.plan(),
	                   atoms ? (u32)Pass16aCfg::TILE : (u32)C2::TILE, tiles, ctl, btile, off1, cap1,
	                   (const u32 *)sv.cursors(1), (u32)ntiles0, atoms1 ? PASS32_BACK : 0u,
	                   atoms64 ? (u32)Pass2wCfg<u32>::TILE : 0u, c.narrow1 ? (u32)Pass64aCfgLow::TILE : 0u);
	RSX_TRY(launch_seg_pass<KT>(c, lo ? aux : nullptr, nullptr, n, ka, -2, 2));
	hipLaunchKernelGGL((rsx_seg_slack_plan_kernel<u32>), dim3(256), dim3(256), 0, c.stream,
	                   (const u32 *)sv.cursors(0), (const u32 *)btile, (const u64 *)c.ghist(),
	                   (const Plan *)c.plan(), ctl, segtab, cap2, c.dev_host_segctl, (const u64 *)off1,
	                   (atoms ? 2u : atoms64 ? 3u : 1u) | ((env().probe & 1u) << 8));
	HIP_TRY(hipGetLastError());
	if (c.seg_ev)
		HIP_TRY(hipEventRecord(c.seg_ev, c.stream));
	u32 leaf_shape = LeafShapes<KT>::shape_for_slots(cap2);
	if (dense_slots<KT>(c))
		leaf_shape |= 0x100u;   // (the leaves read 2-byte slots: the cut shapes have that variant)
	if (sizeof(KT) == 8 && cap2 <= 5120u)
		leaf_shape |= 0x200u;   // (8-byte keys in slots of up to 5120: rsx_leafk_kernel)
	RSX_TRY(launch_leaves<KT>(c, src, aux, n, ka, HYB_TWO_LEVEL, leaf_shape, (const u64 *)off1));
	*enqueued = 1;
	return RSX_OK;
}

// The blocking sorts' end of an attempt that was enqueued: the host waits for the verdict (the event lies behind the slack plan
// kernel, in front of the leaves).  *through = false: called off -- the context remembers it (blind_called_off: back-off) and the
// profile forgets the attempt's launches; true: the sort went through, the back-off of its kind starts over.
inline int blind_verdict(Ctx &c, int kind, size_t pmark, bool *through)
{
	HIP_TRY(hipEventSynchronize(c.seg_ev));
	*through = c.host_segctl->mode == SEG_MODE_LEAVES;
	if (*through) {
		c.blind_backoff[kind] = 0;
	} else {
		blind_called_off(c, kind);
		prof_called_off(pmark, c.stream);
	}
	return RSX_OK;
}

template <typename KT>
int sort_keys_blind(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, KT **result, rsx_info *info, int *done)
{
	*done = 0;
	int enqueued = 0;
	const size_t pmark = prof_mark();
	RSX_TRY(blind_enqueue<KT>(c, src, aux, n, ka, &enqueued));
	if (!enqueued)
		return RSX_OK;
	bool through = false;
	RSX_TRY(blind_verdict(c, blind_kind<KT>(0), pmark, &through));
	if (!through) {
		c.slack_cap = 0;
		return RSX_OK;
	}
	if (sizeof(KT) == 8 && c.host_segctl->narrow) {
		// the sample chose four-byte level-2 slots (SegCtl::narrow): the level-2 pass wrote 4 bytes per key, the leaves read 4
		// (narrow == 2: the level-1 slots hold four bytes per key too)
		const bool n1 = c.host_segctl->narrow == 2u;
		prof_rebook(pmark, c.stream, 2, (u64)n * (4 + sizeof(KT)));
		prof_rebook(pmark, c.stream, 1, (u64)n * ((n1 ? 4 : sizeof(KT)) + 4), 3);   // (the whole-key form of the level-2 pass returned at once)
		if (n1)
			prof_rebook(pmark, c.stream, 1, (u64)n * (sizeof(KT) + 4));            // (what is left of kind 1: the level-1 pass)
	}
	const Plan plan = *c.host_plan;
	info_from_plan(info, plan);
	KT *final = (plan.ncols & 1) ? aux : src;   // radix_sort.hpp:92
	*result = final;
	if (info) {
		info->result_in_aux = final == aux;
		info->hybrid = 5u;
	}
	*done = 1;
	return RSX_OK;
}

// What a sort of n keys WITHOUT a histogram needs on top of seg_bytes (blind_enqueue): the level-1 slots that do not fit the
// caller's second buffer, the level-2 slots, the control block / tables / status words of the two passes.
template <typename KT> WsBlind blind_sizes(size_t n)
{
	typedef Sc2Cfg<KT, NoVal> C2;
	const u32 cap1 = level1_slot_cap<KT>((u32)(n >> 8)), cap2 = slot_cap_for((u32)(n >> 16));
	const u32 lo = cap1 >= (u32)C2::TILE ? (u32)std::min<size_t>(n / cap1, 255) : 0u;
	const size_t slot2 = (sizeof(KT) == 4 && cap2 <= dense_cap_max<KT>()) ? 2 : sizeof(KT);
	WsBlind b;
	b.gscan = 256 * sizeof(u64);
	b.seg = ws_align256(seg_bytes<KT>(n));
	b.slack1 = ws_align256(((size_t)(256 - lo) * cap1 + C2::TILE) * sizeof(KT));
	b.slack = ws_align256(((size_t)65536 * cap2 + C2::TILE) * slot2);
	return b;
}

// ... handed to the context if the workspace has it (rsx_workspace_bytes_fast): the attempt is then made inside the workspace
inline void borrow_blind(Ctx &v, char *ws, size_t ws_bytes, const WsLayout &l)
{
	if (!l.blind_fits(ws_bytes))
		return;
	v.gscan.borrow(ws + l.gscan_off, l.blind.gscan);
	v.seg.borrow(ws + l.seg_off, l.blind.seg);
	v.slack1.borrow(ws + l.slack1_off, l.blind.slack1);
	v.slack.borrow(ws + l.slack_off, l.blind.slack);
	v.ws_blind = true;
}

// the pairs' LDS leaves over the two-byte key slots of c.slack / c.slack_v, in shape LC (redo: only the leaves of that list)
template <typename KT, typename VT, typename LC>
void launch_leaf_pairs16(Ctx &c, unsigned grid, u32 cap2, KT *kfinal, VT *vfinal, const LeafSeg *segtab, const SegCtl *ctl,
                         KdfArgs<KT> ka, const u32 *redo)
{
	hipLaunchKernelGGL((rsx_leaf_pairs_kernel<KT, VT, LC, true>), dim3(grid), dim3(LC::BLOCK), 0, c.stream, (const KT *)c.slack.p,
	                   (const VT *)c.slack_v.p, cap2, kfinal, vfinal, (const Plan *)c.plan(), segtab, ctl, ka, (u32)HYB_TWO_LEVEL,
	                   (const u64 *)nullptr, (u64)0, redo);
}

// Rank sorts and key + payload sorts without the histogram (sort_keys_blind's scheme with the (key, payload) pass kernel and
// the pairs' leaves): both MSB passes into slots -- the first reads the caller's (kin, vin), or makes the indices (vin ==
// nullptr) --, the leaves write to (kfinal, vfinal).  *done = 0: called off, nothing the caller owns has been written.
template <typename KT, typename VT>
int pairs_blind_enqueue(Ctx &c, const KT *kin, const VT *vin, KT *kfinal, VT *vfinal, size_t n, KdfArgs<KT> ka, int *enqueued,
                        KT *kspare = nullptr, VT *vspare = nullptr)
{
	typedef Sc2Cfg<KT, VT> C2;
	typedef LeafCfg<u32, 4, 20, 3> L;
	// The level-2 slots hold the low two bytes of what the level-2 pass reads (derived keys, or the packed keys of SegCtl::compact):
	// the two MSB passes have decided every bit above them, and no leaf ever looked at more of a key (rsx_leafp_kernel, K16)
	typedef unsigned short K2;
	static_assert(sizeof(KT) == 4, "two MSB digits above two bytes");
	*enqueued = 0;
	const u32 mean1 = (u32)(n >> 8), mean2 = (u32)(n >> 16);
	const u32 cap1 = slot_cap_for(mean1), cap2 = slot_cap_for(mean2);
	typedef LeafCfg<u32, 16, 12, 1> LB;          // ... and up to 12288 (slots of 10240 pairs: 2^28 .. 2^29 pairs), one workgroup per CU
	typedef LeafKCfg<1024, 10240, 4, 13> P10;   // the compound leaves' shape for those slots
	if (cap2 > (u32)P10::CAP)
		return RSX_OK;
	const bool big = cap2 > (u32)L::CAP || env().pairs_leaf_big;
	if (c.blind_no_room)
		return RSX_OK;
	// Where the level-1 slots lie (as blind_enqueue: nothing is written before the sample has proven the input unsorted and every
	// column kept, after which the caller's spare buffers belong to the sort whatever route finishes it).  `kspare` / `vspare`: n
	// elements each that the attempt may use -- the second key and payload buffers of a key + payload sort; of a rank sort the
	// two halves of its index buffer (the first for the indices until the leaves write it, the second, through which the
	// reference's passes ping-pong, for the 4-byte keys).  The slots that fit (n / cap1 of them: 204 of 256) lie there, the
	// others in scratch; keys and payloads split at the same slot, either spare buffer may be missing.
	u32 lo = (!env().no_aux_slots && cap1 >= (u32)C2::TILE && (kspare || vspare)) ? (u32)std::min<size_t>(n / cap1, 255) : 0u;
	for (int attempt = 0; attempt < 2; ++attempt) {
		const u32 klo = kspare ? lo : 0u, vlo = vspare ? lo : 0u;
		if (c.slack1.ensure(((size_t)(256 - klo) * cap1 + C2::TILE) * sizeof(KT)) != RSX_OK ||
		    c.slack1_v.ensure(((size_t)(256 - vlo) * cap1 + C2::TILE) * sizeof(VT)) != RSX_OK)
			break;   // (the test below sees it)
		// (both parts of either array within 2^32 elements of the lower one?)
		if (lo && ((klo && !SlotParts(kspare, c.slack1.p, lo, cap1, sizeof(KT), C2::TILE).fits32()) ||
		           (vlo && !SlotParts(vspare, c.slack1_v.p, lo, cap1, sizeof(VT), C2::TILE).fits32()))) {
			lo = 0;   // too far apart for 32-bit element offsets: all slots in scratch
			continue;
		}
		break;
	}
	const u32 klo = kspare ? lo : 0u, vlo = vspare ? lo : 0u;
	if (c.slack1.ensure(((size_t)(256 - klo) * cap1 + C2::TILE) * sizeof(KT)) != RSX_OK ||
	    c.slack1_v.ensure(((size_t)(256 - vlo) * cap1 + C2::TILE) * sizeof(VT)) != RSX_OK ||
	    c.slack.ensure(((size_t)65536 * cap2 + C2::TILE) * sizeof(K2)) != RSX_OK ||
	    c.slack_v.ensure(((size_t)65536 * cap2 + C2::TILE) * sizeof(VT)) != RSX_OK) {
		blind_give_up_room(c, c.slack1, c.slack1_v, c.slack, c.slack_v);   // (no room: as blind_enqueue -- what was allocated goes back, nobody asks again)
		return RSX_OK;
	}
	RSX_TRY(seg_layout<KT>(c, n));   // (Sc2Cfg<KT, NoVal> and <KT, VT> have the same tile: 32 Ki elements)
	static_assert((int)C2::TILE == (int)Sc2Cfg<KT, NoVal>::TILE, "one layout for both");
	RSX_TRY(c.gscan.ensure(256 * sizeof(u64)));
	const SegView sv(c);
	const u64 rows = sv.L.rows, ntiles0 = rows - seg_extra_rows<KT>();   // (the level-1 pass's tiles: no partial ones)
	SegCtl *ctl = sv.ctl();
	SegTile *tiles = sv.tiles();
	LeafSeg *segtab = sv.segtab();
	u32 *btile = sv.btile();
	u64 *off1 = (u64 *)c.gscan.p;
	if (!c.seg_ev)
		HIP_TRY(hipEventCreateWithFlags(&c.seg_ev, hipEventDisableTiming));
	c.host_segctl->mode = SEG_MODE_NONE;
	RSX_TRY(blind_forget_device_backoff(c));
	hipLaunchKernelGGL((rsx_blind_precheck_kernel<KT>), dim3(1 + 512), dim3(1024), 0, c.stream, kin, (u64)n, ka, ctl, c.plan(),
	                   c.dev_host_plan, (u32x4 *)sv.status(0), (u64)(2 * sv.L.st_bytes / 16),
	                   (u32)sizeof(KT),   // (every column kept: the callers' parity rule below counts on it)
	                   0u, 0u,
	                   // rank sorts (no keys wanted back): keys whose byte columns do not spread but whose VARYING bits would, packed
	                   // together, go by those (SegCtl::compact, README.md:716-758)
	                   (u32)((vin == nullptr && kfinal == nullptr && !env().no_packed_keys) ? 1 : 0), (u32)(g_in_async ? 1 : 0));
	SegArgs sa = sv.args(sizeof(KT));
	// the two parts of the level-1 slots (SegArgs): one base per array for the level-1 pass's stores and the parts' offsets from it;
	// for the level-2 pass the spare buffer as the array and the scratch part's virtual slot 0 as the other one
	KT *k1out = (KT *)c.slack1.p, *k1lo = (KT *)c.slack1.p;
	VT *v1out = (VT *)c.slack1_v.p, *v1lo = (VT *)c.slack1_v.p;
	const void *k1hi = nullptr, *v1hi = nullptr;
	sa.lo_slots = lo;
	if (klo) {
		const SlotParts parts(kspare, c.slack1.p, lo, cap1, sizeof(KT), C2::TILE);
		sa.out_off_lo = parts.off_lo;
		sa.out_off_hi = parts.off_hi;
		k1out = (KT *)parts.base;
		k1lo = kspare;
		k1hi = (const void *)parts.hi;
	}
	if (vlo) {
		const SlotParts parts(vspare, c.slack1_v.p, lo, cap1, sizeof(VT), C2::TILE);
		sa.v_off_lo = parts.off_lo;
		sa.v_off_hi = parts.off_hi;
		v1out = (VT *)parts.base;
		v1lo = vspare;
		v1hi = (const void *)parts.hi;
	}
	{
		ProfScope prof(1, (u64)n * (2 * sizeof(KT) + (vin ? 2 : 1) * sizeof(VT)), c.stream);
		sa.slack_cap = cap1;
		const u32 flags = (u32)SCATTER_SEG_SLACK | (u32)SCATTER_BLIND | (u32)SCATTER_BLIND_TOP | (vin ? 0u : (u32)SCATTER_GEN_INDEX);
		hipLaunchKernelGGL((rsx_scatter2_kernel<KT, VT, u32, C2, false, DIG_GENERIC, false, KT, true>), dim3((unsigned)ntiles0),
		                   dim3(C2::BLOCK), 0, c.stream, kin, k1out, vin, v1out, (u64)n, 0u,
		                   (const u64 *)c.ghist(), 1u, sv.cursors(1), sv.status(1), ka, flags, (u64 *)nullptr,
		                   (const Plan *)c.plan(), 0u, 0u, (const u32 *)nullptr, sa);
	}
	sa.out_off_lo = sa.out_off_hi = sa.v_off_lo = sa.v_off_hi = 0;
	sa.kin_hi = k1hi;
	sa.vin_hi = v1hi;
	hipLaunchKernelGGL(rsx_seg_tiles_kernel, dim3(32), dim3(256), 0, c.stream, (const u64 *)c.ghist(), (u64)n, (const Plan *)c.plan(),
	                   (u32)C2::TILE, tiles, ctl, btile, off1, cap1, (const u32 *)sv.cursors(1), (u32)ntiles0);
	{
		ProfScope prof(1, (u64)n * (sizeof(KT) + sizeof(K2) + 2 * sizeof(VT)), c.stream);
		sa.slack_cap = cap2;
		hipLaunchKernelGGL((rsx_scatter2_kernel<KT, VT, u32, C2, false, DIG_GENERIC, false, K2, true>), dim3((unsigned)rows),
		                   dim3(C2::BLOCK), 0, c.stream, (const KT *)k1lo, (K2 *)c.slack.p, (const VT *)v1lo,
		                   (VT *)c.slack_v.p, (u64)n, 0u, (const u64 *)c.ghist(), 1u, sv.cursors(0), sv.status(0), ka,
		                   (u32)SCATTER_SEG_SLACK | (u32)SCATTER_BLIND, (u64 *)nullptr, (const Plan *)c.plan(), 0u, 0u,
		                   (const u32 *)nullptr, sa);
	}
	hipLaunchKernelGGL((rsx_seg_slack_plan_kernel<u32>), dim3(256), dim3(256), 0, c.stream, (const u32 *)sv.cursors(0), (const u32 *)btile,
	                   (const u64 *)c.ghist(), (const Plan *)c.plan(), ctl, segtab, cap2, c.dev_host_segctl, (const u64 *)off1,
	                   1u | ((env().probe & 1u) << 8));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c.seg_ev, c.stream));
	{
		ProfScope prof(2, (u64)n * (sizeof(K2) + 2 * sizeof(VT) + (kfinal ? sizeof(KT) : 0)), c.stream);
		unsigned lds_grid = env().leaf_grid;
		const u32 *lds_redo = nullptr;
		if (!env().no_leaf16) {
			// the compounds (key half, position) through one placement and the register passes (rsx_leafp_kernel); what it
			// leaves alone -- or everything, if the sample saw the keys' low bits cluster -- through the LDS passes of round 3
			// Three shapes by the slots' capacity (the host knows it): a leaf's fixed costs -- cells zeroed and scanned, barriers
			// of the whole workgroup -- follow the shape, not the pairs in it (16 Mi pairs through the 5120-pair shape: 0.48 ms
			// for the leaves alone, as much as 128 Mi pairs take)
			typedef LeafKCfg<512, 5120, 8> P5;
			typedef LeafKCfg<256, 2560, 8, 11> P2;
			typedef LeafKCfg<128, 1280, 6, 10> P1;
			u32 *redo = sv.redo();
#define RSX_LEAFP(P) \
	hipLaunchKernelGGL((rsx_leafp_kernel<KT, VT, P, true>), dim3(65536u), dim3(P::BLOCK), 0, c.stream, (const KT *)c.slack.p, \
	                   (const VT *)c.slack_v.p, cap2, kfinal, vfinal, (const Plan *)c.plan(), (const LeafSeg *)segtab, ctl, ka, redo, \
	                   (u32)env().leaf16_maxbin)
			typedef LeafKCfg<64, 256, 8, 9> P0;    // slots of up to 256 pairs: a wave per leaf
			typedef LeafKCfg<64, 512, 8, 10> P0b;  // ... and of 512 (arrays of 11.5 .. 27 Mi pairs)
			if (big)
				RSX_LEAFP(P10);
			else if (cap2 <= (u32)P0::CAP && !env().no_leaf16q)
				RSX_LEAFP(P0);
			else if (cap2 <= (u32)P0b::CAP && !env().no_leaf16q)
				RSX_LEAFP(P0b);
			else if (cap2 <= (u32)P1::CAP)
				RSX_LEAFP(P1);
			else if (cap2 <= (u32)P2::CAP)
				RSX_LEAFP(P2);
			else
				RSX_LEAFP(P5);
#undef RSX_LEAFP
			lds_grid = 4096;
			lds_redo = redo;
		}
		// the LDS passes: of what the compound leaves left alone (their list), or -- RSX_NO_LEAF16 -- of every leaf
		if (big)
			launch_leaf_pairs16<KT, VT, LB>(c, lds_grid, cap2, kfinal, vfinal, segtab, ctl, ka, lds_redo);
		else
			launch_leaf_pairs16<KT, VT, L>(c, lds_grid, cap2, kfinal, vfinal, segtab, ctl, ka, lds_redo);
	}
	HIP_TRY(hipGetLastError());
	*enqueued = 1;
	return RSX_OK;
}

// ... and the blocking sorts' use of it: the host waits for the verdict (the event lies behind the slack plan kernel, in front of
// the leaves) and remembers an attempt that was called off (blind_called_off: back-off)
template <typename KT, typename VT>
int pairs_blind(Ctx &c, const KT *kin, const VT *vin, KT *kfinal, VT *vfinal, size_t n, KdfArgs<KT> ka, rsx_info *info, int *done,
                KT *kspare = nullptr, VT *vspare = nullptr)
{
	*done = 0;
	int enqueued = 0;
	const size_t pmark = prof_mark();
	RSX_TRY((pairs_blind_enqueue<KT, VT>(c, kin, vin, kfinal, vfinal, n, ka, &enqueued, kspare, vspare)));
	if (!enqueued)
		return RSX_OK;
	bool through = false;
	RSX_TRY(blind_verdict(c, blind_kind<KT>(sizeof(VT), vin == nullptr), pmark, &through));   // (no payloads given: a rank sort)
	if (!through)
		return RSX_OK;
	info_from_plan(info, *c.host_plan);
	if (info)
		info->hybrid = 5u;
	*done = 1;
	return RSX_OK;
}

}   // namespace
