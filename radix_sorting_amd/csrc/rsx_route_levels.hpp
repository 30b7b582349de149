// rsx_route_levels.hpp: the routes with MSB passes and leaves behind a histogram -- the layout of their control block (seg_layout,
// SegView), the leaves' shapes and launches, the segmented passes, one and two levels for keys alone and for (key, payload);
// part of librsx.so's host side, included by rsx.hip behind rsx_ctx.hpp, ahead of rsx_route_blind.hpp and the drivers.
#pragma once

namespace {

// ---- the control block of the segmented routes: c.seg, laid out by SegLayout (rsx_seg_layout.hpp) ------------------------------
static_assert(sizeof(SegCtl) <= SEG_CTL_BYTES && sizeof(LeafSeg) == SEG_LEAFSEG_BYTES && sizeof(SegTile) == SEG_TILE_BYTES,
              "rsx_seg_layout.hpp states the sizes of rsx_hybrid.hpp's structs");

// Rows of status words (and tile-table entries) a segmented pass may need beyond n / TILE: a partial tile per level-1 bucket, and
// -- 8-byte keys, whose level-1 pass may be rsx_pass32a_kernel in front of the CHAINED level-2 pass -- one more per bucket for
// what lies at its slot's end (rsx_seg_tiles_kernel, back_cap).
template <typename KT> constexpr u64 seg_extra_rows() { return sizeof(KT) == 8 ? 512 : 256; }

// rows of the tile table of a two-level sort's level-2 pass: the tiles of the pass that may run (the chained pass's, or the smaller
// ones of rsx_pass16a_kernel / rsx_pass64a_kernel) + per bucket a partial tile and one for what lies at its slot's end
template <typename KT> u64 seg_tile_rows(size_t n, u64 rows)
{
	if (sizeof(KT) == 4)
		return (n + Pass16aCfg::TILE - 1) / Pass16aCfg::TILE + 514;
	return std::max<u64>(rows, (n + Pass2wCfg<u32>::TILE - 1) / Pass2wCfg<u32>::TILE + 514);
}

// where the parts of a two-level sort's device-side state lie in c.seg (the key + payload routes use it too: pairs_two_level, pairs_blind_enqueue)
template <typename KT> SegLayout seg_layout_of(size_t n)
{
	typedef Sc2Cfg<KT, NoVal> C2;
	const u64 rows = seg_rows(n, C2::TILE, seg_extra_rows<KT>());
	return seg_layout_for(sizeof(KT), n, C2::TILE, seg_extra_rows<KT>(), seg_tile_rows<KT>(n, rows));
}

// bytes of c.seg for a two-level sort of n keys
template <typename KT> size_t seg_bytes(size_t n) { return seg_layout_of<KT>(n).total; }

template <typename KT> int seg_layout(Ctx &c, size_t n)
{
	c.seg_lay = seg_layout_of<KT>(n);
	const void *before = c.seg.p;
	RSX_TRY(c.seg.ensure(c.seg_lay.total));
	if (c.seg.p != before || c.seg.external)   // (a new control block -- or a caller's workspace, whose contents are scratch: SegCtl::boff_*)
		HIP_TRY(hipMemsetAsync(c.seg.p, 0, SEG_CTL_BYTES, c.stream));
	return RSX_OK;
}

// typed pointers to the parts of c.seg, as the last seg_layout of the context laid them out
struct SegView {
	char *const p;
	const SegLayout &L;
	explicit SegView(const Ctx &c) : p((char *)c.seg.p), L(c.seg_lay) {}
	SegCtl *ctl() const { return (SegCtl *)p; }
	u32 *hist() const { return (u32 *)(p + L.hist_off); }
	SegTile *tiles() const { return (SegTile *)(p + L.tiles_off); }
	LeafSeg *segtab() const { return (LeafSeg *)(p + L.segtab_off); }
	u32 *btile() const { return (u32 *)(p + L.btile_off); }
	u32 *redo() const { return (u32 *)(p + L.redo_off); }
	// segmented pass j: the ticket word at the head of its status region, and the status words (or cursors) behind it
	u32 *status(u32 j) const { return (u32 *)(p + L.status(j)); }
	u32 *cursors(u32 j) const { return (u32 *)(p + L.cursors(j)); }
	// what every segmented pass over keys of `key_bytes` bytes is told about the block (slots, spare buffers: the caller's)
	SegArgs args(size_t key_bytes) const
	{
		SegArgs sa{};
		sa.ctl = ctl();
		sa.hist = hist();
		sa.tiles = tiles();
		sa.slots = (u32)key_bytes - 1;
		sa.overflow = &ctl()->overflow;
		return sa;
	}
	// the control block, the digit counts and the status words of the first segmented pass zeroed together, then the tile table
	// of a level-2 pass over tiles of `tile` keys from the histogram's buckets
	int reset_and_tiles(Ctx &c, size_t n, u32 tile) const
	{
		HIP_TRY(hipMemsetAsync(p, 0, L.status(1), c.stream));
		hipLaunchKernelGGL(rsx_seg_tiles_kernel, dim3(32), dim3(256), 0, c.stream, (const u64 *)c.ghist(), (u64)n, (const Plan *)c.plan(),
		                   tile, tiles(), ctl(), btile());
		return RSX_OK;
	}
};

// ---- one MSB pass and leaves (rsx_hybrid.hpp; README.md:647-650) ---------------------------------------------------------
template <typename KT> struct LeafShapes {
	typedef LeafCfg<KT, 4, 32, sizeof(KT) == 8 ? 2 : 4, true, false> Small;   // 8 Ki keys: several workgroups per CU
	typedef LeafCfg<KT, 16, sizeof(KT) == 8 ? 16 : 32> Big;      // as many keys as the LDS stages at once: one workgroup per CU
	// 4-byte keys: a shape in between (16 Ki keys, two workgroups per CU) -- leaves of 8-16 Ki keys (2^29 keys in 65536 buckets)
	// in the large shape were no faster than four passes.  8-byte keys: the small shape already holds 64 KiB.
	static constexpr bool HAS_MEDIUM = sizeof(KT) == 4;
	typedef LeafCfg<KT, 8, 32, 4, true, false> Medium;
	// 4-byte keys, leaves read from slots of at most 5120 keys (2^28 keys in 65536 slots: BASELINE.json's headline): the small
	// shape cut to that size -- twenty rounds per lane instead of thirty-two, 24.5 instead of 37 KiB of LDS: the leaves of 2^28
	// keys take 0.587 instead of 0.640 ms (tools/ubench/leaf_probe, profiles/r03/leaf_probe.txt; with room for a fifth
	// workgroup's registers the compiler spills: 1.5 ms)
	static constexpr bool HAS_FIT = sizeof(KT) == 4;
	typedef LeafCfg<KT, 4, 20, 4, true, false> Fit;
	// ... and two smaller cuts for smaller arrays (the slots of 56 Mi .. 100 Mi keys hold up to 2048 keys, those of up to
	// 157 Mi up to 3072): eight / twelve rounds per lane.  tools/ubench/leaf_probe, 65536 leaves of 1024 keys: 0.229 against
	// 0.346 ms in the 5120-key shape; of 2048 keys: 0.321 against 0.421
	typedef LeafCfg<KT, 4, 8, 8, true, false> Fit2k;
	typedef LeafCfg<KT, 4, 12, 6, true, false> Fit3k;
	// ... the shape (bits 5, 6, 3: the three cuts) for leaves that lie in slots of `cap` keys
	static u32 shape_for_slots(u32 cap)
	{
		if (HAS_FIT && cap <= (u32)Fit2k::CAP)
			return 32u;
		if (HAS_FIT && cap <= (u32)Fit3k::CAP)
			return 64u;
		if (HAS_FIT && cap <= (u32)Fit::CAP)
			return 8u;
		return shape_for(cap);
	}
	// the shape (bit 0 small, bit 2 medium, bit 1 large) for leaves of up to `m` keys
	static u32 shape_for(u32 m)
	{
		if (m <= (u32)Small::CAP)
			return 1u;
		if (HAS_MEDIUM && m <= (u32)Medium::CAP)
			return 4u;
		return 2u;
	}
};

// RSX_NO_HYBRID=1: one pass per kept column whatever the keys look like (the reference's loop, radix_sort.hpp:82-90)
bool hybrid_enabled() { return !env().no_hybrid; }

template <typename KT> HybCaps hybrid_caps(size_t n)
{
	HybCaps caps{0, 0, 0, 0};
	if constexpr (sizeof(KT) >= 4) {
		if (hybrid_enabled() && n < ((size_t)1 << 30)) {
			caps.cap1 = (u32)LeafShapes<KT>::Big::CAP;
			caps.min_cols1 = 3;
			// Two levels pay from about 2^27 keys on (tools/size_sweep.py, profiles/r03/size_sweep.txt: 128 Mi keys 1.16 ms
			// against 1.22 with one pass per column, 256 Mi 1.89 against 2.30; at 64 Mi 0.73 against 0.62 -- a dozen launches
			// and two host round trips are a fixed cost).  Between the reach of one level (about 7 Mi evenly spread keys)
			// and that, one pass per kept column.
			if (n >= ((size_t)1 << env().two_level_min_log2)) {
				caps.cap2 = (u32)LeafShapes<KT>::Big::CAP;   // (leaves beyond the small shape's 8 Ki keys take the large one)
				caps.min_cols2 = 4;
			}
		}
	}
	return caps;
}

// The capacity of a slot for buckets of `mean` keys: 1.25 times the mean, and at least seven standard deviations of an evenly
// spread array's bucket sizes above it, rounded up to 256 keys.  (The second term is what small slots need: with 1.25 x alone a
// mean of 200 keys gets 256-key slots, 3.6 sigma -- evenly spread arrays of 11.5 .. 13 Mi keys overflowed one of their 65536
// slots in one sort out of seven to nine out of ten and were sorted by one pass per column after a lost attempt.)
static inline u32 slot_cap_for(u32 mean)
{
	u32 r = 0;
	while ((u64)(r + 1) * (r + 1) <= mean)
		++r;
	const u32 need = std::max(mean + mean / 4, mean + 7 * (r + 1) + 8);
	return ((need + 255) / 256) * 256;
}

// The capacity -- and the spacing -- of the 256 level-1 slots of a keys-only sort without a histogram.
// The slots fill at the same rate, so the 256 write streams of the level-1 pass stand at the same offset of their slots at any
// time, one slot stride apart: with strides of 15 or 17 x 2 MiB (1.5 x 2^30 four-byte keys: 30 MiB) they meet in the same memory
// channels and the pass runs at 3.6 TB/s instead of 4.5 (tools/stride_probe.py, profiles/r06/stride_probe.txt: +64 KiB .. +1 MiB
// per slot restore it, +4 MiB = 17 x 2 MiB is as bad again).  Slots of a MiB and more are an ODD number of 64 KiB apart
// (RSX_NO_ODD_STRIDE=1: as round 5).  RSX_CAP1_PAD_KIB: that many KiB more per slot (the probe).
template <typename KT> u32 level1_slot_cap(u32 mean)
{
	u32 cap1 = slot_cap_for(mean) + env().cap1_pad_kib * (1024u / (u32)sizeof(KT));
	if (!env().no_odd_stride && (size_t)cap1 * sizeof(KT) >= ((size_t)1 << 20)) {
		const u32 unit = 65536u / (u32)sizeof(KT);
		cap1 = (cap1 + unit - 1) / unit * unit;
		if ((cap1 / unit) % 2u == 0)
			cap1 += unit;
	}
	return cap1;
}

// 8-byte keys: may the sample choose four-byte level-2 slots (SegCtl::narrow)?  Where rsx_leafk_kernel sorts the slots, from
// slots of 512 keys (arrays of ~13 Mi keys) on: the second form of the level-2 pass and of the leaves are two more launches, which
// 8 Mi keys notice (0.267 against 0.252 ms; 16 Mi: 0.328 against 0.337, 64 Mi 0.77 against 0.87, 192 Mi 2.06 against 2.29:
// tools/u64_threshold_probe.py, keys & 0xFFFFFFFFFF).
template <typename KT> bool narrow_slots_ok(u32 cap2)
{
	return sizeof(KT) == 8 && cap2 >= 512u && cap2 <= 5120u && !env().no_leaf16 && !env().no_narrow_slots;
}

// Sorts without a histogram of 4-byte keys (all four columns kept): the level-2 pass writes only the low two bytes of the
// derived keys into its slots and the leaves put the rest back from the slot's digits (RSX_NO_DENSE_SLOTS=1: whole keys).
// (where the slots fit the leaf shape that reads them: up to 5120 keys each, 2^28 keys in all)
// the largest two-byte slot there are leaves for: rsx_leaf16_kernel's 5120 values; round 5: 40960 (slots of 2^31 keys) with the
// counting leaves of rsx_leafc.hpp behind larger shapes of that kernel
constexpr u32 LEAFC_CAP = 40960;
template <typename KT> u32 dense_cap_max()
{
	if (sizeof(KT) != 4)
		return 0u;
	const bool big = !env().no_leafc && !env().no_leaf16 && !env().no_pass16 && !env().no_pass16a && !env().no_unstable;
	return big ? LEAFC_CAP : (u32)LeafShapes<KT>::Fit::CAP;
}
template <typename KT> bool dense_slots(const Ctx &c)
{
	if (sizeof(KT) != 4 || env().no_dense_slots || c.slack_cap == 0 || c.slack_cap > dense_cap_max<KT>())
		return false;
	if (c.slack_cap > (u32)LeafShapes<KT>::Fit::CAP)
		return true;   // (rsx_leafc.hpp: on unless dense_cap_max says otherwise)
	// round 4: rsx_leaf16_kernel (rsx_leaf16.hpp) sorts two-byte slots of every size up to 5120 values faster than the
	// leaves of whole keys are sorted (tools/ubench/leaf16_probe: 2^28 keys 0.39 against 0.67 ms, 2^27 0.25 against 0.46)
	if (!env().no_leaf16)
		return true;
	// RSX_NO_LEAF16=1, round 3's leaves: slots of 3073 .. 5120 keys only (with the smaller cuts the two-byte leaves are level
	// or a little behind -- 64 Mi keys 0.565 against 0.548 ms, 128 Mi 0.867 against 0.862); RSX_DENSE_SLOTS=1: every size
	return env().force_dense_slots || c.slack_cap > (u32)LeafShapes<KT>::Fit3k::CAP;
}

// The leaves of a level (rsx_leaf_sort_kernel).  `shapes`: bit 0 the shape for leaves of up to 8 Ki keys, bit 1 the one that
// fills the LDS; a launched shape does nothing unless the device-side plan has leaves of its size, so both may be enqueued
// before the host knows (nothing then waits for the host).
template <typename KT>
int launch_leaves(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, u32 level, u32 shapes, const u64 *off1 = nullptr)
{
	typedef typename LeafShapes<KT>::Small S;
	typedef typename LeafShapes<KT>::Big B;
	// one workgroup per bucket at level 1; level 2: a workgroup per table entry (0.569 against 0.585 ms for 2^28 keys with
	// 8192 persistent ones, tools/ubench/leaf_probe; RSX_LEAF_GRID to probe other grids)
	const unsigned grid_s = level == HYB_TWO_LEVEL ? env().leaf_grid : 256u;
	const unsigned grid_1 = 65536u;   // the kernels of rsx_leaf16.hpp take one leaf per workgroup (wave, row): the grid IS the table (LEAF_ONE_PER_GROUP)
	const unsigned grid_b = 256u;
	const SegView sv(c);
	const LeafSeg *segtab = level == HYB_TWO_LEVEL ? (const LeafSeg *)sv.segtab() : nullptr;
	const SegCtl *ctl = sv.ctl();
	const bool dense = (shapes & 0x100u) != 0;   // (bit 8: the leaves read two-byte slots, dense_slots)
	ProfScope prof(2, (u64)n * (dense ? 2 + sizeof(KT) : 2 * sizeof(KT)), c.stream);
	const KT *slots = level == HYB_TWO_LEVEL ? (const KT *)c.slack.p : nullptr;   // (only leaves of a slack attempt name slots)
	const u32 nopre = env().no_leaf_prefix ? 2u : 0u;   // RSX_NO_LEAF_PREFIX=1: 8-byte-key leaves go through all their columns
	u32 skip_narrowable = nopre;
	if constexpr (sizeof(KT) == 8) {
		if ((shapes & 0x200u) && !env().no_leaf16) {
			// a sort without a histogram, slots of up to 5120 keys: one placement by twelve bits + register passes on 4- or
			// 8-byte values (rsx_leafk_kernel, rsx_leaf16.hpp: the instantiation whose carried type the leaves' columns need
			// works, the other does nothing); what they leave alone goes through the LDS passes of round 3
			u32 *redo = sv.redo();
			SegCtl *wctl = sv.ctl();
			// (three shapes by the slots' capacity, as the pairs' leaves: a leaf's fixed costs follow its shape)
#define RSX_LEAFK(K4, K8)                                                                                                      \
	do {                                                                                                                       \
		hipLaunchKernelGGL((rsx_leafk_kernel<KT, u32, K4>), dim3(grid_1), dim3(K4::BLOCK), 0, c.stream, src, aux,               \
		                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)K4::CAP, slots, c.slack_cap, redo,               \
		                   (u32)env().leaf16_maxbin);                                                                          \
		hipLaunchKernelGGL((rsx_leafk_kernel<KT, u64, K8>), dim3(grid_1), dim3(K8::BLOCK), 0, c.stream, src, aux,               \
		                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)K8::CAP, slots, c.slack_cap, redo,               \
		                   (u32)env().leaf16_maxbin);                                                                          \
		if (narrow_slots_ok<KT>(c.slack_cap))   /* four-byte slots (SegCtl::narrow) */                                          \
			hipLaunchKernelGGL((rsx_leafk_kernel<KT, u32, K4, true>), dim3(grid_1), dim3(K4::BLOCK), 0, c.stream, src, aux,     \
			                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)K4::CAP, slots, c.slack_cap, redo,           \
			                   (u32)env().leaf16_maxbin);                                                                      \
	} while (0)
			typedef LeafKCfg<512, 5120, 8> K4;
			typedef LeafKCfg<512, 5120, 8> K8;   // (8-byte values staged in 6 bytes: four workgroups per CU)
			typedef LeafKCfg<256, 2560, 8, 11> K2;
			typedef LeafKCfg<128, 1280, 6, 10> K1;
			typedef LeafKCfg<64, 256, 8, 9> K0;    // slots of up to 256 keys (arrays of up to ~13 Mi keys): a wave per leaf
			typedef LeafKCfg<64, 512, 8, 10> K0b;  // ... and of 512 (arrays of 11.5 .. 27 Mi keys)
			if (c.slack_cap <= (u32)K0::CAP && !env().no_leaf16q)
				RSX_LEAFK(K0, K0);
			else if (c.slack_cap <= (u32)K0b::CAP && !env().no_leaf16q)
				RSX_LEAFK(K0b, K0b);
			else if (c.slack_cap <= (u32)K1::CAP)
				RSX_LEAFK(K1, K1);
			else if (c.slack_cap <= (u32)K2::CAP)
				RSX_LEAFK(K2, K2);
			else {
				// the 5120-key shape (arrays above 2^27 keys: BASELINE.json's cfg 3): the 8-byte-carried leaves by their own kernel
				hipLaunchKernelGGL((rsx_leafk_kernel<KT, u32, K4>), dim3(grid_1), dim3(K4::BLOCK), 0, c.stream, src, aux,
				                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)K4::CAP, slots, c.slack_cap, redo,
				                   (u32)env().leaf16_maxbin);
				hipLaunchKernelGGL((rsx_leafk8_kernel<KT, u64, LeafK8Cfg>), dim3(grid_1), dim3(LeafK8Cfg::BLOCK), 0, c.stream, src, aux,
				                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)LeafK8Cfg::CAP, slots, c.slack_cap, redo,
				                   (u32)env().leaf16_maxbin);
				if (narrow_slots_ok<KT>(c.slack_cap))
					hipLaunchKernelGGL((rsx_leafk_kernel<KT, u32, K4, true>), dim3(grid_1), dim3(K4::BLOCK), 0, c.stream, src, aux,
					                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)K4::CAP, slots, c.slack_cap, redo,
					                   (u32)env().leaf16_maxbin);
			}
#undef RSX_LEAFK
			typedef LeafCfg<u32, 4, 32, 3, true, false> N;
			hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, N, u32>), dim3(2048), dim3(N::BLOCK), 0, c.stream, src, aux, (u64)n,
			                   (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u, (u32)S::CAP, slots,
			                   c.slack_cap, nopre, off1, (const u32 *)redo);
			hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, S>), dim3(2048), dim3(S::BLOCK), 0, c.stream, src, aux, (u64)n,
			                   (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u, (u32)S::CAP, slots,
			                   c.slack_cap, nopre | 1u, off1, (const u32 *)redo);
			HIP_TRY(hipGetLastError());
			return RSX_OK;
		}
		// 8-byte keys: leaves whose columns all lie in the low four bytes are carried as 4-byte values (rsx_hybrid.hpp, CT)
		if (shapes & 1u) {
			typedef LeafCfg<u32, 4, 32, 3, true, false> N;   // (131 registers: three workgroups per CU)
			static_assert(N::CAP == S::CAP, "the narrow shape takes the small shape's leaves");
			hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, N, u32>), dim3(grid_s), dim3(N::BLOCK), 0, c.stream, src, aux, (u64)n,
			                   (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u, (u32)S::CAP, slots,
			                   c.slack_cap, nopre, off1);
			skip_narrowable |= 1u;
		}
	}
	if constexpr (sizeof(KT) == 4) {
		if (dense && !env().no_leaf16) {
			// two-byte slots: one placement by the top bits + two register passes (rsx_leaf16.hpp); what that kernel leaves
			// alone (a list; or everything, if the sample saw the low sixteen bits cluster) goes through the two LDS passes
			u32 *redo = sv.redo();
			SegCtl *wctl = sv.ctl();
			if (c.slack_cap > 5120u || (env().force_leafc && c.slack_cap <= LEAFC_CAP)) {
				const unsigned force = env().force_leafc;
				// round 5, arrays beyond 2^28 keys (rsx_leafc.hpp).  Slots of up to 20480 values (2^30 keys): rsx_leaf16_kernel in a larger
				// shape -- 13 or 14 bits name a value's bin, 512 or 1024 threads to a leaf --, and behind it the counting leaves for what
				// it leaves alone; larger slots (2^31 keys: 32 Ki values each): the counting leaves at once.  tools/ubench/leafc_probe,
				// profiles/r05/leafc_probe.txt: 2^29 keys 0.81 ms against 1.78 counting, 2^30 1.80 against 2.35, 2^31 4.33 against 3.20.
				// (the shapes' ladder: tools/ubench/leafc_probe at 300 M, 400 M, 2^29, 700 M, 2^30 and 1.5 x 2^30 keys,
				// profiles/r05/leafc_probe_between.txt -- every step is 10-20 % over the next larger shape at its size)
				typedef Leaf16Cfg<256, 6144, 8, 12> L6k;
				typedef Leaf16Cfg<256, 7680, 8, 12> L7k;
				typedef Leaf16Cfg<512, 10240, 8, 13> L10k;
				typedef Leaf16Cfg<512, 15360, 8, 13> L15k;
				typedef Leaf16Cfg<1024, 20480, 8, 14> L20k;
				const unsigned grid_c = 256u;   // (a workgroup per CU: the cells fill the LDS)
#define RSX_LAUNCH_LC(NVEC, REDO)                                                                                           \
				hipLaunchKernelGGL((rsx_leafc_kernel<KT, LeafCCfg<NVEC>>), dim3(grid_c), dim3(LeafCCfg<NVEC>::BLOCK), 0, c.stream, src, aux, \
				                   (const Plan *)c.plan(), segtab, ctl, ka, 0u, (u32)LeafCCfg<NVEC>::CAP, (const uint16_t *)slots,     \
				                   c.slack_cap, (const u32 *)(REDO))
#define RSX_LAUNCH_L16B(CFG, NVEC)                                                                                          \
				do {                                                                                                        \
					hipLaunchKernelGGL((rsx_leaf16_kernel<KT, CFG>), dim3(grid_1), dim3(CFG::BLOCK), 0, c.stream, src, aux,   \
					                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)CFG::CAP, (const uint16_t *)slots,   \
					                   c.slack_cap, redo, (u32)env().leaf16_maxbin);                                          \
					RSX_LAUNCH_LC(NVEC, redo);                                                                                \
				} while (0)
				const u32 cap = c.slack_cap;
				// (RSX_FORCE_LEAFC, tests: 1 counting, 2 / 3 / 4 / 5 / 6 the 10240- / 20480- / 6144- / 7680- / 15360-value shape)
				const unsigned pick = force ? force
				                            : cap <= (u32)L6k::CAP ? 4u : cap <= (u32)L7k::CAP ? 5u : cap <= (u32)L10k::CAP ? 2u
				                            : cap <= (u32)L15k::CAP ? 6u : cap <= (u32)L20k::CAP ? 3u : 1u;
				if (pick == 4 && cap <= (u32)L6k::CAP)
					RSX_LAUNCH_L16B(L6k, 2);
				else if (pick == 5 && cap <= (u32)L7k::CAP)
					RSX_LAUNCH_L16B(L7k, 2);
				else if (pick == 2 && cap <= (u32)L10k::CAP)
					RSX_LAUNCH_L16B(L10k, 2);
				else if (pick == 6 && cap <= (u32)L15k::CAP)
					RSX_LAUNCH_L16B(L15k, 2);
				else if (pick == 3 && cap <= (u32)L20k::CAP)
					RSX_LAUNCH_L16B(L20k, 3);
				else if (cap <= (u32)LeafCCfg<4>::CAP)
					RSX_LAUNCH_LC(4, nullptr);
				else
					RSX_LAUNCH_LC(5, nullptr);
#undef RSX_LAUNCH_L16B
#undef RSX_LAUNCH_LC
				HIP_TRY(hipGetLastError());
				return RSX_OK;
			}
			typedef Leaf16Cfg<256, 5120, 8, 12> L5k;
			// (128 threads per leaf for slots of up to 2560 values -- arrays of 52 Mi .. 128 Mi keys: a 1280-value leaf keeps 80 lanes
			// busy in the register passes, and sixteen small workgroups per CU overlap better than eight: tools/ubench/leaf16_probe,
			// profiles/r05/leaf16_probe_mid.txt: 56 Mi keys 0.118 against 0.163 ms, 128 Mi 0.214 against 0.252)
			typedef Leaf16Cfg<128, 2560, 8, 11> L2k;
			typedef Leaf16WCfg<1024, 10, 4> W1k;   // small slots (arrays of up to ~50 Mi keys): a wave per leaf
			typedef Leaf16WCfg<512, 9, 4> W512;
			// ... and, round 5, up to 2048 values (arrays of up to ~100 Mi keys: two chunks of sixteen values per lane in the register
			// passes, slots read from both ends behind rsx_pass16a_kernel): tools/ubench/leaf16_probe against the 128-thread
			// workgroup shape -- 54 Mi keys 0.110 against 0.119 ms, 64 Mi 0.131 / 0.143, 80 Mi 0.145 / 0.167, 96 Mi 0.162 / 0.180
			typedef Leaf16WCfg<2048, 10, 4> W2k;
			if (c.slack_cap > (u32)W1k::CAP && c.slack_cap <= (u32)W2k::CAP && !env().no_leaf16w2k) {
				hipLaunchKernelGGL((rsx_leaf16w_kernel<KT, W2k>), dim3(grid_1 / W2k::NW), dim3(W2k::BLOCK), 0, c.stream, src, aux,
				                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)W2k::CAP, (const uint16_t *)slots, c.slack_cap);
				HIP_TRY(hipGetLastError());
				return RSX_OK;
			}
			if (c.slack_cap <= (u32)W1k::CAP) {
				// (no list, no second launch: the wave kernel goes on until its leaf is in order)
				typedef Leaf16QCfg<4> Q256;            // slots of up to 256 values (arrays of up to ~13 Mi keys): four leaves per wave
				if (c.slack_cap <= (u32)Q256::CAP && !env().no_leaf16q)
					hipLaunchKernelGGL((rsx_leaf16q_kernel<KT, Q256>), dim3(grid_1 / Q256::ROWS), dim3(Q256::BLOCK), 0, c.stream, src, aux,
					                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)Q256::CAP, (const uint16_t *)slots, c.slack_cap);
				else if (c.slack_cap <= (u32)W512::CAP)
					hipLaunchKernelGGL((rsx_leaf16w_kernel<KT, W512>), dim3(grid_1 / W512::NW), dim3(W512::BLOCK), 0, c.stream, src, aux,
					                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)W512::CAP, (const uint16_t *)slots, c.slack_cap);
				else
					hipLaunchKernelGGL((rsx_leaf16w_kernel<KT, W1k>), dim3(grid_1 / W1k::NW), dim3(W1k::BLOCK), 0, c.stream, src, aux,
					                   (const Plan *)c.plan(), segtab, wctl, ka, 0u, (u32)W1k::CAP, (const uint16_t *)slots, c.slack_cap);
				HIP_TRY(hipGetLastError());
				return RSX_OK;
			}
#define RSX_LAUNCH_L16(KERNEL, CFG, GRID)                                                                                     \
			hipLaunchKernelGGL((KERNEL<KT, CFG>), dim3(GRID), dim3(CFG::BLOCK), 0, c.stream, src, aux, (const Plan *)c.plan(),  \
			                   segtab, wctl, ka, 0u, (u32)CFG::CAP, (const uint16_t *)slots, c.slack_cap, redo,                \
			                   (u32)env().leaf16_maxbin)
			if (c.slack_cap <= (u32)L2k::CAP)
				RSX_LAUNCH_L16(rsx_leaf16_kernel, L2k, grid_1);
			else
				RSX_LAUNCH_L16(rsx_leaf16_kernel, L5k, grid_1);
#undef RSX_LAUNCH_L16
			typedef typename LeafShapes<KT>::Fit F_;
			hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, F_, uint16_t, true>), dim3(4096), dim3(F_::BLOCK), 0, c.stream, src, aux,
			                   (u64)n, (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u, (u32)F_::CAP, slots,
			                   c.slack_cap, nopre, off1, (const u32 *)redo);
			HIP_TRY(hipGetLastError());
			return RSX_OK;
		}
	}
	if constexpr (LeafShapes<KT>::HAS_FIT) {
		// the shapes cut to the slots' size (exactly one of them is asked for; each takes the leaves up to its capacity)
#define RSX_LAUNCH_FIT(BIT, SHAPE)                                                                                          \
		if (shapes & (BIT)) {                                                                                               \
			typedef typename LeafShapes<KT>::SHAPE F_;                                                                      \
			if (dense)                                                                                                      \
				hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, F_, uint16_t, true>), dim3(grid_s), dim3(F_::BLOCK), 0, c.stream, \
				                   src, aux, (u64)n, (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u, \
				                   (u32)F_::CAP, slots, c.slack_cap, nopre, off1);                                          \
			else                                                                                                            \
				hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, F_>), dim3(grid_s), dim3(F_::BLOCK), 0, c.stream, src, aux,     \
				                   (u64)n, (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u,       \
				                   (u32)F_::CAP, slots, c.slack_cap, nopre, off1);                                          \
		}
		RSX_LAUNCH_FIT(32u, Fit2k)
		RSX_LAUNCH_FIT(64u, Fit3k)
		RSX_LAUNCH_FIT(8u, Fit)
#undef RSX_LAUNCH_FIT
	}
	if (shapes & 1u)
		hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, S>), dim3(grid_s), dim3(S::BLOCK), 0, c.stream, src, aux, (u64)n,
		                   (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, 0u, (u32)S::CAP, slots,
		                   c.slack_cap, skip_narrowable, off1);
	typedef typename LeafShapes<KT>::Medium M;
	const u32 big_lo = LeafShapes<KT>::HAS_MEDIUM ? (u32)M::CAP : (u32)S::CAP;
	if constexpr (LeafShapes<KT>::HAS_MEDIUM) {
		if (shapes & 4u)
			hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, M>), dim3(level == HYB_TWO_LEVEL ? env().leaf_grid : 256u), dim3(M::BLOCK), 0, c.stream, src,
			                   aux, (u64)n, (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, (u32)S::CAP, (u32)M::CAP,
			                   slots, c.slack_cap, nopre, off1);
	}
	if (shapes & 2u)
		hipLaunchKernelGGL((rsx_leaf_sort_kernel<KT, B>), dim3(grid_b), dim3(B::BLOCK), 0, c.stream, src, aux, (u64)n,
		                   (const u64 *)c.ghist(), (const Plan *)c.plan(), segtab, ctl, ka, level, big_lo, (u32)B::CAP, slots,
		                   c.slack_cap, nopre, off1);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// The level-2 pass of a keys-only sort of 4-byte keys without a histogram writes whole 64-byte atoms (rsx_pass16a_kernel,
// rsx_pass16.hpp) where the leaves are rsx_leaf16_kernel's (slots of more than 1024 values: arrays from about 52 Mi keys),
// which read a slot from both ends; its tiles are Pass16aCfg::TILE keys.
template <typename KT> bool pass16a_wanted(const Ctx &c)
{
	if constexpr (sizeof(KT) == 4)
	{
		if (!dense_slots<KT>(c) || env().no_pass16 || env().no_pass16a || env().no_unstable || env().no_leaf16)
			return false;
		if (c.slack_cap > 1024u)
			return true;
		// slots of 1024 values (38 .. 52 M keys; the wave per leaf reads both ends since round 5): where the 128 places kept for a
		// slot's back still leave its front the room slot_cap_for wanted for the whole slot -- mean + 7 standard deviations:
		// 37.7 M .. 45.9 M keys (the reference's own headline size, 4 * 10^7, among them)
		if (c.slack_cap == 1024u && c.slack_mean) {
			u32 r = 0;
			while ((u64)(r + 1) * (r + 1) <= c.slack_mean)
				++r;
			return c.slack_mean + 7 * (r + 1) + 8 <= c.slack_cap - LEAF16_BACK;
		}
		return false;
	}
	return false;
}

// a pass inside the level-1 buckets (SEG instantiation of the pass kernel): j < 0 the one by the level-2 column (runs in
// SEG_MODE_LEAVES), j >= 0 LSB-first pass j (runs in SEG_MODE_LSD).  aux -> src, src -> aux for odd j.
// j == -2: the slack attempt (aux -> the slots of c.slack, no counts needed).
// blind (a sort without a histogram, sort_keys_blind): 1 = its level-1 pass (`aux` = the caller's array -> the 256 slots of
// c.slack1, by the top column, status region 1), 2 = its level-2 pass (j == -2, reading c.slack1 instead of `aux`).
// 8-byte keys, the level-2 pass into FOUR-byte slots (SegCtl::narrow) as rsx_pass64a_kernel: whole atoms, cursors, two-ended slots
// (rsx_leafk_kernel's SLOT32 form reads both ends whatever its shape)
template <typename KT> bool pass64a_narrow_wanted(const Ctx &c)
{
	if (sizeof(KT) != 8 || !narrow_slots_ok<KT>(c.slack_cap) || env().no_pass64a || env().no_unstable || !c.slack_mean)
		return false;
	// the 128 places kept for a slot's back must leave its front mean + 6 standard deviations (what is carried to the back, a
	// few dozen values per slot, comes on top): just below a step of slot_cap_for they do not -- 64 Mi keys, mean 1024 in slots
	// of 1280, lost the attempt -- and the chained pass, whose slots have no back, stays
	u32 r = 0;
	while ((u64)(r + 1) * (r + 1) <= c.slack_mean)
		++r;
	return c.slack_mean + 6 * (r + 1) + 8 <= c.slack_cap - Pass2wCfg<u32>::BACK;
}

template <typename KT>
int launch_seg_pass(Ctx &c, const KT *aux, KT *src, size_t n, KdfArgs<KT> ka, int j, int blind = 0)
{
	typedef Sc2Cfg<KT, NoVal> C2;
	const SegView sv(c);
	const u64 rows = sv.L.rows;
	const u32 region = blind == 1 ? 1u : j < 0 ? 0u : (u32)j;   // the pass's status region: its ticket, then its status words
	u32 *const ticket = sv.status(region), *const st = sv.cursors(region);
	SegArgs sa = sv.args(sizeof(KT));
	sa.slack_cap = blind == 1 ? c.slack1_cap : j == -2 ? c.slack_cap : 0u;
	KT *const second = blind == 1 ? src : blind == 2 ? const_cast<KT *>(aux) : nullptr;
	if (j == -2)
		src = (KT *)c.slack.p;
	// blind: `src` (level-1 pass) / `aux` (level-2 pass) name the caller's second buffer when the first slack1_lo level-1 slots
	// lie there (blind_enqueue); the others lie in c.slack1
	if (blind == 1 || blind == 2) {
		KT *first = (KT *)c.slack1.p;
		if (second && c.slack1_lo) {
			sa.lo_slots = c.slack1_lo;
			const SlotParts parts(second, c.slack1.p, c.slack1_lo, c.slack1_cap, sizeof(KT), C2::TILE);
			if (blind == 1) {
				// one base for the level-1 pass's stores, the parts' offsets in its run offsets (blind_enqueue has checked
				// that both lie within 2^32 elements of the lower one)
				sa.out_off_lo = parts.off_lo;
				sa.out_off_hi = parts.off_hi;
				first = (KT *)parts.base;
			} else {
				sa.kin_hi = (const void *)parts.hi;   // (virtual slot 0 of the scratch part: slack1_lo slots before the array)
				first = second;
			}
		}
		if (blind == 1)
			src = first;
		else
			aux = first;
	}
	const bool dense = sizeof(KT) == 4 && blind == 2 && dense_slots<KT>(c);   // (keys written as two bytes: its own line in the profile)
	ProfScope prof(dense ? 3 : 1, (u64)n * (dense ? sizeof(KT) + 2 : 2 * sizeof(KT)), c.stream);
	const bool plain = ka.fmask == 0 && ka.sflip == 0 && ka.desc == 0;
	u32 flags = j == -2 ? (u32)SCATTER_SEG_SLACK : j < 0 ? (u32)SCATTER_SEG_LEAVES : 0u;
	if (blind)
		flags |= SCATTER_BLIND | (blind == 1 ? (u32)SCATTER_BLIND_TOP : 0u);
	// keys only, and what these two passes write is sorted by leaves that do not care in which order a bucket's keys arrive
	// (any ascending order of equal bits is the reference's output): no row of cells per wave, no layout over the rows
	if (blind && !env().no_unstable)
		flags |= SCATTER_UNSTABLE;
	const u32 pi = j < 0 ? 0u : (u32)j;
	const unsigned grid = blind == 1 ? (unsigned)(rows - seg_extra_rows<KT>()) : (unsigned)rows;
	const u32 shift0 = 0u;   // (every segmented pass reads its column from the device-side plan)
#define RSX_LAUNCH_SEG(DIGV)                                                                                               \
	hipLaunchKernelGGL((rsx_scatter2_kernel<KT, NoVal, u32, C2, false, DIGV, false, KT, true>), dim3(grid),                 \
	                   dim3(C2::BLOCK), 0, c.stream, aux, src, (const NoVal *)nullptr, (NoVal *)nullptr, (u64)n, shift0,     \
	                   (const u64 *)c.ghist(), 1u, st, ticket, ka, flags, (u64 *)nullptr,             \
	                   (const Plan *)c.plan(), pi, 0u, (const u32 *)nullptr, sa)
	if constexpr (sizeof(KT) == 4) {
		if (dense && pass16a_wanted<KT>(c)) {
			// ... and with whole 64-byte atoms: a workgroup takes a range of tiles and carries what does not fill an atom
			const unsigned pgrid = 512;
			if (plain)
				hipLaunchKernelGGL((rsx_pass16a_kernel<KT, DIG_PLAIN>), dim3(pgrid), dim3(Pass16aCfg::BLOCK), 0, c.stream, (const KT *)aux,
				                   (const KT *)sa.kin_hi, sa.lo_slots, (unsigned short *)src, sa.tiles, sa.ctl, (const Plan *)c.plan(),
				                   st, sa.slack_cap, sa.overflow, ka);
			else
				hipLaunchKernelGGL((rsx_pass16a_kernel<KT, DIG_GENERIC>), dim3(pgrid), dim3(Pass16aCfg::BLOCK), 0, c.stream, (const KT *)aux,
				                   (const KT *)sa.kin_hi, sa.lo_slots, (unsigned short *)src, sa.tiles, sa.ctl, (const Plan *)c.plan(),
				                   st, sa.slack_cap, sa.overflow, ka);
			HIP_TRY(hipGetLastError());
			return RSX_OK;
		}
		if (dense && !env().no_pass16 && !env().no_unstable && !env().no_leaf16) {
			// round 5: the pass as a kernel of its own (rsx_pass16.hpp): values staged in two bytes, two workgroups per CU, cursors
			// instead of the chain, 16-byte stores.  (Its slots hold a bucket's values in arbitrary order: for leaves that sort.)
			const u32 *btile = sv.btile();
#define RSX_LAUNCH_P16(DIGV, CFG)                                                                                          \
	hipLaunchKernelGGL((rsx_pass16_kernel<KT, DIGV, CFG>), dim3(grid), dim3(CFG::BLOCK), 0, c.stream, (const KT *)aux,      \
	                   (const KT *)sa.kin_hi, sa.lo_slots, (unsigned short *)src, sa.tiles, btile, sa.ctl,                  \
	                   (const Plan *)c.plan(), st, sa.slack_cap, sa.overflow, ka, (u32)env().pass16_dbg)
			if (env().pass16_wgs == 1) {
				if (plain)
					RSX_LAUNCH_P16(DIG_PLAIN, Pass16Cfg<1>);
				else
					RSX_LAUNCH_P16(DIG_GENERIC, Pass16Cfg<1>);
			} else {
				if (plain)
					RSX_LAUNCH_P16(DIG_PLAIN, Pass16Cfg<2>);
				else
					RSX_LAUNCH_P16(DIG_GENERIC, Pass16Cfg<2>);
			}
#undef RSX_LAUNCH_P16
			HIP_TRY(hipGetLastError());
			return RSX_OK;
		}
		if (dense) {
			// 4-byte keys, every column kept: the leaves sort by the two low bytes and the slot says the rest -- the pass writes
			// the low half of every DERIVED key (rsx_leaf_sort_kernel, DENSE)
#define RSX_LAUNCH_SEG16(DIGV)                                                                                             \
	hipLaunchKernelGGL((rsx_scatter2_kernel<KT, NoVal, u32, C2, false, DIGV, false, uint16_t, true>), dim3(grid),           \
	                   dim3(C2::BLOCK), 0, c.stream, aux, (uint16_t *)src, (const NoVal *)nullptr, (NoVal *)nullptr, (u64)n, \
	                   shift0, (const u64 *)c.ghist(), 1u, st, ticket, ka, flags, (u64 *)nullptr,      \
	                   (const Plan *)c.plan(), pi, 0u, (const u32 *)nullptr, sa)
			if (plain)
				RSX_LAUNCH_SEG16(DIG_PLAIN);
			else
				RSX_LAUNCH_SEG16(DIG_GENERIC);
#undef RSX_LAUNCH_SEG16
			HIP_TRY(hipGetLastError());
			return RSX_OK;
		}
	}
	if (plain)
		RSX_LAUNCH_SEG(DIG_PLAIN);
	else
		RSX_LAUNCH_SEG(DIG_GENERIC);
#undef RSX_LAUNCH_SEG
	if constexpr (sizeof(KT) == 8) {
		if (blind == 2 && narrow_slots_ok<KT>(c.slack_cap)) {
			// ... and the form that writes the low word of every derived key (SegCtl::narrow decides on the device which of the
			// two works; it uses its own status words: the same region, which the form that left has not touched)
#define RSX_LAUNCH_SEG32(DIGV)                                                                                             \
	hipLaunchKernelGGL((rsx_scatter2_kernel<KT, NoVal, u32, C2, false, DIGV, false, u32, true>), dim3(grid),                \
	                   dim3(C2::BLOCK), 0, c.stream, aux, (u32 *)src, (const NoVal *)nullptr, (NoVal *)nullptr, (u64)n,     \
	                   shift0, (const u64 *)c.ghist(), 1u, st, ticket, ka, flags, (u64 *)nullptr,     \
	                   (const Plan *)c.plan(), pi, 0u, (const u32 *)nullptr, sa)
			if (pass64a_narrow_wanted<KT>(c)) {
				typedef Pass2wCfg<u32> P64;
				hipLaunchKernelGGL((rsx_pass64a_kernel<KT, u32>), dim3(P64::GRID), dim3(P64::BLOCK), 0, c.stream, (const KT *)aux,
				                   (const KT *)sa.kin_hi, sa.lo_slots, (u32 *)src, sa.tiles, sa.ctl, (const Plan *)c.plan(),
				                   st, sa.slack_cap, sa.overflow, ka);
				if (c.narrow1 && second) {
					// SegCtl::narrow == 2: the level-1 slots are four-byte places in the caller's second buffer (blind_enqueue), the
					// same element indices; what they hold is derived already
					typedef Pass64aCfgLow P64L;
					hipLaunchKernelGGL((rsx_pass64a_kernel<u32, u32, P64L>), dim3(P64L::GRID), dim3(P64L::BLOCK), 0, c.stream, (const u32 *)second,
					                   (const u32 *)nullptr, 0u, (u32 *)src, sa.tiles, sa.ctl, (const Plan *)c.plan(),
					                   st, sa.slack_cap, sa.overflow, KdfArgs<u32>{0, 0, 0});
				}
			} else if (plain)
				RSX_LAUNCH_SEG32(DIG_PLAIN);
			else
				RSX_LAUNCH_SEG32(DIG_GENERIC);
#undef RSX_LAUNCH_SEG32
		}
	}
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

// The second level of a two-level sort.  Pass 1 (by the highest kept column, src -> aux) is on its way; `plan` says so.
// Ends with the sorted keys in the buffer the reference's parity rule names (radix_sort.hpp:92); *result says which.
template <typename KT>
int sort_keys_two_level(Ctx &c, KT *src, KT *aux, size_t n, KdfArgs<KT> ka, const Plan &plan, KT **result, u32 *how)
{
	typedef Sc2Cfg<KT, NoVal> C2;
	RSX_TRY(seg_layout<KT>(c, n));
	const SegView sv(c);
	const size_t st_bytes = sv.L.st_bytes;
	SegCtl *ctl = sv.ctl();
	u32 *seghist = sv.hist();
	SegTile *tiles = sv.tiles();
	LeafSeg *segtab = sv.segtab();
	u32 *btile = sv.btile();
	KT *final = (plan.ncols & 1) ? aux : src;
	if (!c.seg_ev)
		HIP_TRY(hipEventCreateWithFlags(&c.seg_ev, hipEventDisableTiming));
	RSX_TRY(sv.reset_and_tiles(c, n, (u32)C2::TILE));
	HIP_TRY(hipGetLastError());
	// The slack attempt: evenly spread keys need no counts for the second pass.  Every (digit, digit) bucket gets a slot of
	// 1.25 times its expected size in a scratch array and the pass writes each key where the look-back chain puts it inside
	// its bucket's slot; the bucket sizes are then read off the chain, and the leaves gather from the slots into the dense
	// result.  One read of the keys less than the counted path below (rsx_seg_hist1_kernel: 0.25 of 2.1 ms at 2^28 keys).
	// A slot that overflows (keys clustered after all) only costs the attempt: pass 1's output in `aux` is untouched.
	c.slack_cap = 0;
	if (!env().no_slack && n >= ((size_t)1 << 26)) {
		const u32 mean = (u32)(n >> 16);
		const u32 cap = slot_cap_for(mean);
		if (cap <= (u32)LeafShapes<KT>::Big::CAP && c.slack.ensure(((size_t)65536 * cap + C2::TILE) * sizeof(KT)) == RSX_OK) {
			c.slack_cap = cap;
			RSX_TRY(launch_seg_pass<KT>(c, aux, src, n, ka, -2));
			hipLaunchKernelGGL((rsx_seg_slack_plan_kernel<u32>), dim3(256), dim3(256), 0, c.stream,
			                   (const u32 *)sv.cursors(0), (const u32 *)btile, (const u64 *)c.ghist(),
			                   (const Plan *)c.plan(), ctl, segtab, cap, c.dev_host_segctl);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c.seg_ev, c.stream));
			RSX_TRY(launch_leaves<KT>(c, src, aux, n, ka, HYB_TWO_LEVEL, LeafShapes<KT>::shape_for_slots(cap)));
			HIP_TRY(hipEventSynchronize(c.seg_ev));
			if (c.host_segctl->mode == SEG_MODE_LEAVES) {
				*result = final;
				*how = 4u;
				return RSX_OK;
			}
			// a slot overflowed: the counted path, from `aux` again
			c.slack_cap = 0;
			RSX_TRY(sv.reset_and_tiles(c, n, (u32)C2::TILE));
		} else {
			(void)hipGetLastError();
		}
	}
	{
		ProfScope prof(0, (u64)n * sizeof(KT), c.stream);
		hipLaunchKernelGGL((rsx_seg_hist1_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, (const KT *)aux, (const SegTile *)tiles,
		                   (const SegCtl *)ctl, (const Plan *)c.plan(), ka, seghist);
	}
	hipLaunchKernelGGL((rsx_seg_plan_kernel<KT>), dim3(256), dim3(256), 0, c.stream, seghist, (const u64 *)c.ghist(), (u64)n,
	                   (const Plan *)c.plan(), ctl, segtab, (u32)LeafShapes<KT>::Big::CAP, c.dev_host_segctl, 0u);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c.seg_ev, c.stream));
	// the pass by the level-2 column and the small leaves are enqueued before the host knows whether the (digit, digit)
	// buckets fit leaves: they do nothing if not
	RSX_TRY(launch_seg_pass<KT>(c, aux, src, n, ka, -1));
	RSX_TRY(launch_leaves<KT>(c, src, aux, n, ka, HYB_TWO_LEVEL, 1u));
	HIP_TRY(hipEventSynchronize(c.seg_ev));
	const SegCtl hc = *c.host_segctl;
	if (hc.mode == SEG_MODE_LEAVES) {
		if (hc.maxleaf > (u32)LeafShapes<KT>::Small::CAP)   // (rare: the leaves need a larger shape)
			RSX_TRY(launch_leaves<KT>(c, src, aux, n, ka, HYB_TWO_LEVEL, LeafShapes<KT>::shape_for(hc.maxleaf)));
	} else {
		// keys clustered in their top two columns: one pass per remaining column inside the level-1 buckets, LSB first
		// (the counts of the columns below the level-2 one are only made now)
		if (plan.ncols > 2) {
			ProfScope prof(0, (u64)n * sizeof(KT), c.stream);
			hipLaunchKernelGGL((rsx_seg_hist_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, (const KT *)aux, (const SegTile *)tiles,
			                   (const SegCtl *)ctl, (const Plan *)c.plan(), ka, seghist);
		}
		hipLaunchKernelGGL((rsx_seg_plan_kernel<KT>), dim3(256), dim3(256), 0, c.stream, seghist, (const u64 *)c.ghist(), (u64)n,
		                   (const Plan *)c.plan(), ctl, segtab, 0u, (SegCtl *)nullptr, 1u);
		if (plan.ncols > 2)
			HIP_TRY(hipMemsetAsync(sv.status(1), 0, (plan.ncols - 2) * st_bytes, c.stream));
		for (u32 j = 0; j + 1 < plan.ncols; ++j)
			RSX_TRY(launch_seg_pass<KT>(c, aux, src, n, ka, (int)j));
	}
	*result = final;
	*how = hc.mode == SEG_MODE_LEAVES ? 2u : 3u;
	return RSX_OK;
}

// ---- two MSB passes and leaves for key + payload sorts and rank sorts (4-byte keys, 4-byte payloads; rsx_leaf_pairs_kernel) ----
template <typename KT> HybCaps hybrid_caps_pairs(size_t n, size_t val_bytes_, bool counted_too = false)
{
	HybCaps caps{0, 0, 0, 0};
	if (sizeof(KT) != 4 || val_bytes_ != 4 || !hybrid_enabled())
		return caps;
	// one level where every bucket of the highest kept column fits the pairs' leaf (5120 pairs: up to about a million pairs)
	caps.cap1 = 5120;
	caps.min_cols1 = 3;
	// two levels: the slack route, and only where a slot fits the pairs' leaf shape: 2^27 .. 2^28 pairs (cfg 4); key + payload
	// sorts (counted_too) with RSX_NO_SLACK=1: the second pass counted first, as for keys alone (pairs_two_level)
	if ((!env().no_slack || counted_too) && n >= ((size_t)1 << env().two_level_min_log2) && n <= ((size_t)1 << 28)) {
		caps.cap2 = (u32)LeafShapes<KT>::Small::CAP;
		caps.min_cols2 = 4;
	}
	return caps;
}

// Pass 1 (by the highest kept column) has written (k1, v1).  The second pass goes into slots, the leaves write the payloads
// (and the keys, if kfinal) to (kfinal, vfinal).  *ok = false: a slot overflowed -- nothing the caller owns was written, it
// sorts with one pass per column.
// RSX_NO_SLACK=1 (key + payload sorts only: kdense / vdense are their first buffers, which pass 1 has read): the counted second
// pass of sort_keys_two_level -- the level-2 column counted per bucket (rsx_seg_hist1_kernel), the pass (k1, v1) -> (kdense,
// vdense) at those offsets, the leaves on the dense buckets.  *ok = false: a (digit, digit) bucket does not fit the pairs' leaf --
// known before the pass is enqueued, nothing but (k1, v1) has been written.
template <typename KT, typename VT>
int pairs_two_level(Ctx &c, const KT *k1, const VT *v1, KT *kfinal, VT *vfinal, size_t n, KdfArgs<KT> ka, bool *ok,
                    KT *kdense = nullptr, VT *vdense = nullptr)
{
	typedef Sc2Cfg<KT, VT> C2;
	typedef LeafCfg<u32, 4, 20, 3> L;   // 5120 pairs: the slack slot of 2^28 pairs; three workgroups per CU
	*ok = false;
	RSX_TRY(seg_layout<KT>(c, n));   // (Sc2Cfg<KT, NoVal> and <KT, VT> have the same tile: 32 Ki elements)
	static_assert((int)C2::TILE == (int)Sc2Cfg<KT, NoVal>::TILE, "one layout for both");
	static_assert(sizeof(KT) == 4, "the pairs' leaves take 4-byte keys");
	const SegView sv(c);
	const u64 rows = sv.L.rows;
	SegCtl *ctl = sv.ctl();
	SegTile *tiles = sv.tiles();
	LeafSeg *segtab = sv.segtab();
	u32 *btile = sv.btile();
	if (env().no_slack) {
		if (!kdense || !vdense || !kfinal)
			return RSX_OK;
		u32 *seghist = sv.hist();
		if (!c.seg_ev)
			HIP_TRY(hipEventCreateWithFlags(&c.seg_ev, hipEventDisableTiming));
		c.host_segctl->mode = SEG_MODE_NONE;
		RSX_TRY(sv.reset_and_tiles(c, n, (u32)C2::TILE));
		{
			ProfScope prof(0, (u64)n * sizeof(KT), c.stream);
			hipLaunchKernelGGL((rsx_seg_hist1_kernel<KT>), dim3(512), dim3(1024), 0, c.stream, k1, (const SegTile *)tiles, (const SegCtl *)ctl,
			                   (const Plan *)c.plan(), ka, seghist);
		}
		hipLaunchKernelGGL((rsx_seg_plan_kernel<KT>), dim3(256), dim3(256), 0, c.stream, seghist, (const u64 *)c.ghist(), (u64)n,
		                   (const Plan *)c.plan(), ctl, segtab, (u32)L::CAP, c.dev_host_segctl, 0u);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(c.seg_ev, c.stream));
		HIP_TRY(hipEventSynchronize(c.seg_ev));
		if (c.host_segctl->mode != SEG_MODE_LEAVES)
			return RSX_OK;
		const SegArgs sa = sv.args(sizeof(KT));
		{
			ProfScope prof(1, (u64)n * 2 * (sizeof(KT) + sizeof(VT)), c.stream);
			hipLaunchKernelGGL((rsx_scatter2_kernel<KT, VT, u32, C2, false, DIG_GENERIC, false, KT, true>), dim3((unsigned)rows),
			                   dim3(C2::BLOCK), 0, c.stream, k1, kdense, v1, vdense, (u64)n, 0u, (const u64 *)c.ghist(), 1u,
			                   sv.cursors(0), sv.status(0), ka, (u32)SCATTER_SEG_LEAVES, (u64 *)nullptr, (const Plan *)c.plan(), 0u, 0u,
			                   (const u32 *)nullptr, sa);
		}
		{
			ProfScope prof(2, (u64)n * 2 * (sizeof(KT) + sizeof(VT)), c.stream);
			hipLaunchKernelGGL((rsx_leaf_pairs_kernel<KT, VT, L>), dim3(env().leaf_grid), dim3(L::BLOCK), 0, c.stream, (const KT *)kdense,
			                   (const VT *)vdense, 0u, kfinal, vfinal, (const Plan *)c.plan(), (const LeafSeg *)segtab, (const SegCtl *)ctl,
			                   ka);
		}
		HIP_TRY(hipGetLastError());
		*ok = true;
		return RSX_OK;
	}
	const u32 mean = (u32)(n >> 16);
	const u32 cap = slot_cap_for(mean);
	if (cap > (u32)L::CAP)
		return RSX_OK;
	if (c.slack.ensure(((size_t)65536 * cap + C2::TILE) * sizeof(KT)) != RSX_OK ||
	    c.slack_v.ensure(((size_t)65536 * cap + C2::TILE) * sizeof(VT)) != RSX_OK) {
		(void)hipGetLastError();
		return RSX_OK;   // (no room for the slots: one pass per column)
	}
	if (!c.seg_ev)
		HIP_TRY(hipEventCreateWithFlags(&c.seg_ev, hipEventDisableTiming));
	RSX_TRY(sv.reset_and_tiles(c, n, (u32)C2::TILE));
	SegArgs sa = sv.args(sizeof(KT));
	sa.slack_cap = cap;
	{
		ProfScope prof(1, (u64)n * 2 * (sizeof(KT) + sizeof(VT)), c.stream);
		hipLaunchKernelGGL((rsx_scatter2_kernel<KT, VT, u32, C2, false, DIG_GENERIC, false, KT, true>), dim3((unsigned)rows),
		                   dim3(C2::BLOCK), 0, c.stream, k1, (KT *)c.slack.p, v1, (VT *)c.slack_v.p, (u64)n, 0u, (const u64 *)c.ghist(), 1u,
		                   sv.cursors(0), sv.status(0), ka, (u32)SCATTER_SEG_SLACK, (u64 *)nullptr, (const Plan *)c.plan(), 0u, 0u,
		                   (const u32 *)nullptr, sa);
	}
	hipLaunchKernelGGL((rsx_seg_slack_plan_kernel<u32>), dim3(256), dim3(256), 0, c.stream, (const u32 *)sv.cursors(0), (const u32 *)btile,
	                   (const u64 *)c.ghist(), (const Plan *)c.plan(), ctl, segtab, cap, c.dev_host_segctl);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c.seg_ev, c.stream));
	{
		ProfScope prof(2, (u64)n * (sizeof(KT) + 2 * sizeof(VT) + (kfinal ? sizeof(KT) : 0)), c.stream);
		hipLaunchKernelGGL((rsx_leaf_pairs_kernel<KT, VT, L>), dim3(env().leaf_grid), dim3(L::BLOCK), 0, c.stream, (const KT *)c.slack.p,
		                   (const VT *)c.slack_v.p, cap, kfinal, vfinal, (const Plan *)c.plan(), (const LeafSeg *)segtab,
		                   (const SegCtl *)ctl, ka);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventSynchronize(c.seg_ev));
	*ok = c.host_segctl->mode == SEG_MODE_LEAVES;
	return RSX_OK;
}

// One MSB pass has written (k1, v1); the 256 buckets' pairs sorted by the remaining columns into (kfinal, vfinal).
template <typename KT, typename VT>
int pairs_one_level(Ctx &c, const KT *k1, const VT *v1, KT *kfinal, VT *vfinal, size_t n, KdfArgs<KT> ka)
{
	typedef LeafCfg<u32, 4, 20, 3> L;
	ProfScope prof(2, (u64)n * (sizeof(KT) + 2 * sizeof(VT) + (kfinal ? sizeof(KT) : 0)), c.stream);
	hipLaunchKernelGGL((rsx_leaf_pairs_kernel<KT, VT, L>), dim3(256), dim3(L::BLOCK), 0, c.stream, k1, v1, 0u, kfinal, vfinal,
	                   (const Plan *)c.plan(), (const LeafSeg *)nullptr, (const SegCtl *)nullptr, ka, (u32)HYB_ONE_LEVEL,
	                   (const u64 *)c.ghist(), (u64)n);
	HIP_TRY(hipGetLastError());
	return RSX_OK;
}

}   // namespace
