// rsx_env.hpp: the RSX_* switches of the environment (Env, env()) -- part of librsx.so's host side, included by rsx.hip (one
// translation unit).  Nothing of HIP is used here: tests/cpp/env_check.cpp includes this file alone and drives Env::load() on the CPU.
#pragma once

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <mutex>

namespace {

// ---- the RSX_* switches of the environment, read ONCE per process (rsx_reload_env() reads them again: tests) ----------------
// "set" switches are on when the variable exists, "=1" switches when its value starts with '1' (as documented in rsx.h).
std::atomic<uint32_t> g_env_epoch{0};   // bumped by rsx_reload_env()
// rsx_sort_unique*: the widest bitmap the library was compiled for, and the widest it takes by default
enum : unsigned { UNIQUE_MAX_BITS_COMPILED = 30, UNIQUE_MAX_BITS_DEFAULT = 24 };
// rsx_sort_group*: the same for the bitmap its rank cells stand on
enum : unsigned { GROUP_MAX_BITS_COMPILED = 30, GROUP_MAX_BITS_DEFAULT = 24 };
// rsx_sort_lex*: neighbouring columns are packed into one key of at most this many bytes
enum : unsigned { LEX_PACK_BYTES_DEFAULT = 4 };
// rsx_sort_locate*: the search route takes at most this many distinct values
enum : unsigned { LOCATE_MAX_VALUES_DEFAULT = 4096 };
// rsx_sort_reduce*: the widest table of cells the library was compiled for (in LDS, in device memory) and the widest it takes by
// default -- the LDS cut-off: the cells in device memory lost to the sort route in every measured row
enum : unsigned { REDUCE_LDS_BITS_COMPILED = 12, REDUCE_MAX_BITS_COMPILED = 24, REDUCE_MAX_BITS_DEFAULT = 12 };
// rsx_sort_partition*: the scatter route takes at most this many distinct edges by default (the measured cut-off: beyond it the sort
// route won some row of the probe; the kernels take 255), and ranks by ballots up to this many parts (the shape
// header's own copy of the second is PARTITION_BALLOT_PARTS_DEFAULT)
enum : unsigned { PARTITION_MAX_EDGES_COMPILED = 255, PARTITION_MAX_EDGES_DEFAULT = 3, PARTITION_BALLOT_PARTS_ENV_DEFAULT = 7 };
// rsx_sort_segments*: the most long segments the host loop of the MIXED route may be asked to take and how many it takes by default
// (the largest count at which MIXED still beat the baseline on the probe's CSR shape); the size classes (bits 1 << class,
// rsx_segments_shape.hpp) in which the LDS route is the default: BLOCK, which beat the baseline 6 .. 8x -- WAVE lost with rows of 16 keys
// and GROUP has no row of its own in the probe; those run under RSX_SEGMENTS_FORCE=1
enum : unsigned { SEGMENTS_MAX_LONG_COMPILED = 4096, SEGMENTS_MAX_LONG_DEFAULT = 8, SEGMENTS_DEFAULT_CLASSES = 8 };
struct Env {
	bool host_register = false;      // RSX_HOST_REGISTER=1
	bool force_table_rank = false;   // RSX_FORCE_TABLE_RANK=1
	bool verify = false;             // RSX_VERIFY=1
	bool verify_whole = false;       // RSX_VERIFY=2: keys-only sorts check their whole result (sortedness + checksums), any route
	bool verify_inject = false;      // RSX_VERIFY_INJECT (set)
	bool no_hot = false;             // RSX_NO_HOT (set)
	bool elem_loads = false;         // RSX_ELEM_LOADS=1
	bool no_small_tiles = false;     // RSX_NO_SMALL_TILES (set)
	bool no_hybrid = false;          // RSX_NO_HYBRID=1
	bool no_small_sort = false;      // RSX_NO_SMALL_SORT (set)
	bool no_fill_runs = false;       // RSX_NO_FILL_RUNS (set)
	bool no_speculation = false;     // RSX_NO_SPECULATION (set)
	bool compact_bits = false;       // RSX_COMPACT_BITS=1
	bool no_narrow_keys = false;     // RSX_NO_NARROW_KEYS (set)
	bool no_host_small = false;      // RSX_NO_HOST_SMALL (set)
	bool no_fused_hist = false;      // RSX_NO_FUSED_HIST=1
	bool no_slack = false;           // RSX_NO_SLACK=1
	bool no_self_plan = false;       // RSX_NO_SELF_PLAN=1
	bool no_blind = false;           // RSX_NO_BLIND=1: every sort starts with the histogram
	unsigned blind_min_log2 = 0;     // RSX_BLIND_MIN_LOG2: keys-only sorts may skip the histogram from 2^this keys on (0: the measured floors)
	bool no_leaf_prefix = false;     // RSX_NO_LEAF_PREFIX=1: leaves of 8-byte keys sort by every column they have left (rsx_hybrid.hpp)
	bool no_leaf16w2k = false;       // RSX_NO_LEAF16W2K=1: slots of 1025 .. 2048 values take a 128-thread workgroup per leaf (rsx_leaf16_kernel) instead of a wave
	bool no_leaf16q = false;         // RSX_NO_LEAF16Q=1: slots of up to 256 values take a wave per leaf (rsx_leaf16w_kernel) instead of a row of sixteen lanes
	bool no_narrow_slots = false;    // RSX_NO_NARROW_SLOTS=1: the level-2 slots of 8-byte keys always hold whole keys (SegCtl::narrow)
	bool no_aux_slots = false;       // RSX_NO_AUX_SLOTS=1: the level-1 slots of a sort without a histogram all lie in scratch memory
	bool no_narrow1 = false;         // RSX_NO_NARROW_LEVEL1=1: the level-1 pass of 8-byte keys always writes whole keys (SegCtl::narrow stays below 2)
	bool no_dense_slots = false;     // RSX_NO_DENSE_SLOTS=1: the level-2 pass of a sort without a histogram writes whole keys
	bool force_dense_slots = false;  // RSX_DENSE_SLOTS=1: (kept for old scripts: two-byte slots are now written for every slot size rsx_leaf16_kernel takes)
	bool no_unstable = false;        // RSX_NO_UNSTABLE=1: the MSB passes of a sort without a histogram rank per wave (stable), as every other pass
	bool no_shift = false;           // RSX_NO_SHIFT=1: the MSB digits of a sort without a histogram are whole bytes (the two highest kept columns) always
	bool no_pass16 = false;          // RSX_NO_PASS16=1: the level-2 pass into two-byte slots is rsx_scatter2_kernel<..., KTO = u16, SEG> as in round 4 (rsx_pass16.hpp)
	unsigned pass16_wgs = 2;         // RSX_PASS16_WGS=1: ... one workgroup per CU (probe)
	bool no_packed_keys = false;     // RSX_NO_PACKED_KEYS=1: rank sorts without a histogram go by byte columns only (SegCtl::compact never set)
	bool no_pass32a = false;         // RSX_NO_PASS32A=1: the level-1 pass of such a sort is rsx_scatter2_kernel<..., SEG> with its look-back chain (rsx_pass32.hpp)
	unsigned pass32_min_mi = 0;      // RSX_PASS32_MIN_MI=k (probe): the level-1 atom pass from k Mi keys on (default: 52 Mi 4-byte keys, 24 Mi 8-byte keys)
	int pass32_prefetch = -1;        // RSX_PASS32_PREFETCH=0|1 (probe): rsx_pass32a_kernel requests a tile's keys while it writes the tile before (1) or when it starts on the tile (0, the default)
	bool no_pass16a = false;         // RSX_NO_PASS16A=1: ... whose runs are ragged (rsx_pass16_kernel) instead of whole 64-byte atoms (rsx_pass16a_kernel)
	unsigned pass16_dbg = 0;         // RSX_PASS16_DBG=1|2 (probe, WRONG OUTPUT): no stores / only whole aligned 64-byte atoms stored
	bool no_leafc = false;           // RSX_NO_LEAFC=1: no two-byte slots of more than 5120 values (rsx_leafc.hpp): sorts without a histogram of 4-byte keys end below 2^30 keys and their larger leaves sort whole keys, as in round 4
	unsigned force_leafc = 0;        // RSX_FORCE_LEAFC=1..6 (tests): two-byte slots of ANY size take the leaves of the large ones -- 1 the counting leaves at once, 2 / 3 / 4 / 5 / 6 rsx_leaf16_kernel's 10240- / 20480- / 6144- / 7680- / 15360-value shape and the counting leaves behind it
	bool no_leaf16 = false;          // RSX_NO_LEAF16=1: two-byte slots are sorted by rsx_leaf_sort_kernel (two LDS passes) as in round 3
	unsigned leaf16_maxbin = 25;     // RSX_LEAF16_MAXBIN (tests): leaves with a fuller bin go to rsx_leaf_sort_kernel (0: every leaf)
	unsigned leaf_grid = 65536;      // RSX_LEAF_GRID (probe): workgroups of a level-2 leaf launch (65536: one per table entry)
	unsigned two_level_min_log2 = 27; // RSX_TWO_LEVEL_MIN_LOG2: two MSB passes + leaves from 2^this keys on (tests: 22)
	bool no_odd_stride = false;      // RSX_NO_ODD_STRIDE=1: the level-1 slots of a sort without a histogram lie 1.25 means apart, rounded to 1 KiB, as in round 5
	unsigned cap1_pad_kib = 0;       // RSX_CAP1_PAD_KIB=k (probe): k KiB more per level-1 slot of a sort without a histogram
	unsigned probe = 0;              // RSX_PROBE=bits (measurements; results stay right): 1 the leaf table of a sort without a histogram in reverse slot order, 4 every device-scheduled sort as if hinted (rsx_sort_inplace_async_hint)
	bool no_pass64a = false;         // RSX_NO_PASS64A=1: the level-2 pass of 8-byte keys into four-byte slots is the chained rsx_scatter2_kernel of round 4 (rsx_pass64.hpp)
	bool no_log = false;             // RSX_NO_LOG=1: 8-byte keys never take the (bit length, mantissa) digits of rsx_logroute.hpp (rsx_info.hybrid never 6)
	bool log_leaf_big = false;       // RSX_LOG_LEAF_BIG=1 (tests): that route's leaves in the shape for 10240 values at every size
	bool pairs_leaf_big = false;     // RSX_PAIRS_LEAF_BIG=1 (tests): key + payload and rank sorts without a histogram: the leaves' shape for 10240 pairs at every size
	unsigned log_min_log2 = 0;       // RSX_LOG_MIN_LOG2: ... from 2^this keys on (tests: 20; default: from 24 Mi keys)
	unsigned unique_max_bits = UNIQUE_MAX_BITS_DEFAULT;   // RSX_UNIQUE_MAX_BITS=k: rsx_sort_unique*: the widest bitmap is 2^k bits (0: never a bitmap or a table; at most 30)
	unsigned group_max_bits = GROUP_MAX_BITS_DEFAULT;     // RSX_GROUP_MAX_BITS=k: rsx_sort_group*: the widest bitmap under the rank cells is 2^k bits (0: never a bitmap, cells or a table; at most 30)
	bool rankdata_no_tables = false; // RSX_RANKDATA_NO_TABLES=1 (tests, probe): rsx_sort_rankdata* always takes the sort route (no column table, no count table)
	unsigned nth_force = 0;          // RSX_NTH_FORCE=1: rsx_sort_nth* selects whenever n >= 2 and 1 <= distinct ranks <= 64; =2: always the sort route
	unsigned topk_force = 0;         // RSX_TOPK_FORCE=1: rsx_sort_topk* selects whenever n >= 2 and 0 < k <= n; =2: always the sort route
	unsigned locate_force = 0;       // RSX_LOCATE_FORCE=2: rsx_sort_locate* always takes the sort route
	unsigned locate_max_values = LOCATE_MAX_VALUES_DEFAULT;   // RSX_LOCATE_MAX_VALUES=k (1 .. 4096; tests): rsx_sort_locate* searches while there are at most k distinct values
	unsigned locate_counter_sets = 0; // RSX_LOCATE_COUNTER_SETS=k (tests, probe): the search kernel keeps k sets of LDS counters (0: as many as fit, at most 32)
	unsigned reduce_max_bits = REDUCE_MAX_BITS_DEFAULT;   // RSX_REDUCE_MAX_BITS=k (0 .. 24): rsx_sort_reduce* accumulates into cells while at most k bits of the keys vary (0: never)
	unsigned reduce_lds_bits = REDUCE_LDS_BITS_COMPILED;  // RSX_REDUCE_LDS_BITS=k (0 .. 12): ... and keeps the cells in LDS while at most k do (beyond: in device memory)
	unsigned reduce_replicas = 0;    // RSX_REDUCE_REPLICAS=k (tests, probe): the cells kernel keeps k copies of the cells in LDS (0: as many as fit, at most 32)
	unsigned reduce_force = 0;       // RSX_REDUCE_FORCE=2: rsx_sort_reduce* always takes the sort route
	unsigned join_force = 0;         // RSX_JOIN_FORCE=2: rsx_sort_join* always searches the left keys as they come; =3: always sorts the left side too
	bool join_no_table = false;      // RSX_JOIN_NO_TABLE=1: rsx_sort_join* never takes the table route
	unsigned lex_pack_bytes = LEX_PACK_BYTES_DEFAULT;   // RSX_LEX_PACK_BYTES=k (1 .. 8): rsx_sort_lex* packs columns into keys of at most k bytes (1: one sort per column)
	unsigned partition_force = 0;    // RSX_PARTITION_FORCE=2: rsx_sort_partition* always takes the sort route
	unsigned partition_max_edges = PARTITION_MAX_EDGES_DEFAULT;     // RSX_PARTITION_MAX_EDGES=k (1 .. 255; default 3): rsx_sort_partition* scatters while there are at most k distinct edges
	unsigned partition_ballot_parts = PARTITION_BALLOT_PARTS_ENV_DEFAULT;   // RSX_PARTITION_BALLOT_PARTS=k (0 .. 256; default 7): ... and ranks a tile by one ballot per part while there are at most k parts (beyond: per-wave cells in LDS)
	unsigned segments_force = 0;     // RSX_SEGMENTS_FORCE=1: rsx_sort_segments* sorts in LDS (and the long segments one by one) wherever that is possible at all; =2: always the composed route
	unsigned segments_max_long = SEGMENTS_MAX_LONG_DEFAULT;   // RSX_SEGMENTS_MAX_LONG=k (0 .. 4096): ... and takes at most k segments too long for LDS one by one (beyond: the composed route)
	// What a variable's text means.  An absent variable leaves the member's default initialiser, which load() restores first:
	// rsx_reload_env() after a test has taken its variable away is back at the default.
	static bool is_set(const char *name) { return getenv(name) != nullptr; }
	static unsigned one_or_two(const char *name)   // the first character: '1' -> 1, '2' -> 2, anything else (or absent) -> 0
	{
		const char *e = getenv(name);
		return !e ? 0u : e[0] == '1' ? 1u : e[0] == '2' ? 2u : 0u;
	}
	static bool is_one(const char *name) { return one_or_two(name) == 1; }
	static void number(const char *name, unsigned *x, int lo = INT_MIN, int hi = INT_MAX)   // atoi, brought into [lo, hi]
	{
		if (const char *e = getenv(name))
			*x = (unsigned)std::max(lo, std::min(hi, atoi(e)));
	}
	static void within(const char *name, unsigned *x, int lo, int hi)   // atoi, taken only inside [lo, hi]
	{
		const char *e = getenv(name);
		if (e && atoi(e) >= lo && atoi(e) <= hi)
			*x = (unsigned)atoi(e);
	}
	static void one_else_two(const char *name, unsigned *x)   // atoi: 1 -> 1, anything else -> 2
	{
		if (const char *e = getenv(name))
			*x = atoi(e) == 1 ? 1u : 2u;
	}
	void load()
	{
		*this = Env{};
		host_register = is_one("RSX_HOST_REGISTER");
		force_table_rank = is_one("RSX_FORCE_TABLE_RANK");
		verify = one_or_two("RSX_VERIFY") == 1;
		verify_whole = one_or_two("RSX_VERIFY") == 2;
		verify_inject = is_set("RSX_VERIFY_INJECT");
		no_hot = is_set("RSX_NO_HOT");
		elem_loads = is_one("RSX_ELEM_LOADS");
		no_small_tiles = is_set("RSX_NO_SMALL_TILES");
		no_hybrid = is_one("RSX_NO_HYBRID");
		no_small_sort = is_set("RSX_NO_SMALL_SORT");
		no_fill_runs = is_set("RSX_NO_FILL_RUNS");
		no_speculation = is_set("RSX_NO_SPECULATION");
		compact_bits = is_one("RSX_COMPACT_BITS");
		no_narrow_keys = is_set("RSX_NO_NARROW_KEYS");
		no_host_small = is_set("RSX_NO_HOST_SMALL");
		no_fused_hist = is_one("RSX_NO_FUSED_HIST");
		no_slack = is_one("RSX_NO_SLACK");
		no_self_plan = is_one("RSX_NO_SELF_PLAN");
		no_blind = is_one("RSX_NO_BLIND");
		number("RSX_BLIND_MIN_LOG2", &blind_min_log2, 22, 30);
		no_leaf_prefix = is_one("RSX_NO_LEAF_PREFIX");
		no_leaf16q = is_one("RSX_NO_LEAF16Q");
		no_narrow_slots = is_one("RSX_NO_NARROW_SLOTS");
		no_aux_slots = is_one("RSX_NO_AUX_SLOTS");
		no_narrow1 = is_one("RSX_NO_NARROW_LEVEL1");
		no_dense_slots = is_one("RSX_NO_DENSE_SLOTS");
		force_dense_slots = is_one("RSX_DENSE_SLOTS");
		no_leaf16 = is_one("RSX_NO_LEAF16");
		no_leafc = is_one("RSX_NO_LEAFC");
		no_leaf16w2k = is_one("RSX_NO_LEAF16W2K");
		number("RSX_PASS32_MIN_MI", &pass32_min_mi);
		if (is_set("RSX_PASS32_PREFETCH"))
			pass32_prefetch = is_one("RSX_PASS32_PREFETCH");
		number("RSX_FORCE_LEAFC", &force_leafc);
		no_pass16 = is_one("RSX_NO_PASS16");
		no_pass16a = is_one("RSX_NO_PASS16A");
		no_pass32a = is_one("RSX_NO_PASS32A");
		no_packed_keys = is_one("RSX_NO_PACKED_KEYS");
		one_else_two("RSX_PASS16_WGS", &pass16_wgs);
		number("RSX_PASS16_DBG", &pass16_dbg);
		no_shift = is_one("RSX_NO_SHIFT");
		no_unstable = is_one("RSX_NO_UNSTABLE");
		number("RSX_LEAF16_MAXBIN", &leaf16_maxbin, 0, 25);
		number("RSX_LEAF_GRID", &leaf_grid, 256, 65536);
		no_odd_stride = is_one("RSX_NO_ODD_STRIDE");
		number("RSX_CAP1_PAD_KIB", &cap1_pad_kib, 0, 65536);
		number("RSX_PROBE", &probe);
		no_pass64a = is_one("RSX_NO_PASS64A");
		no_log = is_one("RSX_NO_LOG");
		log_leaf_big = is_one("RSX_LOG_LEAF_BIG");
		pairs_leaf_big = is_one("RSX_PAIRS_LEAF_BIG");
		number("RSX_LOG_MIN_LOG2", &log_min_log2, 20, 29);
		rankdata_no_tables = is_one("RSX_RANKDATA_NO_TABLES");
		topk_force = one_or_two("RSX_TOPK_FORCE");
		nth_force = one_or_two("RSX_NTH_FORCE");
		locate_force = one_or_two("RSX_LOCATE_FORCE");
		within("RSX_LOCATE_MAX_VALUES", &locate_max_values, 1, (int)LOCATE_MAX_VALUES_DEFAULT);
		within("RSX_LOCATE_COUNTER_SETS", &locate_counter_sets, 1, 32);
		within("RSX_LEX_PACK_BYTES", &lex_pack_bytes, 1, 8);
		partition_force = one_or_two("RSX_PARTITION_FORCE");
		within("RSX_PARTITION_MAX_EDGES", &partition_max_edges, 1, (int)PARTITION_MAX_EDGES_COMPILED);
		within("RSX_PARTITION_BALLOT_PARTS", &partition_ballot_parts, 0, 256);
		segments_force = one_or_two("RSX_SEGMENTS_FORCE");
		within("RSX_SEGMENTS_MAX_LONG", &segments_max_long, 0, (int)SEGMENTS_MAX_LONG_COMPILED);
		number("RSX_REDUCE_MAX_BITS", &reduce_max_bits, 0, (int)REDUCE_MAX_BITS_COMPILED);
		number("RSX_REDUCE_LDS_BITS", &reduce_lds_bits, 0, (int)REDUCE_LDS_BITS_COMPILED);
		within("RSX_REDUCE_REPLICAS", &reduce_replicas, 1, 32);
		reduce_force = one_or_two("RSX_REDUCE_FORCE");
		within("RSX_JOIN_FORCE", &join_force, 2, 3);
		join_no_table = is_one("RSX_JOIN_NO_TABLE");
		number("RSX_UNIQUE_MAX_BITS", &unique_max_bits, 0, (int)UNIQUE_MAX_BITS_COMPILED);
		number("RSX_GROUP_MAX_BITS", &group_max_bits, 0, (int)GROUP_MAX_BITS_COMPILED);
		within("RSX_TWO_LEVEL_MIN_LOG2", &two_level_min_log2, 22, 30);
	}
};
Env g_env;
std::once_flag g_env_once;
inline const Env &env()
{
	std::call_once(g_env_once, [] { g_env.load(); });
	return g_env;
}

}  // namespace
