/*
 * rsx.h -- C ABI of the MI355X-native LSD radix sort (librsx.so).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference has
 * no FFI: its surface is the header-only templates
 *
 *     T*       radix_sort(T* src, T* aux, size_t n, KeyFunc&& kf = basic_kdfs::kdf)
 *                                                           radix_sort.hpp:98-99
 *     IdxType* radix_sort_rank(const T* src, IdxType* index_buffer, size_t n, KeyFunc&& kf)
 *                                                           radix_sort_rank.hpp:97-98
 *     T*       rs_sort_main(src, aux, n, Hist&, kf)         radix_sort.hpp:31-32
 *
 * include/radix_sort.hpp, radix_sort_rank.hpp and radix_sort_basic_kdf.hpp in
 * this directory re-create those templates on top of the functions below
 * (see INTEGRATION.md).  All entry points use plain pointers and sizes only.
 *
 * Conventions
 *   - Return value: 0 on success, a negative RSX_E* code on failure;
 *     rsx_last_error() gives the message for the calling thread.  There is no
 *     CPU fallback: without a usable gfx950 device every sort call fails with
 *     RSX_ENODEVICE.
 *   - "Returned pointer" rule (radix_sort.hpp:89,:92): the result is in `src`
 *     when the number of kept (non-constant) 8-bit key columns is even, in
 *     `aux` when it is odd; n < 2 and already-sorted inputs return `src` and
 *     leave `aux` untouched (radix_sort.hpp:37-38,:60-62).  The buffer that is
 *     not returned has unspecified contents except in those early exits.
 *   - Order is a stable sort by kdf(key): output element images are bit-exact
 *     copies of the input's (NaN payloads, -0.0), radix_sort.hpp:85-87.
 *
 * Scratch memory.  The reference allocates nothing (radix_sort.hpp:98-115: two caller buffers, counters on the stack).
 *   This library keeps, per (device, stream) and until rsx_release / rsx_release_stream: status words of the look-back
 *   chains (1 KiB per 32 Ki-key tile and pass), and -- for the sorts without a histogram, which large evenly spread arrays
 *   take (rsx_info.hybrid == 5) -- slots: 256 x 1.25 n / 256 keys for the first MSB pass, of which the 204 that fit lie in the
 *   caller's SECOND buffer (keys-only sorts: the sample has proven the input unsorted before anything is written, so that
 *   buffer belongs to the sort as in the reference, radix_sort.hpp:82-92; the early exits leave it untouched as before) and
 *   the other 52 -- 0.25 n keys -- in scratch memory, and 65536 slots of 1.25 n / 65536 keys for the second pass (two bytes per
 *   key for 4-byte keys: 0.63 n keys' worth -- keys-only sorts of 4-byte keys up to 2^31 keys, round 5).  Key + payload and rank
 *   sorts (round 6): the level-1 slots of keys and payloads likewise in the spare buffers -- the second key and payload
 *   buffers; of a rank sort the index buffer's second half for the keys and its first half, until the ranks are written there,
 *   for the indices -- and, for the second pass, slots of two bytes per key and whole payloads in scratch memory (the two MSB
 *   digits are the slot, no leaf looks at more of a key than the two bytes below them).  A buffer's first allocation is
 *   what the sort needs; one that has to GROW grows in steps of an eighth of the next power of two (a slightly larger n does
 *   not reallocate again), the new one is allocated before the old one is freed, and nothing grows or is released inside a
 *   stream capture or a *_inplace_async call.  Measured (tools/footprint_probe.py, profiles/r06/footprint_probe.txt):
 *   2^28 u32 keys 1.10 GiB in all, 2^27 u64 keys 1.58, 2^28 u64 keys 3.14; 2^28 f32 keys + u32 payloads 2.42 GiB, -> u32
 *   ranks 2.42 (round 5: 5.5 for both, whole keys and all slots in scratch memory; RSX_NO_AUX_SLOTS=1: 4.41).  Round 6, 8-byte keys by
 *   (bit length, mantissa) digits (rsx_info.hybrid == 6): the level-1
 *   buckets lie in the caller's second buffer, scratch memory holds the level-2 slots -- four bytes per key, sized
 *   (1.125 n + 46 M) x 4 bytes for any distribution (2^28 keys: 1.4 GiB, of which BASELINE's Zipf-like keys use 0.8).
 *   If an allocation fails the sort takes the histogram-first
 *   route and the (device, stream) context does not ask again until rsx_reload_env() or rsx_release_stream();
 *   RSX_NO_BLIND=1 never asks.
 *   rsx_sort_unique*: the bitmap is at most 2^RSX_UNIQUE_MAX_BITS / 8 bytes (2 MiB by default, 128 MiB at the compiled
 *   maximum of 30 bits), plus 16 bytes per 4 KiB of it and per tile of 8192 4-byte keys of a compaction.  It lives in the
 *   (device, stream) context like every other buffer here and is freed by rsx_release / rsx_release_stream.  It is never
 *   allocated inside a stream capture (the call refuses a capturing stream: it waits for the number of distinct keys).  If
 *   its allocation fails the call takes the sort route.
 *   rsx_sort_topk*: the select route keeps, in the (device, stream) context, a candidate buffer of n / 8 + 1024 (key, index)
 *   pairs, 4 x k keys and indices (the k pairs and the second buffers of their sort) and about 2 MiB of counts per
 *   workgroup; the sort route keeps what rsx_sort_rank keeps (2 n indices and the rank sort's workspace).  All of it is
 *   freed by rsx_release / rsx_release_stream and never allocated inside a stream capture (the call refuses a capturing
 *   stream).  If an allocation of the select route fails the call takes the sort route.
 *   rsx_sort_nth*: the select route keeps, in the (device, stream) context, a control block with its tables (the records of
 *   up to 64 ranks, 64 x 256 eight-byte counts, one count per workgroup: about 140 KiB), a candidate buffer of
 *   cap = n / 8 + 1024 (key, index) pairs plus the second buffers of their sort (keys only when no indices are wanted), and
 *   per rank asked for 28 bytes (the rank, n_less, n_equal, its record); rsx_sort_nth on host buffers also the staged keys and
 *   the m staged outputs; the sort route keeps what rsx_sort_rank keeps (2 n indices and the rank sort's workspace).  All of
 *   it is freed by rsx_release / rsx_release_stream and never allocated inside a stream capture (the call refuses a capturing
 *   stream).  If an allocation of the select route fails the call takes the sort route.
 *   rsx_sort_lex*: in the (device, stream) context, apart from what its inner rank and key + payload sorts keep: 3 n indices
 *   of idx_bytes (the permutation and the second buffers of its sorts) and, unless the call is one lone column, 2 n keys of
 *   the widest packed type (2, 4 or 8 bytes); rsx_sort_lex on host buffers also the staged columns and n indices.  Freed by
 *   rsx_release / rsx_release_stream, never allocated inside a stream capture (the call refuses a capturing stream); a
 *   failed allocation fails the call with RSX_ENOMEM.
 *   rsx_sort_locate*: in the (device, stream) context: a copy of the m values and the second buffer of its sort (4- and 8-byte
 *   keys, and the bins of the sort route); the search route's table -- up to 4096 edges, as many 8-byte cumulative counts, and
 *   one row of 2 x 4097 eight-byte counts per workgroup (at most 256: 16 MiB) --, the table route's two sets of counts and
 *   offsets (1.5 MiB for 2-byte keys); the sort route keeps what rsx_sort keeps for a copy of the keys (2 n keys and the sort's
 *   workspace); rsx_sort_locate on host buffers also the staged keys, values and outputs.  Freed by rsx_release /
 *   rsx_release_stream, never allocated inside a stream capture (the call refuses a capturing stream).  If an allocation of
 *   the search or table route fails the call takes the sort route.
 *   rsx_sort_partition*: in the (device, stream) context: a copy of the m edges and the second buffer of its sort; the scatter
 *   route's table -- up to 255 edges, 256 eight-byte cumulative counts and two rows of 256 eight-byte entries per workgroup (at
 *   most 256: 1 MiB); the sort route n bins, 2 n indices and 2 m counts on top of what rsx_sort_locate and rsx_sort_rank keep;
 *   rsx_sort_partition on host buffers also the staged keys, edges and outputs.  Freed by rsx_release / rsx_release_stream, never
 *   allocated inside a stream capture (the call refuses a capturing stream).  If the allocation of the scatter route's table
 *   fails the call takes the sort route.
 *   rsx_sort_segments*: in the (device, stream) context: the plan -- a record, two rows of eight 8-byte counts per workgroup (at most
 *   256), 64 KiB for the long segments and m 4-byte segment numbers; the composed route the segment number of every key (n entries
 *   of 1, 2 or 4 bytes) and n indices on top of what rsx_sort_lex keeps; the long segments' sorts work in rsx_sort_lex's buffers.
 *   rsx_sort_segments on host buffers also the staged keys, offsets and outputs.  Freed by rsx_release / rsx_release_stream, never
 *   allocated inside a stream capture (the call refuses a capturing stream).
 *   rsx_sort_join*, rsx_join_pairs*: in the (device, stream) context: the table route's counts and offsets of the right keys
 *   (768 KiB) and two sums per workgroup of its probe; what rsx_sort_pairs / rsx_sort keeps for a copy of the right keys (2 m
 *   keys, 2 m indices where right_perm is wanted); the merge route the same for the left side plus 2 n indices; n indices where
 *   count is not asked for; 8 bytes per RSX_JOIN_ROW_TILE rows for the expansion; on host buffers also the staged keys, inputs and
 *   outputs.  Freed by rsx_release / rsx_release_stream, never allocated inside a stream capture (the calls refuse a capturing
 *   stream).  If the allocation of the table fails the call takes the general route.
 *
 * Environment switches (read ONCE, at the library's first call; rsx_reload_env() reads them again)
 *   RSX_VERIFY=1            after every scatter pass one tile is re-ranked without LDS
 *                           atomics and compared with the pass's output; a mismatch fails
 *                           the call (RSX_EVERIFY) -- at once for the blocking sorts (which
 *                           then keep to one pass per kept column), at rsx_verify_poll() or
 *                           the next blocking sort for the *_inplace_async ones.
 *   RSX_VERIFY=2            every blocking device sort runs as usual (any route, see rsx_info.hybrid)
 *                           and its RESULT is checked on the device (RSX_EVERIFY if not): keys only --
 *                           sorted, the input's key sum and key mix; key + payload -- no descent, the
 *                           input's key sum and a mix of its PAIRS; ranks -- a permutation of 0 .. n-1
 *                           through which the keys do not descend, equal keys in index order.
 *   RSX_FORCE_TABLE_RANK=1  use the table-ranked scatter kernel, which does not rely
 *                           on the lane order of returning LDS atomics (slower).
 *   RSX_NO_HYBRID=1         one scatter pass per kept column always (the reference's loop);
 *   RSX_NO_BLIND=1          every sort starts with the histogram (rsx_info.hybrid never 5);
 *   RSX_NO_LEAF_PREFIX=1    leaves of 8-byte keys sort by every column they have left;
 *   RSX_NO_DENSE_SLOTS=1    the second pass of such a sort writes whole keys into its slots;
 *   RSX_NO_LEAF16=1         its leaves are round 3's (two LDS passes per slot) instead of rsx_leaf16_kernel / rsx_leafk_kernel;
 *   RSX_NO_AUX_SLOTS=1      level-1 slots all in scratch memory; RSX_NO_NARROW_SLOTS=1: 8-byte keys always in whole-key slots;
 *   RSX_NO_NARROW_LEVEL1=1  8-byte keys: the level-1 slots always hold whole keys (round 6: low words where nothing below the
 *                           level-1 digit varies above bit 32 -- keys below 2^40 --, 12 + 8 + 12 instead of 16 + 12 + 12 bytes per key);
 *   RSX_LEAF16_MAXBIN=k     (tests) the fullest bin a leaf may have before it goes to those; RSX_NO_SHIFT=1: MSB digits on bytes only;
 *   RSX_NO_LEAF16Q=1        slots of up to 256 values take a wave per leaf instead of a row of sixteen lanes;
 *   RSX_NO_LEAF16W2K=1      slots of 1025 .. 2048 values take a 128-thread workgroup per leaf instead of a wave;
 *   RSX_NO_PASS16A=1        the level-2 pass of such a sort of 4-byte keys writes ragged runs (rsx_pass16_kernel) instead of whole
 *                           64-byte atoms (rsx_pass16a_kernel); RSX_NO_PASS32A=1: the level-1 pass is the chained kernel of round 4
 *                           (rsx_scatter2_kernel) instead of rsx_pass32a_kernel; RSX_NO_PASS16=1: so is the level-2 pass;
 *                           RSX_PASS16_WGS=1, RSX_PASS16_DBG=1|2: probes of rsx_pass16_kernel (DBG gives WRONG output);
 *   RSX_PASS32_PREFETCH=1   (probe) rsx_pass32a_kernel requests the next tile's keys while it writes the current one (default: when it
 *                           starts on the tile); RSX_PASS32_MIN_MI=k: that pass from k Mi keys on (default 52 / 24 Mi 4- / 8-byte keys);
 *   RSX_NO_LEAFC=1          no two-byte slots of more than 5120 values: keys-only sorts of 4-byte keys beyond 2^28 keys run as in
 *                           round 4 (whole-key slots up to 2^30 keys, one pass per column beyond; rsx_leafc.hpp);
 *   RSX_FORCE_LEAFC=1..6    (tests) two-byte slots of any size go through the leaves of the large ones: 1 the counting leaves,
 *                           2 .. 6 rsx_leaf16_kernel's 10240- / 20480- / 6144- / 7680- / 15360-value shape + the counting leaves' list launch;
 *   RSX_NO_PACKED_KEYS=1    rank sorts without a histogram go by byte columns only: neither the keys' packed varying bits nor, for
 *                           floats on a grid, their fixed-point integers are tried (SegCtl::compact);
 *   RSX_NO_UNSTABLE=1       the MSB passes of a sort without a histogram rank per wave (stable) as every other pass does;
 *   RSX_NO_LOG=1            8-byte keys never go by (bit length, mantissa) digits (rsx_info.hybrid never 6; rsx_logroute.hpp);
 *                           RSX_LOG_MIN_LOG2=k (tests): that route from 2^k keys on (default: from 24 Mi keys; at least 2^20);
 *                           RSX_LOG_LEAF_BIG=1 (tests): its leaves in the shape for 10240 values at every size;
 *   RSX_PAIRS_LEAF_BIG=1    (tests) key + payload and rank sorts without a histogram: the leaves' shape for slots of 10240 pairs (what
 *                           2^28 .. 2^29 pairs take, round 6) at every size;
 *   RSX_NO_PASS64A=1        the level-2 pass of 8-byte keys into four-byte slots is round 4's chained kernel (rsx_pass64.hpp);
 *   RSX_NO_ODD_STRIDE=1     the level-1 slots of a sort without a histogram lie 1.25 means apart as in round 5 (default: an odd
 *                           number of 64 KiB apart); RSX_CAP1_PAD_KIB=k (probe): k KiB more per level-1 slot;
 *   RSX_PROBE=bits          (measurements; results stay right) 1: the leaf table in reverse slot order, 4: every device-scheduled
 *                           sort as if called through rsx_sort_inplace_async_hint;
 *   RSX_NO_SLACK=1, RSX_TWO_LEVEL_MIN_LOG2=k, RSX_NO_SELF_PLAN=1, RSX_NO_FUSED_HIST=1
 *                           parts of the other routes; RSX_NO_FUSED_HIST=1 (the histogram and the plan
 *                           as two launches) is exercised by tests/test_gpu_decisions.py.
 *   RSX_NO_SMALL_SORT, RSX_NO_HOST_SMALL, RSX_NO_FILL_RUNS, RSX_NO_SMALL_TILES, RSX_NO_SPECULATION,
 *   RSX_NO_NARROW_KEYS
 *                           switch single optimisations off (tests).
 *   RSX_UNIQUE_MAX_BITS=k   rsx_sort_unique*: the widest bitmap is 2^k bits (default 24, at most 30); 0: never a bitmap or a
 *                           count table -- everything but all-equal keys goes through the sort and one compaction (tests
 *                           force that route with it, tools/unique_probe.py sweeps the cut-off);
 *   RSX_GROUP_MAX_BITS=k    rsx_sort_group*: the widest bitmap under the rank cells is 2^k bits (default 24, at most 30); 0: never
 *                           a bitmap, cells or a count table -- everything but all-equal keys goes through the sort and the
 *                           heads pass (tests force that route with it, tools/group_probe.py sweeps the cut-off);
 *   RSX_RANKDATA_NO_TABLES=1  rsx_sort_rankdata*: never a column table or a count table -- everything but all-equal keys goes
 *                           through the sort and the runs pass (tests force that route with it, tools/rankdata_probe.py times it);
 *   RSX_TOPK_FORCE=1        rsx_sort_topk*: the select route whenever n >= 2 and 0 < k <= n; =2: always the sort route
 *                           (tests run both and compare; tools/topk_probe.py times both);
 *   RSX_NTH_FORCE=1         rsx_sort_nth*: the select route whenever n >= 2 and 1 <= distinct ranks <= RSX_NTH_MAX_SELECT_RANKS;
 *                           =2: always the sort route (tests run both and compare; tools/nth_probe.py times both);
 *   RSX_LOCATE_FORCE=2      rsx_sort_locate*: always the sort route (tests run both and compare; tools/locate_probe.py times both);
 *   RSX_LOCATE_MAX_VALUES=k rsx_sort_locate*: the search route while there are at most k distinct values, k in 1 .. 4096 (default
 *                           RSX_LOCATE_MAX_SEARCH_VALUES; tests lower the cut-off with it);
 *   RSX_LOCATE_COUNTER_SETS=k  (tests, probe) the search kernel keeps k sets of its LDS counters, k in 1 .. 32 (default: as many
 *                           as fit, at most 32);
 *   RSX_PARTITION_FORCE=2   rsx_sort_partition*: always the sort route (tests run both and compare; tools/partition_probe.py times both);
 *   RSX_PARTITION_MAX_EDGES=k  rsx_sort_partition*: the scatter route while there are at most k distinct edges, k in 1 .. 255
 *                           (default RSX_PARTITION_DEFAULT_MAX_EDGES = 3, the measured cut-off, DESIGN.md 4q: with more edges the sort
 *                           route won where only out_idx is asked for; a caller who wants the keys moved gains by raising it);
 *   RSX_PARTITION_BALLOT_PARTS=k  rsx_sort_partition*: tiles are ranked by one ballot per part while there are at most k parts, k in
 *                           0 .. 256 (default 7; beyond: per-wave cells in LDS; rsx_partition_info.rank_form says which ran);
 *   RSX_SEGMENTS_FORCE=1    rsx_sort_segments*: the LDS route (with long segments: MIXED) wherever it is possible at all, whatever the
 *                           measured defaults say; =2: always the composed route (tests run all and compare;
 *                           tools/segments_probe.py times them);
 *   RSX_SEGMENTS_MAX_LONG=k rsx_sort_segments*: at most k segments too long for LDS are sorted one by one (MIXED), k in 0 .. 4096
 *                           (default 8, the most with which the host loop still won); more of them: the composed route;
 *   RSX_LEX_PACK_BYTES=k    rsx_sort_lex*: neighbouring columns are packed into keys of at most k bytes, k in 1 .. 8 (default 4;
 *                           1: one sort per column; tests run 1, 4 and 8 and compare, tools/lex_probe.py times them);
 *   RSX_REDUCE_MAX_BITS=k   rsx_sort_reduce*: the cells routes while at most k bits of the derived keys vary, k in 0 .. 24 (default 12,
 *                           the LDS cut-off: beyond it the cells in device memory lost to the sort in every measured row, DESIGN.md
 *                           4o); 0: never cells -- everything goes through the sort and the runs pass;
 *   RSX_REDUCE_LDS_BITS=k   rsx_sort_reduce*: the cells lie in LDS while at most k bits vary, k in 0 .. 12 (default 12); beyond that,
 *                           up to RSX_REDUCE_MAX_BITS, in device memory;
 *   RSX_REDUCE_REPLICAS=k   (tests, probe) the cells kernel keeps k copies of its LDS cells, k in 1 .. 32 brought down to a power
 *                           of two that fits (default: as many as fit, at most 32);
 *   RSX_REDUCE_FORCE=2      rsx_sort_reduce*: always the sort route (tests run both and compare; tools/reduce_probe.py times both);
 *   RSX_JOIN_FORCE=2|3      rsx_sort_join*: 2: always the search route (the left keys as they come), 3: always the merge route (the
 *                           left side sorted too); tests run both and compare, tools/join_probe.py times both;
 *   RSX_JOIN_NO_TABLE=1     rsx_sort_join*: never the table route;
 *   RSX_COMPACT_BITS=1, RSX_HOST_REGISTER=1, RSX_ELEM_LOADS=1   opt-in variants.
 */
#ifndef RSX_H
#define RSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Key kinds = the scalar types basic_kdfs::kdf accepts
 * (radix_sort_basic_kdf.hpp:19-46; radix_experiment.cpp:264-282). */
typedef enum rsx_dtype {
	RSX_U8 = 0, RSX_U16 = 1, RSX_U32 = 2, RSX_U64 = 3,
	RSX_I8 = 4, RSX_I16 = 5, RSX_I32 = 6, RSX_I64 = 7,
	RSX_F32 = 8, RSX_F64 = 9
} rsx_dtype;

/* RSX_ASCENDING = basic_kdfs::kdf; RSX_DESCENDING = its bitwise complement,
 * the reference's descending KDF (README.md:564-574, radix_tests.cpp:111-113,
 * :175-177).  Equal keys keep input order either way. */
typedef enum rsx_order { RSX_ASCENDING = 0, RSX_DESCENDING = 1 } rsx_order;

enum {
	RSX_OK = 0,
	RSX_EINVAL = -1,     /* bad dtype / size / null pointer                */
	RSX_ENODEVICE = -2,  /* no usable gfx950 device / HIP runtime failure  */
	RSX_ENOMEM = -3,     /* device workspace allocation failed             */
	RSX_EHIP = -4,       /* a HIP call failed (see rsx_last_error)         */
	RSX_EVERIFY = -5     /* RSX_VERIFY=1: a pass disagreed with its re-computation; RSX_VERIFY=2: a result is not the sorted input */
};

/* What the front half of rs_sort_main decided (radix_sort.hpp:48-80). */
typedef struct rsx_info {
	uint32_t key_bytes;     /* wc = sizeof(KeyType), radix_sort.hpp:40          */
	uint32_t ncols;         /* kept columns, radix_sort.hpp:64-70               */
	uint32_t cols[8];       /* their indices, LSB first                          */
	uint32_t early_exit;    /* 0 none; 1 n<2 (:37-38); 2 pre-sorted (:60-62)    */
	uint32_t result_in_aux; /* 1 iff the result is the second buffer / half     */
	uint32_t hybrid;        /* how the passes were made: 0 one per kept column (:82-90); 1 / 2: one / two passes by the
	                           highest kept column(s), then the remaining columns per bucket in LDS (README.md:647-650);
	                           3: one pass by the highest kept column, then one pass per remaining column inside its
	                           buckets; 4: as 2, the second pass written into per-bucket slots of a scratch array without
	                           counting first (evenly spread keys); 5: as 4 without the histogram -- a sample of the keys
	                           has PROVED the input unsorted and which columns are kept (the two facts radix_sort.hpp:60-70
	                           takes from the histogram; columns the sample found constant are checked on every key by
	                           the first pass), both passes write into slots, the bucket sizes come off the look-back
	                           chains (large arrays; blocking keys-only, rank and key + payload sorts);
	                           6: 8-byte keys whose magnitudes spread where their bytes do not (Zipf-like keys): the keys
	                           below 2^14 are counted and written out, the others go by (bit length, leading mantissa bits)
	                           into buckets of exactly counted sizes, by the next eight bits into slots, and through leaves
	                           (rsx_logroute.hpp; the pre-sorted exit and the kept columns come from that route's own
	                           one-read histogram kernel, exactly).  The
	                           result and the returned buffer are the same whichever it is. */
} rsx_info;

/* ---- environment ---------------------------------------------------------- */

int         rsx_device_count(void);   /* gfx950 devices visible; 0 if none / no runtime */
const char *rsx_last_error(void);     /* message of the calling thread's last failure   */
const char *rsx_version(void);
size_t      rsx_dtype_size(rsx_dtype dtype);
/* Bytes of device workspace a sort of n keys of this shape will hold on to. */
size_t      rsx_workspace_bytes(size_t n, rsx_dtype dtype, size_t payload_bytes);
/* Release every cached workspace / stream context of the calling process.  No other thread may be inside the library
 * while this runs (the contexts are freed without waiting for their locks). */
void        rsx_release(void);
/* One context is kept per (device, stream) the library has been called with; a
 * program that creates many short-lived streams releases them one by one: frees the
 * workspace of (current device, stream) after synchronising the stream.  No other thread may be inside the library
 * on that (device, stream) while this runs, or start a call on it before it returns. */
void        rsx_release_stream(void *stream);

/* The RSX_* switches of the environment (diagnostics and A/B switches; every one is named where it acts, in
 * DESIGN.md) are read once, at the library's first call.  A process that changes them afterwards -- tests do -- calls
 * this to have them read again; RSX_FORCE_TABLE_RANK is only honoured before the first sort on a device.
 * NOT thread-safe against running sorts: the switches live in one process-wide record that every entry point reads
 * without a lock, so no other thread may be inside the library while this runs (as for rsx_release_stream). */
void        rsx_reload_env(void);

/* ---- radix_sort<T>(src, aux, n) -- radix_sort.hpp:98-115 ------------------ */

/* src/aux may be host pointers (staged over PCIe) or device pointers on the
 * current device (sorted in place in HBM); both must be of the same kind.
 * *result receives src or aux.  Blocking. */
int rsx_sort(void *src, void *aux, size_t n, rsx_dtype dtype, rsx_order order,
             void **result, rsx_info *info);

/* The same sort without any host synchronisation: every pass is scheduled on the
 * device (each finds its column, its buffers and "nothing to do" in the plan the
 * histogram kernels left in device memory), and the result always ends in d_buf --
 * when the number of kept columns is odd (radix_sort.hpp:89,:92 would return aux) a
 * last kernel copies it back.  d_scratch is the auxiliary buffer (n elements; its
 * contents afterwards are unspecified, untouched if the input was sorted).  Nothing
 * is returned but the status of the enqueue: the call can be captured into a HIP
 * graph (after one uncaptured call of the same size has sized the workspace) and
 * replayed on new contents of d_buf.
 * Round 4: the ROUTE is chosen on the device as well (rsx_async_route reports it): one MSB pass and leaves for mid-size
 * arrays; for large arrays (4-byte keys from 9 Mi keys, 8-byte keys from 8 Mi keys through this entry point; the blocking
 * rsx_sort_device starts at 7.5 Mi / 4.5 Mi) the sort without a histogram is
 * enqueued first and the histogram-first kernels behind it do nothing if it went through.  That attempt works in d_scratch
 * (once its sample has proven the input unsorted) and in slots in the (device, stream) workspace: 0.25 n + 0.625 n .. 1.25 n
 * keys of device memory (see "Scratch memory" above); rsx_sort_inplace_async_ws, whose state lies in the caller's
 * workspace, makes it when the workspace was sized by rsx_workspace_bytes_fast (below).  rsx_sort_pairs_inplace_async and rsx_sort_rank_inplace_async (4-byte keys with 4-byte
 * payloads / indices, 16 Mi .. 2^29 pairs) make the same attempt; rsx_async_route reports the last call's route for them too. */
int rsx_sort_inplace_async(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order,
                           void *stream);
/* ... with what the caller knows about the keys.  RSX_HINT_EVEN_TOP_DIGITS: the caller has COUNTED the keys by their most
 * significant varying byte and found the counts even (no digit with twice its share) -- what the local sorts of a distributed
 * sort know from the split's gathered histogram.  Keys that an MSD split has put in order of that byte, piece by
 * piece, look clustered at each of the 64 places the sample of a sort without a histogram reads, and the sample would call the
 * attempt off: with the hint the level-1 digit's evenness is the caller's word, everything else is checked as always (the
 * level-2 digit in the sample; every slot's capacity by the passes themselves, so a wrong hint costs a lost attempt, never a
 * wrong result).  2^29 keys as rank 0 of 2 would receive them: 4.46 -> 3.44 ms (tools/presplit_probe.py). */
enum { RSX_HINT_EVEN_TOP_DIGITS = 1 };
int rsx_sort_inplace_async_hint(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order,
                                void *stream, uint32_t hints);

/* LIFETIME of what a captured graph refers to.  The two *_inplace_async entry points
 * above and below keep their device state (flags, plan, histograms, status words of
 * the look-back) in the library's workspace of (current device, stream), which is
 * cached, GROWN -- freed and reallocated -- by a later larger sort on the same
 * (device, stream), and freed by rsx_release / rsx_release_stream.  A graph
 * captured from them is valid only until one of these happens, and its replays
 * must be ordered (stream order) against every other sort that uses the same
 * (device, stream) workspace.  A caller that keeps a graph should use the *_ws forms:
 * there all device state lies in d_workspace (256-byte aligned, at least
 * rsx_workspace_bytes(n, dtype, payload_bytes) bytes, owned by the caller for as
 * long as the graph lives; contents are scratch), so nothing the graph touches can
 * move, and graphs with different workspaces may replay on any streams. */
int rsx_sort_inplace_async_ws(void *d_buf, void *d_scratch, size_t n, rsx_dtype dtype, rsx_order order,
                              void *d_workspace, size_t workspace_bytes, void *stream);
/* Round 5: a workspace of rsx_workspace_bytes_fast(n, dtype) bytes (0.25 n + 0.63 n .. 1.25 n keys more than the minimum:
 * the slots of a sort without a histogram) lets rsx_sort_inplace_async_ws make that attempt INSIDE the workspace, so a graph
 * that is kept runs on the route of DESIGN.md 4c like every other sort (4- and 8-byte keys, 4 Mi .. 2^30 keys).  A smaller
 * workspace (at least rsx_workspace_bytes) works as before: histogram first.  rsx_async_route_ws reads the route the last sort
 * (or replay) in that workspace took (it waits for `stream`): 5, 1 or 0 as rsx_async_route. */
size_t rsx_workspace_bytes_fast(size_t n, rsx_dtype dtype);
int rsx_async_route_ws(const void *d_workspace, size_t workspace_bytes, size_t n, rsx_dtype dtype, void *stream, uint32_t *route);
int rsx_sort_pairs_inplace_async_ws(void *d_keys, void *d_keys_scratch, void *d_vals, void *d_vals_scratch,
                                    size_t n, rsx_dtype dtype, size_t payload_bytes, rsx_order order,
                                    void *d_workspace, size_t workspace_bytes, void *stream);

/* Key + payload in the same manner: both arrays sorted in place by the keys (stable),
 * never a host synchronisation, HIP-graph capturable.  payload_bytes: 4 or 8. */
int rsx_sort_pairs_inplace_async(void *d_keys, void *d_keys_scratch, void *d_vals, void *d_vals_scratch,
                                 size_t n, rsx_dtype dtype, size_t payload_bytes, rsx_order order,
                                 void *stream);

/* radix_sort_rank (radix_sort_rank.hpp:97-112) in the same manner: the stable argsort of d_src (untouched) without a
 * host synchronisation, HIP-graph capturable.  The ranks ALWAYS end in the first half of d_index_buffer (2n entries of
 * idx_bytes = 4 or 8 bytes): the number of passes is only known on the device, where the passes take their buffers from
 * the plan so that the last one writes the first half; sorted keys give 0 .. n-1 there (:52,:55-57).  The keys' work
 * copies live in the (device, stream) workspace: call it once outside a capture so that the workspace has its size.  Keys
 * travel at full width here (the blocking rsx_sort_rank_device hands on only the bytes still to be sorted by). */
int rsx_sort_rank_inplace_async(const void *d_src, void *d_index_buffer, size_t n, rsx_dtype dtype,
                                size_t idx_bytes, rsx_order order, void *stream);

/* RSX_VERIFY=1 also checks one tile of every pass of the *_inplace_async sorts (re-ranked with ballots on the device, as
 * for the blocking sorts), but those never wait: their mismatches add up on the device.  This waits for `stream`, reports
 * the count (RSX_EVERIFY if it is not zero) and resets it; the next blocking sort on the stream does the same. */
int rsx_verify_poll(void *stream, uint64_t *mismatches);

/* The route the LAST rsx_sort_inplace_async on (current device, stream) took -- the device decides it and the call never
 * waits, so it can only be asked for afterwards: this waits for `stream` and reads the device's words back.  *route as
 * rsx_info.hybrid: 5 = no histogram, two MSB passes into slots and leaves; 1 = one MSB pass and leaves; 0 = histogram and one
 * pass per kept column (also: sorted input, and the one-launch sort of small arrays).  The loop all of them stand for is
 * radix_sort.hpp:82-90.  Replaying a captured graph of such a sort re-decides the route on the device each time; what this
 * reports is the last replay's.  The plan it reads is the device-scheduled sorts' own; the control block of an attempt
 * without a histogram is the context's: a BLOCKING sort of 2^22 keys or more on the same stream between the device-scheduled
 * sort and this call may overwrite it (ask before that sort, or use another stream for it). */
int rsx_async_route(void *stream, uint32_t *route);

/* rs_sort_main / rs_sort_rank with a caller-supplied Hist (radix_sort.hpp:28-33,
 * radix_sort_rank.hpp:22-23): arms the CALLING THREAD's next blocking sort call
 * (rsx_sort, rsx_sort_device, rsx_sort_rank*, rsx_sort_pairs_device,
 * rsx_sort_records*) to also write the counts of loop 1 (radix_sort.hpp:48-58):
 * hist[256 * j + d] = number of keys whose KDF byte j is d, j < key bytes;
 * `entries` = room in hist (>= 256 * key bytes, or the sort fails with
 * RSX_EINVAL).  One shot: the sort disarms it; hist == NULL disarms by hand.
 * Sorts of n < 2 keys and the *_async entry points never write.  From the counts
 * and rsx_info the template wrapper reproduces what the reference leaves in the
 * caller's storage (include/radix_sort.hpp, hist_post_state). */
int rsx_capture_histogram(uint64_t *hist, size_t entries);

/* Device-resident variant for callers that own a HIP stream (`stream` is a
 * hipStream_t, NULL = the default stream).  The column plan has to reach the
 * host to apply the returned-pointer rule, so the call synchronises `stream`
 * once after the histogram pass; the scatter passes are enqueued and NOT
 * waited for: the result is valid for work ordered after them on `stream`. */
int rsx_sort_device(void *d_src, void *d_aux, size_t n, rsx_dtype dtype, rsx_order order,
                    void *stream, void **result, rsx_info *info);

/* ---- sorted distinct keys ("Uniquely sorting with bitmaps", README.md, bitmap_sort_16.c) ------------------ */

/* The distinct keys of the input in order of kdf(key), and optionally how many of each.
 *   - Result: *result is d_src or d_aux; its first *n_unique elements are the distinct BIT PATTERNS of the input,
 *     ascending by kdf(key) (RSX_DESCENDING: by the complemented KDF).  The KDF is a bijection on bit patterns, so
 *     "distinct" is by bit pattern -- the "bit-exact copies" rule above: -0.0 and +0.0 are two keys, NaNs with different
 *     payloads are different keys.
 *   - Buffers: d_src is consumed, as by rsx_sort_device; everything past *n_unique in both buffers is unspecified.
 *   - n < 2 returns d_src with *n_unique = n and leaves d_aux untouched; no device is needed for that, except to write
 *     the one count of n == 1 into device memory (rsx_sort_unique writes it into host memory itself).
 *   - Counts: d_counts may be NULL; otherwise it has room for n entries of count_bytes = 4 or 8 (with 4, n must fit, or
 *     the call fails with RSX_EINVAL "does not fit", as for idx_bytes), and counts[j] = the number of input elements
 *     equal to result[j].
 *   - Blocking: the call returns once *n_unique is on the host; the arrays are valid for work ordered after it on `stream`.
 *   - Errors: no GPU: RSX_ENODEVICE; bad dtype, order or count_bytes: RSX_EINVAL.  A failed allocation of the bitmap is
 *     not an error: the call takes the sort route.
 * The route is chosen from what the call can observe of the keys (rsx_unique_info.route): where few bits of
 * the derived keys vary, one bit per possible value replaces the sort; where one byte column varies (all 1-byte keys), or
 * counts of 2-byte keys are wanted, the answer is read off a count table; everything else is rsx_sort_device -- any of its
 * routes, every early exit -- and one compaction of the sorted buffer into the other one. */
enum { RSX_UNIQUE_TRIVIAL = 0,        /* n < 2, or every key equal                                   */
       RSX_UNIQUE_BITMAP_LDS = 1,     /* per-workgroup bitmaps in LDS, merged into one in HBM        */
       RSX_UNIQUE_BITMAP_GLOBAL = 2,  /* one bitmap in device memory                                 */
       RSX_UNIQUE_TABLE = 3,          /* answer read off a count table that already exists           */
       RSX_UNIQUE_SORT = 4 };         /* the ordinary sort (any route), then one compaction          */
typedef struct rsx_unique_info {
	rsx_info sort;          /* front half: key_bytes, kept columns, early_exit; hybrid as the sort reports it on RSX_UNIQUE_SORT */
	uint32_t route;         /* RSX_UNIQUE_*                                                          */
	uint32_t varying_bits;  /* popcount of the KDF bits that differ among the keys; 0 = not computed */
	uint64_t table_bytes;   /* bitmap / count table used, 0 otherwise                                */
} rsx_unique_info;

int rsx_sort_unique_device(void *d_src, void *d_aux, size_t n, rsx_dtype dtype, rsx_order order,
                           void *d_counts, size_t count_bytes, void *stream,
                           void **result, size_t *n_unique, rsx_unique_info *info);
/* host or device pointers, as rsx_sort (all of the same kind); the distinct keys of host buffers come back into src or aux */
int rsx_sort_unique(void *src, void *aux, size_t n, rsx_dtype dtype, rsx_order order,
                    void *counts, size_t count_bytes,
                    void **result, size_t *n_unique, rsx_unique_info *info);

/* ---- dense group ids of the keys: the inverse of rsx_sort_unique (a rank directory over its bitmap) -------- */

/* For every key the index of its group among the distinct keys in order, and optionally the groups themselves.
 * Let U[0 .. G) be what rsx_sort_unique returns for the same keys, dtype and order: the distinct BIT PATTERNS, ascending by
 * kdf(key) (RSX_DESCENDING: by the complemented KDF) -- -0.0 and +0.0 are two groups, NaNs with different payloads too.
 *   - *n_groups = G; out_inverse[i], i < n, is the j with U[j] bit-equal to src[i]; out_keys[j] = U[j], out_counts[j] = the
 *     number of elements of group j, out_first[j] = the smallest i with out_inverse[i] == j, for j < G.
 *   - Buffers: d_src is never written.  Every output may be NULL, each on its own; n_groups is required.  Each output has
 *     room for n elements and nothing outside [0, n) of any of them is touched; entries of keys, counts and first at or
 *     past G are unspecified.  idx_bytes is 4 or 8 and applies to inverse, counts and first; with 4, n must fit, or the call
 *     fails with RSX_EINVAL "does not fit".
 *   - Errors: bad dtype, order or idx_bytes, NULL n_groups, n && !src: RSX_EINVAL.  n == 0: RSX_OK, *n_groups = 0, nothing
 *     written, no device needed.  n == 1: rsx_sort_group on host pointers needs no device (it writes 0, src[0], 1, 0),
 *     rsx_sort_group_device only for the stores.  Otherwise, without a GPU: RSX_ENODEVICE, nothing written.  A capturing
 *     stream: RSX_EINVAL (the call waits for the number of groups).  A failed allocation of the bitmap or the cells is not
 *     an error: the call takes the sort route.
 *   - Blocking: the call returns once *n_groups is on the host; the device outputs are valid for work ordered after it on
 *     `stream`.
 * The route is chosen from what the call can observe of the keys (rsx_group_info.route).  Where at most
 * RSX_GROUP_MAX_BITS bits of the derived keys vary and neither counts nor first are wanted, rsx_sort_unique's bitmap is
 * made, one 8-byte cell per word of it holds the word and the number of set bits below it, and every key looks its group
 * up with one load and one popcount: two streaming passes over the keys and no sort.  Where one byte column varies (all
 * 1-byte keys) the cells come from the plan's 256 counts, which are the groups' counts as well.  Everything else -- first
 * indices always -- is a stable key + index sort of a workspace copy (rsx_sort_pairs_device's routes; none where the input
 * is sorted already) and one pass over its result that numbers the head flags and scatters through the permutation.
 * Memory, in the (device, stream) context: the bitmap and its cells (at most 12 bytes per 32 packed values: 6 MiB at the
 * default cut-off), or a copy of the keys, its second buffer and 2 n indices; freed by rsx_release / rsx_release_stream. */
enum { RSX_GROUP_TRIVIAL = 0,      /* n < 2, or every key equal                                          */
       RSX_GROUP_RANK_LDS = 1,     /* bitmap + rank cells, the lookup reads the cells from LDS           */
       RSX_GROUP_RANK_GLOBAL = 2,  /* the same, cells read from device memory (L2)                       */
       RSX_GROUP_TABLE = 3,        /* one kept column: cells made from the plan's 256 counts, no mark pass */
       RSX_GROUP_SORT = 4 };       /* stable key + index sort (any route), heads, scan, scatter          */
typedef struct rsx_group_info {
	rsx_info sort;          /* as rsx_unique_info.sort */
	uint32_t route;         /* RSX_GROUP_* */
	uint32_t varying_bits;  /* popcount of the KDF bits that differ among the keys; 0 = not computed */
	uint64_t table_bytes;   /* bitmap + cells used, 0 otherwise */
} rsx_group_info;

int rsx_sort_group_device(const void *d_src, size_t n, rsx_dtype dtype, rsx_order order,
                          void *d_out_inverse, void *d_out_keys, void *d_out_counts, void *d_out_first,
                          size_t idx_bytes, void *stream, size_t *n_groups, rsx_group_info *info);
/* host or device pointers, as rsx_sort (all of the same kind) */
int rsx_sort_group(const void *src, size_t n, rsx_dtype dtype, rsx_order order,
                   void *out_inverse, void *out_keys, void *out_counts, void *out_first,
                   size_t idx_bytes, size_t *n_groups, rsx_group_info *info);

/* ---- every element's place in the sorted order: the inverse of rsx_sort_rank (a counting sort's prefix sums, read per key) -- */

/* For every element where it stands in the stable sorted order, and how many elements are smaller than / equal to it.
 * Let R[0 .. n) be what rsx_sort_rank returns for the same keys, dtype and order: a stable argsort by kdf(key)
 * (RSX_DESCENDING: by the complemented KDF).  All three outputs are 0-based; for every i < n:
 *   - out_place[i] is the j with R[j] == i (the inverse permutation): the number of elements with a smaller derived key plus
 *     the number of bit-equal elements at a lower index;
 *   - out_less[i] is the number of elements whose derived key is below element i's, out_equal[i] the number whose derived key
 *     equals it, itself included (rsx_sort_nth's n_less / n_equal): less[i] <= place[i] < less[i] + equal[i].
 *   The tie methods of a ranking follow: ordinal = place, min = less, max = less + equal - 1, average = less + (equal - 1) / 2;
 *   dense is rsx_sort_group's inverse.  Keys are bit patterns: -0.0 and +0.0 are different keys, NaNs with different payloads too.
 *   - Buffers: d_src is never written.  Each output may be NULL, but not all three.  Each output has room for exactly n entries
 *     of idx_bytes (4 or 8) and nothing outside [0, n) of any of them is touched; with 4, n must fit, or the call fails with
 *     RSX_EINVAL "does not fit".
 *   - Errors: bad dtype, order or idx_bytes, all outputs NULL, n && !src: RSX_EINVAL.  n == 0: RSX_OK, nothing written, no
 *     device needed.  n == 1: it writes (0, 0, 1); rsx_sort_rankdata on host pointers needs no device for it,
 *     rsx_sort_rankdata_device only for the stores.  Otherwise, without a GPU: RSX_ENODEVICE, nothing written.  A capturing
 *     stream: RSX_EINVAL (the call waits for the plan of the keys).  A failed allocation of a table is not an error: the call
 *     takes the sort route.
 *   - Blocking: the call waits for what it has to read of the keys to choose the route (as rsx_sort_group_device); the device
 *     outputs are valid for work ordered after it on `stream`.
 * The route is chosen from what the call can observe of the keys (rsx_rankdata_info.route).  Where one byte
 * column varies (all 1-byte keys) its 256 exclusive offsets, which the plan's histogram holds already, are less and equal of
 * every key, and the place is the address a stable counting sort's scatter would compute, kept instead of used: three
 * ordinary launches (counts per workgroup, their scan, the walk) and no sort.  Where the place is not wanted and at most 16 bits
 * vary in keys of 2 bytes or more, the counts of the packed varying bits are made in LDS (rsx_sort's 16-bit digit), scanned and
 * looked up.  Everything else is a stable key + index sort of a workspace copy (rsx_sort_pairs_device's routes; none where
 * the input is sorted already), then the permutation inverted, or the heads pass and one pass over the runs.
 * Memory, in the (device, stream) context: a table of at most 2 MiB, or a copy of the keys, its second buffer and 2 n indices;
 * freed by rsx_release / rsx_release_stream. */
enum { RSX_RANKDATA_TRIVIAL = 0,   /* n < 2, or every key equal                                          */
       RSX_RANKDATA_TABLE = 1,     /* one kept column: lookups in its 256 offsets, the place by counting */
       RSX_RANKDATA_COUNT16 = 2,   /* at most 16 varying bits, no place: count table in LDS, scan, lookup */
       RSX_RANKDATA_SORT = 3 };    /* stable key + index sort (any route), inverse scatter or runs pass  */
typedef struct rsx_rankdata_info {
	rsx_info sort;          /* as rsx_unique_info.sort */
	uint32_t route;         /* RSX_RANKDATA_* */
	uint32_t varying_bits;  /* popcount of the KDF bits that differ among the keys; 0 = not computed */
	uint64_t table_bytes;   /* offsets, bases or counts used, 0 otherwise */
} rsx_rankdata_info;

int rsx_sort_rankdata_device(const void *d_src, size_t n, rsx_dtype dtype, rsx_order order,
                             void *d_out_place, void *d_out_less, void *d_out_equal,
                             size_t idx_bytes, void *stream, rsx_rankdata_info *info);
/* host or device pointers, as rsx_sort (all of the same kind) */
int rsx_sort_rankdata(const void *src, size_t n, rsx_dtype dtype, rsx_order order,
                      void *out_place, void *out_less, void *out_equal,
                      size_t idx_bytes, rsx_rankdata_info *info);

/* ---- the first k of the sorted order ("Hybrids", README.md:647-650: one MSB pass, then only the sub-result that matters) -- */

/* The first k entries of the stable sorted order, without sorting the rest.
 *   - Result: out_idx[j], j < k, is the j-th entry of what rsx_sort_rank returns for the same keys, dtype and order: a
 *     stable argsort, so equal keys come in ascending index order -- also among the keys equal to the k-th one, of which
 *     the lowest indices are kept.  out_keys[j] is the bit-exact image of src[out_idx[j]] (NaN payloads, -0.0).
 *     RSX_DESCENDING orders by the complemented KDF; ties still come in ascending index order.
 *   - Buffers: d_src is never written.  Each output has room for exactly k elements and nothing past element k - 1 is
 *     touched.  Either output may be NULL, not both.  idx_bytes is 4 or 8; with 4, n must fit, or the call fails with
 *     RSX_EINVAL "does not fit".
 *   - Errors: k > n: RSX_EINVAL "k exceeds n"; bad dtype, order, idx_bytes, both outputs NULL: RSX_EINVAL; k == 0: RSX_OK,
 *     nothing written, no device needed; k > 0 without a GPU: RSX_ENODEVICE, nothing written; a capturing stream:
 *     RSX_EINVAL (the call waits for what the selection found).
 *   - Blocking: as rsx_sort_device -- the call may synchronise `stream`; the outputs are valid for work ordered after it
 *     on `stream`; *info is complete on return.
 * RSX_TOPK_SELECT: a histogram of the keys' most significant byte tells which bucket holds rank k; one more
 * pass over the input moves that bucket into a candidate buffer, the remaining bytes are found there, and the k surviving
 * (key, index) pairs go through the ordinary stable key + payload sort.  A bucket too large for the candidate buffer is
 * narrowed by further histograms over the input instead: input_reads <= key_bytes + 1 always, 2 for keys that spread over
 * their top byte.  RSX_TOPK_SORT is rsx_sort_rank_device on a workspace copy, the first k ranks kept (small n, large k). */
enum { RSX_TOPK_TRIVIAL = 0,   /* k == 0, or n < 2                                              */
       RSX_TOPK_SELECT  = 1,   /* MSD radix select, then a sort of k candidates                 */
       RSX_TOPK_SORT    = 2 }; /* the ordinary stable rank sort, first k kept                   */
typedef struct rsx_topk_info {
	uint32_t route;        /* RSX_TOPK_*                                                         */
	uint32_t key_bytes;
	uint32_t input_reads;  /* SELECT: kernels that read all n keys of d_src; otherwise 0         */
	uint32_t digit_passes; /* SELECT: histogram passes made, over the input or the candidates    */
	uint64_t n_less;       /* elements with kdf(key) <  kdf(k-th key)  (always < k)              */
	uint64_t n_equal;      /* elements with kdf(key) == kdf(k-th key)  (n_less + n_equal >= k)   */
	uint64_t kth_key;      /* bit pattern of the k-th element, zero-extended                     */
} rsx_topk_info;

int rsx_sort_topk_device(const void *d_src, size_t n, size_t k, rsx_dtype dtype, rsx_order order,
                         void *d_out_keys, void *d_out_idx, size_t idx_bytes,
                         void *stream, rsx_topk_info *info);
/* host or device pointers, as rsx_sort (all of the same kind) */
int rsx_sort_topk(const void *src, size_t n, size_t k, rsx_dtype dtype, rsx_order order,
                  void *out_keys, void *out_idx, size_t idx_bytes, rsx_topk_info *info);

/* ---- the elements at given ranks of the sorted order (what a counting sort's prefix sums answer: medians, quantiles, the
 *      splitters of a balanced MSD split) -------------------------------------------------------------------------------- */

/* The entries at m given positions of the stable sorted order, without sorting the rest.
 *   - Result: let R be what rsx_sort_rank returns for the same keys, dtype and order -- a stable argsort: equal keys in
 *     ascending index order, RSX_DESCENDING orders by the complemented KDF.  For every j < m: out_idx[j] = R[ranks[j]] and
 *     out_keys[j] is the bit-exact image of src[out_idx[j]] (NaN payloads, -0.0); n_less[j] is the number of elements whose
 *     derived key is below that key's, n_equal[j] the number whose derived key equals it, so
 *     n_less[j] <= ranks[j] < n_less[j] + n_equal[j].
 *   - ranks, n_less and n_equal are HOST memory in both forms (as `cols` is for rsx_sort_lex).  Ranks are 0-based, in any
 *     order, and may repeat; the outputs are in the caller's order of ranks.  n_less and n_equal may be NULL, each on its own.
 *   - Buffers: d_src is never written.  Each device output has room for exactly m elements and nothing past element m - 1 is
 *     touched.  Either of out_keys / out_idx may be NULL, not both.  idx_bytes is 4 or 8; with 4, n must fit, or the call
 *     fails with RSX_EINVAL "does not fit".
 *   - Errors: a rank >= n: RSX_EINVAL "rank exceeds n", nothing written; bad dtype, order or idx_bytes, both outputs NULL,
 *     ranks == NULL with m > 0: RSX_EINVAL.  m == 0: RSX_OK, nothing written, no device needed.  n == 1: rsx_sort_nth on host
 *     pointers needs no device, rsx_sort_nth_device only for the stores.  Otherwise, without a GPU: RSX_ENODEVICE, nothing
 *     written.  A capturing stream: RSX_EINVAL (the call waits for what the selection found).  A failed allocation of the
 *     select route's buffers is not an error: the call takes the sort route.
 *   - Blocking: as rsx_sort_topk_device -- the call may synchronise `stream`; the device outputs are valid for work ordered
 *     after it on `stream`; *info and the two host arrays are complete on return.
 * RSX_NTH_SELECT: the distinct ranks, sorted, are carried TOGETHER through histograms of the derived keys'
 * bytes, most significant first: a level counts, for every active bucket (a distinct prefix that still holds a wanted rank; at
 * most 64), the next byte of the elements in it, and every rank moves on to the digit that holds it.  As soon as the active
 * buckets together hold at most cap = n / 8 + 1024 elements, those are moved to a candidate buffer in index order (a count and
 * a write over the input), sorted by the ordinary stable key + payload sort, and every answer is read at its place.  Keys that
 * occur more than about n / 8 times never fit: after the last byte the prefixes ARE the keys and n_less / n_equal are known,
 * so a call that wants no indices is answered from them (from_prefix = 1), and one that does takes the sort route.
 * input_reads <= key_bytes + 2 always; 3 for a few ranks of keys that spread over their top byte.  RSX_NTH_SORT is
 * rsx_sort_rank_device on a workspace copy, the m entries read through the ranks (small n, more than
 * RSX_NTH_MAX_SELECT_RANKS distinct ranks). */
enum { RSX_NTH_TRIVIAL = 0,   /* m == 0, or n < 2                                          */
       RSX_NTH_SELECT  = 1,   /* multi-rank MSD radix select, then a sort of the candidates */
       RSX_NTH_SORT    = 2 }; /* the ordinary stable rank sort, m entries read              */
enum { RSX_NTH_MAX_SELECT_RANKS = 64 };   /* more DISTINCT ranks than this: the sort route  */

typedef struct rsx_nth_info {
	uint32_t route;          /* RSX_NTH_*                                                   */
	uint32_t key_bytes;
	uint32_t input_reads;    /* SELECT: kernels that read all n keys of d_src; otherwise 0  */
	uint32_t digit_passes;   /* SELECT: histogram levels made (1 .. key_bytes)              */
	uint32_t active_buckets; /* SELECT: distinct buckets that held a wanted rank at the last level */
	uint32_t from_prefix;    /* SELECT: 1 = answered from the digits alone, no candidates moved     */
	uint64_t candidates;     /* SELECT: (key, index) pairs moved and sorted; otherwise 0    */
} rsx_nth_info;

int rsx_sort_nth_device(const void *d_src, size_t n, const uint64_t *ranks, size_t m,
                        rsx_dtype dtype, rsx_order order,
                        void *d_out_keys, void *d_out_idx, size_t idx_bytes,
                        uint64_t *n_less, uint64_t *n_equal,
                        void *stream, rsx_nth_info *info);
/* host or device pointers for src / out_keys / out_idx, as rsx_sort (all of the same kind) */
int rsx_sort_nth(const void *src, size_t n, const uint64_t *ranks, size_t m,
                 rsx_dtype dtype, rsx_order order, void *out_keys, void *out_idx, size_t idx_bytes,
                 uint64_t *n_less, uint64_t *n_equal, rsx_nth_info *info);

/* ---- where given values fall in the sorted order (the opposite of rsx_sort_nth: searchsorted, bucketize, digitize, the bins of
 *      a histogram with given edges, the parts of a split by given splitters) -------------------------------------------------- */

/* For m values that need not occur among the n keys: how many keys lie below each and how many equal it, and for every key how
 * many of the values lie at or below it -- without sorting the keys where the values are few.
 *   - Result: let K(x) be the derived key of x under dtype and order (the KDF, complemented for RSX_DESCENDING: what the sorts
 *     order by).  For every j < m: less[j] = #{ i : K(src[i]) < K(vals[j]) } -- searchsorted(sorted src, vals[j], 'left') --
 *     and equal[j] = #{ i : K(src[i]) == K(vals[j]) }; less + equal is searchsorted's 'right'.  For every i < n:
 *     bin[i] = #{ j : K(vals[j]) <= K(src[i]) } -- np.digitize(src, sorted vals), torch.bucketize(src, sorted vals, right=True);
 *     with RSX_LOCATE_BINS_BELOW in flags, bin[i] = #{ j : K(vals[j]) < K(src[i]) } -- bucketize with right=False.  Values are
 *     compared as bit patterns through the KDF: NaN payloads and -0.0 / +0.0 are distinct, as everywhere in this library.  The
 *     values may come in any order and may repeat.
 *   - Buffers: d_src and d_vals (both device memory, of the same dtype) are never written.  less and equal have room for exactly
 *     m entries, bin for exactly n, of idx_bytes (4 or 8) each, and nothing past them is touched.  Any of the three may be NULL,
 *     not all.  With idx_bytes == 4, n must fit where less or equal is wanted and m must fit where bin is, or the call fails with
 *     RSX_EINVAL "does not fit".
 *   - Trivial cases: m == 0 and no bins wanted: RSX_OK, nothing written, no device needed.  m == 0 with bins: zeros.  n == 0:
 *     zeros in less and equal.
 *   - Errors: bad dtype, order, idx_bytes or flags, all outputs NULL, src == NULL with n > 0, vals == NULL with m > 0: RSX_EINVAL.
 *     Without a GPU: RSX_ENODEVICE, nothing written.  A capturing stream: RSX_EINVAL (the call waits for the number of distinct
 *     values).  A failed allocation of the search or table route's buffers is not an error: the call takes the sort route.
 *   - Blocking: as rsx_sort_nth_device -- the call may synchronise `stream`; the outputs are valid for work ordered after it on
 *     `stream`; *info is complete on return.
 * Routes (rsx_locate_info.route).  RSX_LOCATE_TABLE, keys of 1 or 2 bytes: the counts of the derived keys and of
 * the values over the at most 2^16 derived keys, scanned; every answer is a table read.  RSX_LOCATE_SEARCH, keys of 4 or 8 bytes
 * and at most RSX_LOCATE_MAX_SEARCH_VALUES DISTINCT values: the values are sorted and reduced to their distinct edges, a start
 * table over the first 8 bits in which the edges differ, and the number of values at or below each edge; ONE kernel reads the
 * keys, finds for each the number of edges at or below it (a start-table lookup and search_steps halvings in LDS), counts it in
 * LDS and writes its bin; the counts of all workgroups, summed and scanned, are less and equal of every value.
 * RSX_LOCATE_SORT, everything else and RSX_LOCATE_FORCE=2: a workspace copy of the keys through rsx_sort_device (none where
 * the keys are in order already: sort.early_exit == 2) and two binary searches per value; for the bins the values sorted and
 * one binary search per key. */
enum { RSX_LOCATE_TRIVIAL = 0,   /* n == 0 or m == 0                                              */
       RSX_LOCATE_TABLE   = 1,   /* 1- and 2-byte keys: count tables, scans, lookups               */
       RSX_LOCATE_SEARCH  = 2,   /* one read of the keys against the distinct values held in LDS   */
       RSX_LOCATE_SORT    = 3 }; /* sorts and binary searches                                      */
enum { RSX_LOCATE_MAX_SEARCH_VALUES = 4096 };    /* more DISTINCT values than this: the sort route */
enum { RSX_LOCATE_BINS_BELOW = 1 };              /* flags: bin[i] counts the values strictly below */

typedef struct rsx_locate_info {
	uint32_t route;            /* RSX_LOCATE_*                                                            */
	uint32_t key_bytes;
	uint32_t input_reads;      /* TABLE, SEARCH: kernels that read all n keys of d_src; otherwise 0        */
	uint32_t distinct_values;  /* SEARCH: D, the distinct derived keys among vals; SORT: where the count stopped (0: not counted) */
	uint32_t search_steps;     /* SEARCH: halvings per key behind the start table (0 .. 12)               */
	uint32_t counter_sets;     /* SEARCH: replicas of the LDS counters per workgroup                      */
	rsx_info sort;             /* SORT: what the inner sort of the keys reported                          */
} rsx_locate_info;

int rsx_sort_locate_device(const void *d_src, size_t n, const void *d_vals, size_t m,
                           rsx_dtype dtype, rsx_order order,
                           void *d_less, void *d_equal, void *d_bin, size_t idx_bytes, uint32_t flags,
                           void *stream, rsx_locate_info *info);
/* host or device pointers for src / vals / less / equal / bin, as rsx_sort_nth (all of the same kind) */
int rsx_sort_locate(const void *src, size_t n, const void *vals, size_t m,
                    rsx_dtype dtype, rsx_order order,
                    void *less, void *equal, void *bin, size_t idx_bytes, uint32_t flags,
                    rsx_locate_info *info);

/* ---- the split itself: the keys moved into the parts that given splitters cut them into (std::stable_partition for one
 *      splitter, np.partition / np.argpartition with several kth, pd.cut followed by ordering by bin, the distribution step of a
 *      sample sort, range partitioning of a table, dispatch of rows to a few destinations) ------------------------------------ */

/* For m edges that need not occur among the n keys: the keys listed part by part, inside a part in their input order.
 *   - Result: let K(x) be the derived key of x under dtype and order, as everywhere.  The bin of key i is rsx_sort_locate's
 *     bin[i] = #{ j : K(edges[j]) <= K(src[i]) }; with RSX_PARTITION_BELOW in flags, #{ j : K(edges[j]) < K(src[i]) }.  There are
 *     m + 1 parts, part p holds the keys with bin p; the result lists the parts in ascending p and inside a part the keys in
 *     ascending input position (stable).  out_keys[0 .. n): the keys in that order, as raw bit patterns, unchanged.
 *     out_idx[0 .. n): for every output position the input row it came from -- np.argsort(bin, kind="stable").
 *     offsets[0 .. m + 2): offsets[j] = #{ i : bin[i] < j }: offsets[0] = 0, offsets[m + 1] = n, part p is
 *     [offsets[p], offsets[p + 1]).  With sv the sorted edges, offsets[1 .. m] is searchsorted(sorted keys, sv, 'left')
 *     ('right' with RSX_PARTITION_BELOW).  The edges may come in any order and may repeat: repeated edges give empty parts.
 *   - Buffers: d_src and d_edges (device memory, of the same dtype) are never written.  out_keys has room for exactly n keys,
 *     out_idx for n and offsets for m + 2 entries of idx_bytes (4 or 8) each, and nothing past them is touched.  out_keys or
 *     out_idx may be NULL, not both; offsets may be NULL.  With idx_bytes == 4, n (and m) must fit, or the call fails with
 *     RSX_EINVAL "does not fit".  out_keys must not overlap src; out_keys == src is RSX_EINVAL.
 *   - Trivial cases: n == 0: offsets all zero, nothing else written.  m == 0: one part -- the keys copied, out_idx = 0 .. n-1,
 *     offsets = {0, n}.
 *   - Errors: bad dtype, order, idx_bytes or flags, both of out_keys and out_idx NULL, src == NULL with n > 0, edges == NULL with
 *     m > 0: RSX_EINVAL.  Without a GPU: RSX_ENODEVICE, nothing written.  A capturing stream: RSX_EINVAL (the call waits for the
 *     number of distinct edges).  A failed allocation of the scatter route's table is not an error: the call takes the sort route.
 *   - Blocking: as rsx_sort_locate_device -- the call may synchronise `stream`; the outputs are valid for work ordered after it
 *     on `stream`; *info is complete on return.
 * Routes (rsx_partition_info.route).  The route depends on the number of distinct edges, the switches and whether
 * the table could be allocated -- never on n.  RSX_PARTITION_SCATTER, every dtype and at most k DISTINCT edges -- k = RSX_PARTITION_DEFAULT_MAX_EDGES
 * unless the switch RSX_PARTITION_MAX_EDGES raises it, to at most RSX_PARTITION_MAX_EDGES (256 parts): the edges are sorted and reduced as rsx_sort_locate's search route reduces its values; a workgroup
 * owns a contiguous share of the keys in memory order; one kernel counts every share's keys per part, one workgroup scans the
 * counts part-major (the start of every part of every share, and the caller's offsets), and one kernel goes through every share
 * again tile by tile: it searches each key's part once, ranks the tile stably by part inside each wave (rank_form 1: one ballot
 * per part; 2: per-wave cells in LDS, the lanes of a part found by one ballot per bit of the part number), stages the tile in LDS
 * in output order and writes it run by run behind per-part cursors in LDS.  Two reads of the keys; no kernel waits for another
 * workgroup and none adds to device memory atomically.  RSX_PARTITION_SORT, everything else and RSX_PARTITION_FORCE=2:
 * rsx_sort_locate_device's bins into workspace, their stable rank sort (rsx_sort_rank_device's machinery: its histogram skips the
 * constant bytes of the bins), a gather of the keys, and the offsets from locate's less / equal over the sorted edges. */
enum { RSX_PARTITION_TRIVIAL = 0,   /* n == 0 or m == 0                                                    */
       RSX_PARTITION_SCATTER = 1,   /* count, scan, stable placement by a searched part: two reads of the keys */
       RSX_PARTITION_SORT    = 2 }; /* locate's bins, their rank sort, a gather                              */
enum { RSX_PARTITION_BELOW = 1 };        /* flags: a key's part counts the edges strictly below it         */
enum { RSX_PARTITION_MAX_EDGES = 255 };  /* more DISTINCT edges than this: the sort route, whatever the switch says */
enum { RSX_PARTITION_DEFAULT_MAX_EDGES = 3 };  /* ... and by default more than this (RSX_PARTITION_MAX_EDGES=k raises it) */

typedef struct rsx_partition_info {
	uint32_t route;            /* RSX_PARTITION_*                                                          */
	uint32_t key_bytes;
	uint32_t input_reads;      /* SCATTER: 2 (kernels that read all n keys of d_src); otherwise 0           */
	uint32_t distinct_edges;   /* SCATTER: D, the distinct derived keys among edges; SORT: where the count stopped (0: not counted) */
	uint32_t search_steps;     /* SCATTER: halvings per key behind the start table (0 .. 8)                 */
	uint32_t rank_form;        /* SCATTER: 1 ballots, 2 per-wave cells in LDS; otherwise 0                  */
	uint32_t shares;           /* SCATTER: workgroups of the count and of the placement                     */
	rsx_locate_info locate;    /* SORT: what the inner rsx_sort_locate_device reported                      */
	rsx_info sort;             /* SORT: what the inner rank sort of the bins reported                       */
} rsx_partition_info;

int rsx_sort_partition_device(const void *d_src, size_t n, const void *d_edges, size_t m,
                              rsx_dtype dtype, rsx_order order,
                              void *d_out_keys, void *d_out_idx, void *d_offsets, size_t idx_bytes, uint32_t flags,
                              void *stream, rsx_partition_info *info);
/* host or device pointers for src / edges / out_keys / out_idx / offsets, as rsx_sort_locate (all of the same kind); n == 0 on
 * host pointers needs no device */
int rsx_sort_partition(const void *src, size_t n, const void *edges, size_t m,
                       rsx_dtype dtype, rsx_order order,
                       void *out_keys, void *out_idx, void *offsets, size_t idx_bytes, uint32_t flags,
                       rsx_partition_info *info);

/* ---- ordering by several key columns (the stability argument one level up: README.md, "this is only possible because
 *      the sort is stable") ------------------------------------------------------------------------------------------ */

/* The stable argsort of n rows by the tuple (kdf_0(col_0[i]), kdf_1(col_1[i]), ...).
 *   - Result: out_idx[0 .. n-1] lists the rows in order of that tuple.  Column 0 is the MOST significant one, as in SQL's
 *     ORDER BY col_0, col_1, ... -- the REVERSE of np.lexsort's argument order, whose last key is the primary one.  Each
 *     column has its own dtype and its own order; RSX_DESCENDING complements that column's KDF.  Rows whose derived keys are
 *     equal in every column come in ascending index order.  With ncols == 1 the result is element for element what
 *     rsx_sort_rank_device returns for that column.
 *   - Buffers: no column is ever written.  out_idx has room for exactly n entries of idx_bytes (4 or 8) and nothing past
 *     entry n - 1 is touched; the ping-pong buffers are the library's (see "Scratch memory"), not the caller's.  With
 *     idx_bytes == 4, n must fit, or the call fails with RSX_EINVAL "does not fit".  The `cols` array itself is host memory
 *     in both forms.  The same column pointer may appear more than once.  A column needs only its element's alignment.
 *   - Errors: ncols == 0 or ncols > RSX_LEX_MAX_COLS, a NULL column, a bad dtype or order, a bad idx_bytes: RSX_EINVAL.
 *     n == 0: RSX_OK, no device needed.  n == 1 writes out_idx[0] = 0 (rsx_sort_lex on host pointers needs no device for
 *     it, rsx_sort_lex_device only for that store).  Otherwise, without a GPU: RSX_ENODEVICE, nothing written.  A capturing
 *     stream: RSX_EINVAL (the call waits between its sorts).  A failed allocation of the library's buffers: RSX_ENOMEM --
 *     there is no cheaper route to fall back to.
 *   - Blocking: as rsx_sort_device -- the call may synchronise `stream`; the output is valid for work ordered after it on
 *     `stream`; *info is complete on return.
 * How: neighbouring columns are GROUPED -- walking from the last column towards column 0, a column joins
 * the current group while the group's bytes plus its own are at most the packing limit P (RSX_LEX_PACK_BYTES, default 4);
 * a column wider than P is a group of its own.  One kernel (rsx_lex.hpp) derives and packs a group's keys into one unsigned
 * key per row, the group's first column in the highest bits; group[0] -- the LEAST significant columns -- is rank-sorted
 * (a lone column directly in the caller's memory, with its own dtype and order), every later group's keys are gathered
 * through the permutation found so far and sorted stably with that permutation as their payload. */
enum { RSX_LEX_MAX_COLS = 16 };
typedef struct rsx_lex_col { const void *data; uint32_t dtype; uint32_t order; } rsx_lex_col;   /* rsx_dtype, rsx_order */

typedef struct rsx_lex_group {
	uint32_t first_col, ncols;   /* the columns first_col .. first_col + ncols - 1 of the call                  */
	uint32_t key_bytes;          /* sum of their widths, 1 .. 8                                                */
	uint32_t sorted_as;          /* rsx_dtype handed to the inner sort (the column's own for a lone column of group 0) */
	uint32_t kept_cols, hybrid;  /* rsx_info.ncols / .hybrid of that sort                                      */
	uint32_t in_order;           /* 1: that sort took its pre-sorted exit (the permutation did not change)     */
	uint32_t pad;
} rsx_lex_group;
typedef struct rsx_lex_info {
	uint32_t ncols, ngroups;     /* ngroups = sorts made; 0 when n < 2                                          */
	uint32_t pack_bytes;         /* the packing limit in force (above)                                         */
	uint32_t early_exit;         /* 0; 1: n < 2; 2: every group was in order, the result is 0 .. n-1           */
	rsx_lex_group group[RSX_LEX_MAX_COLS];   /* group[0] is sorted FIRST = the least significant columns       */
} rsx_lex_info;

int rsx_sort_lex_device(const rsx_lex_col *cols, size_t ncols, size_t n, void *d_out_idx, size_t idx_bytes,
                        void *stream, rsx_lex_info *info);
/* host or device pointers, as rsx_sort (all of the same kind); host columns are staged, each distinct one once */
int rsx_sort_lex(const rsx_lex_col *cols, size_t ncols, size_t n, void *out_idx, size_t idx_bytes, rsx_lex_info *info);

/* ---- many independent arrays sorted in one call (torch.sort(x, dim=-1) on a [batch, length] tensor, argsort per row, the column
 *      indices of every row of a CSR matrix, neighbour and candidate lists; rocprim::segmented_radix_sort) ---------------------- */

/* The n keys of src are cut into m segments, CSR style, and every segment is sorted on its own.
 *   - Segments: d_offsets holds m + 1 entries of idx_bytes (4 or 8); segment s is [offsets[s], offsets[s + 1]).  The offsets must
 *     not decrease, offsets[0] must be 0 and offsets[m] must be n: anything else is RSX_EINVAL "bad offsets" with no output
 *     written -- the check runs on the device before anything is written.  d_offsets == NULL means m equal rows of n / m keys;
 *     then n % m != 0 is RSX_EINVAL.  Empty segments are allowed.
 *   - Result: let K(x) be the derived key of x under dtype and order, as everywhere.  Inside every segment, independently, the keys
 *     come out in ascending K, equal K in ascending input position (stable).  out_keys[0 .. n): the raw bit patterns in that
 *     order; segment s occupies the range it has in the input.  out_idx[0 .. n): the input position each output element came
 *     from -- the position in the whole array (src[out_idx[j]] == out_keys[j] bit for bit), or with RSX_SEGMENTS_LOCAL_IDX in
 *     flags the position relative to the segment's start, as torch.sort(dim=-1).indices.  For one segment out_idx is
 *     rsx_sort_rank_device's result element for element.
 *   - Buffers: d_src and d_offsets are never written.  out_keys and out_idx have room for exactly n elements (out_idx of idx_bytes
 *     each) and nothing past them is touched.  Either may be NULL, not both.  out_keys == src or any overlap of the two is
 *     RSX_EINVAL.  With idx_bytes == 4, n must fit, or the call fails with RSX_EINVAL "does not fit"; m must fit 32 bits always.
 *   - Trivial cases: n == 0 or m == 0: RSX_OK, route RSX_SEGMENTS_TRIVIAL, nothing written; the host form needs no device.
 *   - Errors: bad dtype, order, idx_bytes or flags, both outputs NULL, src == NULL with n > 0: RSX_EINVAL.  Without a GPU:
 *     RSX_ENODEVICE, nothing written.  A capturing stream: RSX_EINVAL (the call waits for its plan).
 *   - Blocking: as rsx_sort_partition_device -- the call may synchronise `stream`; the outputs are valid for work ordered after it
 *     on `stream`; *info is complete on return.
 * Routes (rsx_segments_info.route).  A plan kernel reads the offsets, checks them and lists the segment numbers by
 * size class (rsx_segments_info.class_count; radix_sorting_amd/csrc/rsx_segments_shape.hpp): 0 lengths 0 and 1, copied; 1 up to
 * 256 keys, a wave per segment; 2 up to 2048 keys, a workgroup of 256 threads; 3 up to `cap` keys -- what fits the 160 KiB of a
 * CU's LDS for this key width and these outputs --, a workgroup of 1024 threads; 4 longer than cap.  RSX_SEGMENTS_LDS: no segment is
 * longer than cap; one launch per class that has segments, in which a team of waves loads a whole segment into LDS, finds which
 * byte columns vary IN THAT SEGMENT and whether it is in order already, runs one stable LDS-to-LDS pass per varying column and
 * writes the result: one read and one write of the keys.  RSX_SEGMENTS_MIXED: 1 .. RSX_SEGMENTS_MAX_LONG segments are longer than
 * cap: those go one by one through the plain sorts on their sub-ranges, the others as before.  RSX_SEGMENTS_LEX: everything
 * else and RSX_SEGMENTS_FORCE=2: the segment number of every key in the narrowest of u8 / u16 / u32, rsx_sort_lex_device on
 * (segment, key) and a gather.  Which of the first two is taken BY DEFAULT is a measured choice per size class:
 * today where every segment is of class 0 or 3 (at most one key, or 2049 .. cap keys) and at most 8 are longer than cap; a call with
 * a segment of 2 .. 2048 keys takes RSX_SEGMENTS_LEX.  RSX_SEGMENTS_FORCE=1 takes them wherever they are possible at all. */
enum { RSX_SEGMENTS_TRIVIAL = 0,   /* n == 0 or m == 0                                                         */
       RSX_SEGMENTS_LDS     = 1,   /* every segment sorted in LDS by a wave or a workgroup                      */
       RSX_SEGMENTS_MIXED   = 2,   /* ... and the few too long for LDS by the plain sorts, one by one           */
       RSX_SEGMENTS_LEX     = 3 }; /* rsx_sort_lex_device on (segment number, key), a gather                    */
enum { RSX_SEGMENTS_LOCAL_IDX = 1 };   /* flags: out_idx counts from the segment's start                        */
enum { RSX_SEGMENTS_CLASSES = 5 };

typedef struct rsx_segments_info {
	uint32_t route;            /* RSX_SEGMENTS_*                                                           */
	uint32_t key_bytes;
	uint32_t cap;              /* the longest segment the LDS route takes for this dtype and these outputs  */
	uint32_t pad;
	uint64_t max_len;          /* the longest segment of the call                                          */
	uint64_t n_long;           /* segments longer than cap                                                 */
	uint64_t class_count[RSX_SEGMENTS_CLASSES];   /* segments per size class (above); [4] == n_long        */
	rsx_lex_info lex;          /* LEX: what the inner rsx_sort_lex_device reported                          */
	rsx_info sort;             /* MIXED: what the last per-segment sort reported                            */
} rsx_segments_info;

int rsx_sort_segments_device(const void *d_src, size_t n, const void *d_offsets, size_t m, size_t idx_bytes,
                             rsx_dtype dtype, rsx_order order,
                             void *d_out_keys, void *d_out_idx, uint32_t flags,
                             void *stream, rsx_segments_info *info);
/* host or device pointers for src / offsets / out_keys / out_idx, as rsx_sort_partition (all of the same kind) */
int rsx_sort_segments(const void *src, size_t n, const void *offsets, size_t m, size_t idx_bytes,
                      rsx_dtype dtype, rsx_order order,
                      void *out_keys, void *out_idx, uint32_t flags,
                      rsx_segments_info *info);

/* ---- per-group count, sum, min and max of a second column (reduce_by_key over rsx_sort_unique's groups) -------------- */

/* For every group of equal keys -- the groups of rsx_sort_group, in rsx_sort_unique's order -- how many elements it has and the
 * sum, the smallest and the largest of the values that stand beside its keys.
 * Let U[0 .. G) be what rsx_sort_unique returns for the same keys, dtype and order (distinct BIT PATTERNS, ascending by kdf(key);
 * RSX_DESCENDING: by the complemented KDF).  *n_groups = G, and for j < G:
 *   - out_keys[j] = U[j]; out_counts[j] = the size of group j, idx_bytes (4 or 8) wide; with 4, n must fit, or the call fails
 *     with RSX_EINVAL "does not fit".
 *   - out_sum[j], always 8 bytes wide: integer values (RSX_U32, RSX_I32, RSX_U64, RSX_I64) are zero- or sign-extended to 64 bits
 *     and added modulo 2^64 -- a u64 / i64 bit pattern, exact whatever the order of the additions.  RSX_F32 / RSX_F64 values are
 *     converted to f64 (exact) and added with IEEE double additions, starting from +0.0, in an order the call does not specify
 *     (on the sort route it is the same from run to run); infinities and NaNs propagate as the additions make them.
 *   - out_min[j] / out_max[j], in val_dtype: the value of the group whose kdf(value) under val_dtype and RSX_ASCENDING is
 *     smallest / largest, whatever `order` says about the keys.  That is numeric order for integers; for floats it is the float
 *     KDF's total order on BIT PATTERNS: -0.0 < +0.0, NaNs with the sign bit clear above +inf, NaNs with it set below -inf.
 *     This is the library's "keys are bit patterns" rule, NOT numpy's NaN propagation: a NaN does not poison min or max.
 *   - val_dtype is one of the six 4- and 8-byte dtypes; a narrower one: RSX_EINVAL.
 *   - ops: bits of RSX_REDUCE_SUM | RSX_REDUCE_MIN | RSX_REDUCE_MAX.  Every output may be NULL, each on its own, but sum, min
 *     and max must agree with their bit: a bit whose output is NULL, or an output whose bit is clear: RSX_EINVAL.  ops == 0 with
 *     only keys or counts wanted is legal.  n_groups is required, and with n > 0 so are d_keys and d_vals.
 *   - Buffers: d_keys and d_vals are never written.  Each output has room for n entries and nothing outside [0, n) of any of
 *     them is touched; entries at or past G are unspecified.
 *   - Errors: bad dtype, order, val_dtype, ops or idx_bytes, NULL n_groups: RSX_EINVAL.  n == 0: RSX_OK, *n_groups = 0, nothing
 *     written, no device needed.  n == 1: rsx_sort_reduce on host pointers needs no device, rsx_sort_reduce_device only for the
 *     copies.  Otherwise, without a GPU: RSX_ENODEVICE, nothing written.  A capturing stream: RSX_EINVAL (the call waits for the
 *     number of groups).  A failed allocation of the table of cells is not an error: the call takes the sort route.
 *   - Blocking: as rsx_sort_group_device.
 * The route is chosen from what the call can observe of the keys (rsx_reduce_info.route).  Where at most
 * RSX_REDUCE_LDS_BITS (12) bits of the derived keys vary -- category codes, one byte column, all 1-byte keys -- the packed
 * varying bits number a cell per possible key, every workgroup accumulates its share of keys and values into copies of the
 * cells in its LDS, merges them into one table, and the table is read out in order: one streaming read, nothing sorted, no
 * inverse.  Up to RSX_REDUCE_MAX_BITS the same with the cells in device memory -- off by default (RSX_REDUCE_MAX_BITS = 12): it
 * lost to the sort route wherever it was measured.  Everything else is a stable key + value sort
 * of workspace copies (rsx_sort_pairs_device's routes; none where the input is sorted already) and a segmented reduction over
 * the runs of its result.  Memory, in the (device, stream) context: the table (at most 32 bytes per cell), or copies of keys
 * and values with their second buffers and 80 bytes per tile of the sorted array; freed by rsx_release / rsx_release_stream. */
enum { RSX_REDUCE_SUM = 1, RSX_REDUCE_MIN = 2, RSX_REDUCE_MAX = 4 };          /* bits of `ops` */
enum { RSX_REDUCE_TRIVIAL = 0,       /* n < 2, or every key equal                                             */
       RSX_REDUCE_CELLS_LDS = 1,     /* one read of keys + values into per-packed-value accumulators in LDS   */
       RSX_REDUCE_CELLS_GLOBAL = 2,  /* the same body, the accumulators in device memory                      */
       RSX_REDUCE_SORT = 3 };        /* stable key + value sort (any route), heads, one pass over the runs    */
typedef struct rsx_reduce_info {
	rsx_info sort;          /* as rsx_unique_info.sort */
	uint32_t route;         /* RSX_REDUCE_* */
	uint32_t varying_bits;  /* popcount of the KDF bits that differ among the keys; 0 = not computed */
	uint64_t table_bytes;   /* the table of cells used, 0 otherwise */
} rsx_reduce_info;

int rsx_sort_reduce_device(const void *d_keys, const void *d_vals, size_t n, rsx_dtype dtype, rsx_order order,
                           rsx_dtype val_dtype, unsigned ops,
                           void *d_out_keys, void *d_out_counts, size_t idx_bytes,
                           void *d_out_sum, void *d_out_min, void *d_out_max,
                           void *stream, size_t *n_groups, rsx_reduce_info *info);
/* host or device pointers, as rsx_sort (all of the same kind); host keys and values are staged side by side */
int rsx_sort_reduce(const void *keys, const void *vals, size_t n, rsx_dtype dtype, rsx_order order,
                    rsx_dtype val_dtype, unsigned ops,
                    void *out_keys, void *out_counts, size_t idx_bytes,
                    void *out_sum, void *out_min, void *out_max,
                    size_t *n_groups, rsx_reduce_info *info);

/* ---- matching rows of two key columns: the equi-join (pandas.merge, SQL JOIN ... ON a.k = b.k, np.intersect1d with indices,
 *      isin, the symbolic phase of a sparse product, gathering a dimension table's rows into a fact table) ------------------------ */

/* Two calls.  Phase 1, rsx_sort_join*, writes the join in compressed form -- one range into the sorted right side per left row --
 * and says how many pairs there are; phase 2, rsx_join_pairs*, expands such ranges into the two lists of row numbers.
 * Let K(x) be the derived key of x under dtype and order (the KDF, complemented for RSX_DESCENDING), compared as a BIT PATTERN as
 * everywhere in this library: -0.0 and +0.0 differ, a NaN equals itself exactly when its bits do.  left has n rows, right has m,
 * both of `dtype`; P is the stable argsort of right under K (what rsx_sort_rank returns for it).
 * Phase 1:
 *   - right_perm[0 .. m) = P.  For every i < n: count[i] = #{ j : K(right[j]) == K(left[i]) }, and WHERE count[i] > 0,
 *     start[i] = #{ j : K(right[j]) < K(left[i]) }: the matches of row i are P[start[i] .. start[i] + count[i]), in ascending j.
 *     Where count[i] == 0, start[i] is written but its value is unspecified (the table route cannot order a key that differs
 *     from every right key in a bit that does not vary among them, and no use of the join needs the value).
 *   - *n_pairs = the sum of count[i]; with RSX_JOIN_LEFT in flags the sum of max(count[i], 1).  It is a uint64_t whatever
 *     idx_bytes is: the pairs of 2^17 rows against 2^16 may number 2^33.
 *   - Buffers: d_left and d_right are never written.  start and count have room for exactly n entries, right_perm for exactly m,
 *     of idx_bytes (4 or 8) each, and nothing past them is touched.  Each of the three may be NULL, and all three may be (only
 *     the number of pairs is wanted).  With idx_bytes == 4, n and m must fit, or the call fails with RSX_EINVAL "does not fit".
 *   - Trivial cases: n == 0 or m == 0: route RSX_JOIN_TRIVIAL, count is zeros (start too), right_perm an iota, *n_pairs = 0 (n under
 *     RSX_JOIN_LEFT); no device is needed where that leaves nothing to write, and rsx_sort_join on host pointers never needs one
 *     for it.
 *   - Errors: bad dtype, order, idx_bytes or flags, NULL n_pairs, left == NULL with n > 0, right == NULL with m > 0: RSX_EINVAL.
 *     Without a GPU: RSX_ENODEVICE, nothing written.  A capturing stream: RSX_EINVAL (the call waits for the number of pairs).
 *     A failed allocation of the table is not an error: the call takes the general route.
 *   - Blocking: as rsx_sort_locate_device -- the call may synchronise `stream`; the outputs are valid for work ordered after it
 *     on `stream`; *n_pairs and *info are complete on return.
 * Routes of phase 1 (rsx_join_info.route), chosen from what the call can observe of the RIGHT keys; the left keys are
 * never inspected beforehand.  RSX_JOIN_TABLE, direct addressing: at most 16 bits of the right keys vary, in at most eight runs,
 * and m < 2^32 (all 1-byte keys qualify): the right keys' packed varying bits are counted and scanned, and ONE kernel streams
 * the left keys, tests each against the right keys' non-varying bits and reads two neighbouring offsets of the table; the right
 * side is sorted only where right_perm is wanted.  RSX_JOIN_SEARCH: the right side is sorted (key + iota, or keys alone where
 * right_perm is not wanted; nothing is copied or sorted where the keys are in order already: sort.early_exit == 2 and right_perm
 * an iota) and the left keys are searched in it as they come.  RSX_JOIN_MERGE: the same, but the left side is sorted too (key +
 * iota), the search runs over the SORTED left keys so that neighbouring lanes search neighbouring places, and start / count go
 * back through the left permutation (left_sorted = 1).  RSX_JOIN_FORCE=2 / =3 forces SEARCH / MERGE, RSX_JOIN_NO_TABLE=1 closes
 * TABLE.
 * Phase 2, rsx_join_pairs*, reads only arrays as phase 1 wrote them -- no keys, no sort, no state kept between the calls:
 *   - The pairs are ordered by i ascending, then by j ascending: for the t-th match of row i at pair position p,
 *     out_left[p] = i and out_right[p] = right_perm[start[i] + t].  With RSX_JOIN_LEFT a row without a match yields ONE pair
 *     (i, all ones): -1 in either index width, what pandas.merge(how="left")'s indexer returns.  Pair positions are 64-bit
 *     throughout.
 *   - *n_pairs is always set.  Where it exceeds `capacity` (the entries each output has room for) the call returns RSX_EINVAL
 *     "does not fit" and writes nothing.  Nothing at or past *n_pairs is touched.
 *   - Either output may be NULL, not both.  count is required where n > 0, start and right_perm where out_right is wanted.
 *     A position start[i] + t at or past m -- which arrays of phase 1 never name -- reads nothing and yields all ones.
 *   - Errors: bad idx_bytes or flags, both outputs NULL, a missing input, NULL n_pairs: RSX_EINVAL.  n == 0: RSX_OK, no pairs, no
 *     device needed; rsx_join_pairs on host pointers counts the pairs on the host and needs no device where there are none or
 *     they do not fit.  Otherwise, without a GPU: RSX_ENODEVICE, no output written.  A capturing stream: RSX_EINVAL.
 *   - Blocking, as phase 1.
 * The expansion costs by its OUTPUT, never by how the pairs are spread over the rows: the rows' pairs are summed by
 * tiles of RSX_JOIN_ROW_TILE rows and scanned; one workgroup per RSX_JOIN_EXPAND_TILE consecutive pairs finds its first row tile
 * by binary search, scans that tile's counts in LDS, and every thread finds the row of its pair positions by a search of that
 * scan.  No atomics, no look-back chain, no spin-wait. */
enum { RSX_JOIN_TRIVIAL = 0,   /* n == 0 or m == 0                                                   */
       RSX_JOIN_TABLE   = 1,   /* direct addressing into the count table of the right keys' varying bits */
       RSX_JOIN_SEARCH  = 2,   /* the right side sorted, the left keys searched as they come         */
       RSX_JOIN_MERGE   = 3 }; /* both sides sorted, the sorted left keys searched                   */
enum { RSX_JOIN_LEFT = 1 };    /* flags: a left row without a match yields one pair (i, all ones)    */
enum { RSX_JOIN_ROW_TILE = 1024, RSX_JOIN_EXPAND_TILE = 4096 };   /* the expansion's tiles: rows, pairs */

typedef struct rsx_join_info {
	uint32_t route;            /* RSX_JOIN_*                                                            */
	uint32_t key_bytes;
	uint32_t varying_bits;     /* of the right keys' derived keys (0: not computed)                     */
	uint32_t left_sorted;      /* 1: the left side was sorted too (MERGE)                               */
	uint64_t table_bytes;      /* TABLE: the offsets a probe reads (512 KiB; 1 KiB for 1-byte keys)     */
	rsx_info sort;             /* what the inner sort of the right side reported                        */
} rsx_join_info;

int rsx_sort_join_device(const void *d_left, size_t n, const void *d_right, size_t m,
                         rsx_dtype dtype, rsx_order order,
                         void *d_start, void *d_count, void *d_right_perm, size_t idx_bytes, uint32_t flags,
                         void *stream, uint64_t *n_pairs, rsx_join_info *info);
/* host or device pointers for left / right / start / count / right_perm, as rsx_sort_locate (all of the same kind) */
int rsx_sort_join(const void *left, size_t n, const void *right, size_t m,
                  rsx_dtype dtype, rsx_order order,
                  void *start, void *count, void *right_perm, size_t idx_bytes, uint32_t flags,
                  uint64_t *n_pairs, rsx_join_info *info);

int rsx_join_pairs_device(const void *d_start, const void *d_count, const void *d_right_perm, size_t n, size_t m,
                          size_t idx_bytes, uint32_t flags, void *d_out_left, void *d_out_right, uint64_t capacity,
                          void *stream, uint64_t *n_pairs);
/* host or device pointers for all five arrays (all of the same kind) */
int rsx_join_pairs(const void *start, const void *count, const void *right_perm, size_t n, size_t m,
                   size_t idx_bytes, uint32_t flags, void *out_left, void *out_right, uint64_t capacity,
                   uint64_t *n_pairs);

/* ---- key + payload (struct-of-arrays) ------------------------------------- */

/* Stable sort of (key[i], payload[i]) pairs by kdf(key): the device form of the
 * reference's radix_sort on {key, payload} records (radix_tests.cpp:41-56 shape,
 * SURVEY.md 8d cfg 4).  payload_bytes is 4 or 8.  Keys and payloads ping-pong
 * together; info->result_in_aux tells which pair of buffers holds the result. */
int rsx_sort_pairs_device(void *d_keys, void *d_keys_aux, void *d_vals, void *d_vals_aux,
                          size_t n, rsx_dtype dtype, size_t payload_bytes, rsx_order order,
                          void *stream, rsx_info *info);

/* ---- radix_sort_rank<T,IdxType>(src, index_buffer, n) --------------------- */

/* radix_sort_rank.hpp:97-112 with the pass semantics of Listing 6
 * (radix_sort_u32_ranks.c:85-107), i.e. a correct stable argsort: see
 * SURVEY.md section 4 for the header's defect.  index_buffer holds 2n indices of
 * idx_bytes (1, 2, 4 or 8; n must fit).  *result receives index_buffer (kept
 * columns even, n<2, pre-sorted) or index_buffer + n (odd).  Pre-sorted input
 * writes 0..n-1 to the first half and leaves the second untouched
 * (radix_sort_rank.hpp:52,:55-57); n == 1 writes index_buffer[0] = 0 (:28-32).
 * Host or device pointers (both of the same kind).  Blocking. */
int rsx_sort_rank(const void *src, void *index_buffer, size_t n, rsx_dtype dtype,
                  size_t idx_bytes, rsx_order order, void **result, rsx_info *info);

/* Device-resident variant; idx_bytes is 4 or 8. */
int rsx_sort_rank_device(const void *d_src, void *d_index_buffer, size_t n, rsx_dtype dtype,
                         size_t idx_bytes, rsx_order order, void *stream, void **result,
                         rsx_info *info);

/* ---- records with a host-evaluated key (opaque KeyFunc) -------------------- */

/* radix_sort(src, aux, n, kf) for trivially copyable T and an arbitrary host
 * KeyFunc (radix_tests.cpp:41-43,:111-113; README.md:562-591): the template
 * wrapper evaluates kf once per element into `keys` (n unsigned keys of
 * key_bytes = sizeof(KeyType) in {1,2,4,8}, already KDF-applied); the device
 * rank-sorts the keys and gathers the rec_bytes-sized records.  Host pointers.
 * *result receives src or aux by the returned-pointer rule. */
int rsx_sort_records(void *src, void *aux, size_t n, size_t rec_bytes,
                     const void *keys, size_t key_bytes, void **result, rsx_info *info);

/* ---- records with a declared key (tagged KeyFunc) ----------------------------- */

/* radix_sort(src, aux, n, kf) where kf is "the scalar field at byte key_offset
 * of the element, default KDF of its type, ascending or complemented": the shapes
 * of radix_tests.cpp:41-43,:45-69,:111-113 and README.md:562-591 written as data
 * instead of code (include/radix_sort.hpp: rsx_kdf::by_member<&T::field>).
 * Key extraction, stable rank sort and the gather of the rec_bytes-sized records
 * all run on the device.  *result receives src or aux by the returned-pointer rule
 * (radix_sort.hpp:89,:92); pre-sorted input returns src with aux untouched. */
int rsx_sort_records_tagged(void *src, void *aux, size_t n, size_t rec_bytes, size_t key_offset,
                            rsx_dtype key_dtype, rsx_order order, void **result, rsx_info *info);

/* Device-pointer form: records resident in HBM, work enqueued on `stream`
 * (one synchronisation inside, as rsx_sort_device). */
int rsx_sort_records_tagged_device(void *d_src, void *d_aux, size_t n, size_t rec_bytes,
                                   size_t key_offset, rsx_dtype key_dtype, rsx_order order,
                                   void *stream, void **result, rsx_info *info);

/* Same derivation for radix_sort_rank with an opaque KeyFunc. */
int rsx_sort_rank_keys(const void *keys, size_t key_bytes, void *index_buffer, size_t n,
                       size_t idx_bytes, void **result, rsx_info *info);

/* ---- building blocks exported for the multi-GPU path and the tests --------- */

/* Upfront histogram of every 8-bit KDF column (radix_sort.hpp:48-58):
 * d_hist receives 256 * key_bytes uint64 counts (device memory), *d_unsorted a
 * non-zero uint32 iff some kdf(key[i]) > kdf(key[i+1]).  Enqueued on stream. */
int rsx_histogram_device(const void *d_src, size_t n, rsx_dtype dtype, rsx_order order,
                         uint64_t *d_hist, uint32_t *d_unsorted, void *stream);

/* The MSD split as one ordinary stable scatter pass by the top KDF byte itself
 * (256 digits; README.md:647-650): d_dst = d_src ordered by that
 * byte, top_hist (host, 256 uint64) = its counts.  Destinations that are
 * contiguous ranges of the byte are contiguous ranges of d_dst:
 * digit d occupies [sum(top_hist[0..d)), +top_hist[d]).  The counts are ready on
 * return; the pass is enqueued on stream.  column < 0: the top byte; otherwise
 * the byte to split by (a caller that knows the bytes above it to be constant). */
int rsx_msd_split_device(const void *d_src, void *d_dst, size_t n, rsx_dtype dtype,
                         rsx_order order, int column, uint64_t *top_hist, void *stream);

/* The same pass for a caller that already has the shard's column counts -- d_hist: the 256 * key_bytes uint64 counts
 * rsx_histogram_device left in device memory (one read of the shard gives every column's, so the column to split by can be
 * chosen from them without a trial pass).  Counts nothing, waits for nothing: everything is only enqueued on `stream`.
 * column | RSX_SPLIT_HOT: the caller, who has the counts, says that one digit of the column holds an eighth of the shard's
 * keys or more -- the pass then ranks its dominant digits by ballots (what rsx_msd_split_device decides from its own counts). */
#define RSX_SPLIT_HOT 0x100
int rsx_msd_split_async(const void *d_src, void *d_dst, size_t n, rsx_dtype dtype, rsx_order order,
                        int column, const uint64_t *d_hist, void *stream);

/* radix_sort(src, aux, n, kdf) on HOST buffers with the work spread over `ndev`
 * devices of this one process (radix_sort.hpp:98-115 semantics: early exits,
 * kept columns, returned pointer, `aux` untouched on sorted input -- decided
 * globally, exactly as one rsx_sort call would).  devices: HIP device indices, one
 * per rank; an index may repeat (several ranks then share a device).  Shard r =
 * the r-th n/ndev-th of src; MSD split by the highest kept byte, peer-to-peer
 * exchange of the digit ranges, local LSD sorts, each written to its place in
 * the result buffer.  Blocking.  The one-process-per-GPU form of the same
 * algorithm (RCCL all-to-all-v) is radix_sorting_amd/multi.py. */
int rsx_sort_multi(void *src, void *aux, size_t n, rsx_dtype dtype, rsx_order order,
                   const int *devices, int ndev, void **result, rsx_info *info);

/* ---- measurement hooks and input generator (bench.py, tests) ------------------ */

/* Between rsx_profile_begin() and rsx_profile_end() every histogram and scatter
 * kernel the library launches is bracketed by HIP events recorded on the stream
 * the kernel is launched on; rsx_profile_end() waits for them and returns the
 * summed kernel durations.  scatter_bytes = sum over scatter launches of
 * n * 2 * (key bytes + payload bytes), the algorithmic traffic of one pass
 * (SURVEY.md 8d); hist_bytes = sum of n * key bytes. */
typedef struct rsx_profile {
	double   hist_ms;
	double   scatter_ms;
	uint64_t hist_launches;
	uint64_t scatter_launches;
	uint64_t hist_bytes;
	uint64_t scatter_bytes;
	double   leaf_ms;        /* rsx_leaf_sort_kernel (sorts that take one MSB pass and leaves): n * 2 * key bytes per launch
	                            (n * (2 + key bytes) where the leaves read two-byte slots) */
	uint64_t leaf_launches;
	uint64_t leaf_bytes;
	double   narrow_ms;      /* scatter passes that write their keys narrowed into slots (a different instantiation of the
	                            pass kernel, counted apart from scatter_*): n * (key bytes + 2) per launch */
	uint64_t narrow_launches;
	uint64_t narrow_bytes;
	double   called_off_ms;  /* launches that did nothing, or whose output was discarded: the kernels of a sort without a
	                            histogram that its sample or an overflowing slot called off, leaves enqueued for a route the
	                            plan did not choose.  Their time is here, their bytes are in none of the byte counts; the
	                            narrowed level-2 pass and leaves of 8-byte keys are booked with the four-byte slots the device
	                            chose (blocking sorts: the host knows the verdict; the *_inplace_async sorts never learn it
	                            and book what they enqueued). */
	uint64_t called_off_launches;
} rsx_profile;
int rsx_profile_begin(void);
int rsx_profile_end(rsx_profile *out);

/* d_dst[i] = low elem_bytes bytes of (splitmix64 output number first_index + i
 * of the stream seeded with `seed`) & mask: the generator of SURVEY.md section 4
 * and 8d, evaluated counter-based on the device (element i of the serial
 * generator is finalizer(seed + (i+1) * 0x9E3779B97F4A7C15)). */
int rsx_fill_splitmix_device(void *d_dst, size_t n, size_t elem_bytes, uint64_t seed,
                             uint64_t mask, uint64_t first_index, void *stream);

/* Keeps `stream` busy for about `microseconds` (one spinning wave): a known-length
 * occupant for stream / hardware-queue experiments (multi.py picks the stream whose
 * kernels overlap RCCL's with it). */
int rsx_spin_device(uint64_t microseconds, void *stream);

#ifdef __cplusplus
}
#endif
#endif
