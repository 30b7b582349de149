"""Seeded differential fuzz of the eleven feature entry points (unique, group, rankdata, topk, nth, locate, partition, lex, reduce,
join + join_pairs, segments): a generator that draws ALL the dimensions of a call jointly -- dtype, order, n, key style, feature
parameters, wanted outputs, index width, route switches, stream, device or host form --, the reference of every draw from the
oracle-derived *_lib helpers (never from the code under test), the routes include/rsx.h's rules allow for it, wrong answers a
comparison has to refuse, and the driver that makes the call (test_feature_fuzz_lib_cpu.py, test_gpu_feature_fuzz.py).
TEST INFRASTRUCTURE ONLY.

A CASE holds everything that determines one call; `cases(seed, chunk)` is deterministic in (seed, chunk) alone and `inputs(case)`
in the case alone.  `reference(case, inp)` is {name: value} of everything the call must deliver: arrays as bit patterns (index
arrays as uint64, join pairs as int64), counts as ints, "in:<name>" the inputs the call must leave alone, "tails" the bytes behind
the n-th element of every buffer.  `mismatches` / `check` compare bit for bit -- reduce's general float sums are the one exception
(reduce_lib.fsum_bound, the bound test_general_float_sums_are_within_the_bound derives) and join's start counts only where count
> 0 (include/rsx.h).  `run(case, inp, session)` makes the call on the GPU (torch is imported there only) with every buffer n + PAD
elements of FILL bytes, the device ones between guard bands.

Not every combination of the issue's lists is a valid call: rsx_sort_partition* refuses offsets alone (keys or idx must be
wanted), so partition's subsets are the six that hold keys or idx.  Refusals are not drawn (seq_lib's `refused` kind and the
directed tests have them)."""
import collections
import ctypes as C
import itertools
import os

import numpy as np

import group_lib as grl
import inner_lib as il
import join_lib as jl
import lex_lib
import locate_lib as ll
import nth_lib as nl
import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa
import rankdata_lib as rdl
import reduce_lib as rl
import segments_lib as sg
import seq_lib as sl
import topk_lib as tl
import unique_lib as ul

Case = collections.namedtuple("Case", "feature dt order n style seed params outputs idx_bytes switches stream form")

FEATURES = ("unique", "group", "rankdata", "topk", "nth", "locate", "partition", "lex", "reduce", "join", "segments")
FILL, PAD = sl.FILL, sl.PAD
DEFAULT_SEED, DEFAULT_CHUNKS = 20240, 8       # RSX_FUZZ_SEED / RSX_FUZZ_CHUNKS where they are not set (the seed: test_gpu_fuzz.py's)
# Cases per chunk (eight of every feature).  The references of the most expensive chunk of the default run take 1.7 s of one
# core's time (test_feature_fuzz_lib_cpu.py::test_reference_cost prints it; the limit is 3 s, as seq_lib.M is sized for 1.5 s).
CASES_PER_CHUNK = 88
HOST_MAXN = 70001
MAX_PAIRS = 1 << 21
ANCHORS = (64, 256, 1024, 2048, 4096, 8192, 16384, 65536, 262144)
SIGNED = (ol.I8, ol.I16, ol.I32, ol.I64)
FLOATS = (ol.F32, ol.F64)
# key styles: seq_lib.keys_for's 0 .. 5, 6 sorted by derived key, then
REVERSED, SPECIALS, FEW8, FEW12, FEW16, FEW24 = 7, 8, 9, 10, 11, 12
STYLE_NAMES = ("plain", "const-bytes", "bitmask", "few-values", "nearly-sorted", "all-equal", "sorted", "reversed", "specials",
               "bits<=8", "bits9-12", "bits13-16", "bits17-24")
FEW_BITS = {FEW8: (1, 8), FEW12: (9, 12), FEW16: (13, 16), FEW24: (17, 24)}
_STYLE_DRAW = (0, 0, 1, 2, 3, 3, 4, 5, 6, REVERSED, SPECIALS, SPECIALS, FEW8, FEW12, FEW16, FEW24)
# ... and for the features whose routes go by the number of varying bits
_STYLE_DRAW_BITS = (0, 1, 2, 3, 4, 5, 6, REVERSED, SPECIALS, FEW8, FEW8, FEW12, FEW12, FEW16, FEW16, FEW24, FEW24, FEW24, FEW24, FEW24, FEW24)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

# restated from the text of radix_sorting_amd/csrc (as topk_lib.tile restates rsx_topk.hpp): the sizes from which the select routes
# are the default (rsx_topk_api.hpp TOPK_MIN_N, TOPK_MAX_K_DIV; rsx_nth_api.hpp NTH_MIN_N), the bit limits of the
# sort-free routes (rsx_unique_api.hpp, rsx_group_api.hpp, rsx_rankdata_api.hpp, rsx_reduce_shape.hpp, rsx_join_shape.hpp) and
# the most runs of contiguous varying bits they pack (rsx_keybits.hpp bit_runs)
TOPK_MIN_N, TOPK_MAX_K_DIV, NTH_MIN_N = 1 << 18, 8, 1 << 18
DEFAULT_MAX_BITS, UNIQUE_LDS_BITS, GROUP_LDS_BITS, COUNT16_BITS, REDUCE_LDS_BITS, JOIN_TABLE_BITS, MAX_RUNS = 24, 20, 18, 16, 12, 16, 8

# (feature, route) -> why the fuzz cannot reach it at its sizes.  Empty: every route of every feature is reached by the default run
# (JOIN_MERGE only under RSX_JOIN_FORCE=3 -- by its own rule it needs 2^22 left rows).
EXEMPT = {}

ROUTES = {
    "unique": (rsa.UNIQUE_TRIVIAL, rsa.UNIQUE_BITMAP_LDS, rsa.UNIQUE_BITMAP_GLOBAL, rsa.UNIQUE_TABLE, rsa.UNIQUE_SORT),
    "group": (rsa.GROUP_TRIVIAL, rsa.GROUP_RANK_LDS, rsa.GROUP_RANK_GLOBAL, rsa.GROUP_TABLE, rsa.GROUP_SORT),
    "rankdata": (rsa.RANKDATA_TRIVIAL, rsa.RANKDATA_TABLE, rsa.RANKDATA_COUNT16, rsa.RANKDATA_SORT),
    "topk": (rsa.TOPK_TRIVIAL, rsa.TOPK_SELECT, rsa.TOPK_SORT),
    "nth": (rsa.NTH_TRIVIAL, rsa.NTH_SELECT, rsa.NTH_SORT),
    "locate": (rsa.LOCATE_TRIVIAL, rsa.LOCATE_TABLE, rsa.LOCATE_SEARCH, rsa.LOCATE_SORT),
    "partition": (rsa.PARTITION_TRIVIAL, rsa.PARTITION_SCATTER, rsa.PARTITION_SORT),
    "lex": (),
    "reduce": (rsa.REDUCE_TRIVIAL, rsa.REDUCE_CELLS_LDS, rsa.REDUCE_CELLS_GLOBAL, rsa.REDUCE_SORT),
    "join": (rsa.JOIN_TRIVIAL, rsa.JOIN_TABLE, rsa.JOIN_SEARCH, rsa.JOIN_MERGE),
    "segments": (rsa.SEGMENTS_TRIVIAL, rsa.SEGMENTS_LDS, rsa.SEGMENTS_MIXED, rsa.SEGMENTS_LEX),
}


def _subsets(names):
    return tuple(tuple(c) for r in range(1, len(names) + 1) for c in itertools.combinations(names, r))


# the output subsets of every feature, rotated over its cases so that each occurs
SUBSETS = {
    "unique": (("keys",), ("keys", "counts")),
    # (group: the subsets that leave the sort-free routes open -- neither counts nor first -- three times, or those routes are rare)
    "group": _subsets(("inverse", "keys", "counts", "first")) + 2 * _subsets(("inverse", "keys")),
    "rankdata": _subsets(("place", "less", "equal")),
    "topk": _subsets(("keys", "idx")),
    "nth": _subsets(("keys", "idx")),
    "locate": _subsets(("less", "equal", "bins")),
    "partition": tuple(s for s in _subsets(("keys", "idx", "offsets")) if s != ("offsets",)),
    "lex": (("perm",),),
    "reduce": tuple(tuple(n for n, on in zip(("keys", "counts", "sum", "min", "max"), (j >> 4 & 1 or not j & 15, j >> 3 & 1, j & 1, j >> 1 & 1, j >> 2 & 1))
                          if on) for j in range(32)),
    "join": _subsets(("start", "count", "right_perm")),
    "segments": _subsets(("keys", "idx")),
}
# the values of every switch ("" = unset); a case draws each of its feature's independently
SWITCHES = {
    "unique": {"RSX_UNIQUE_MAX_BITS": ("", "0")},
    "group": {"RSX_GROUP_MAX_BITS": ("", "0")},
    "rankdata": {"RSX_RANKDATA_NO_TABLES": ("", "1")},
    "topk": {"RSX_TOPK_FORCE": ("", "1", "2")},
    "nth": {"RSX_NTH_FORCE": ("", "1", "2")},
    "locate": {"RSX_LOCATE_FORCE": ("", "2"), "RSX_LOCATE_MAX_VALUES": ("", "small"), "RSX_LOCATE_COUNTER_SETS": ("", "1")},
    "partition": {"RSX_PARTITION_FORCE": ("", "2"), "RSX_PARTITION_MAX_EDGES": ("", "255"), "RSX_PARTITION_BALLOT_PARTS": ("", "0", "256")},
    "lex": {"RSX_LEX_PACK_BYTES": ("", "1", "8")},
    "reduce": {"RSX_REDUCE_FORCE": ("", "2"), "RSX_REDUCE_MAX_BITS": ("", "24"), "RSX_REDUCE_REPLICAS": ("", "1")},
    "join": {"RSX_JOIN_FORCE": ("", "2", "3"), "RSX_JOIN_NO_TABLE": ("", "1")},
    "segments": {"RSX_SEGMENTS_FORCE": ("", "1", "2"), "RSX_SEGMENTS_MAX_LONG": ("", "0", "2")},
}
ENV_NAMES = tuple(sorted(name for d in SWITCHES.values() for name in d))


# ---- the generator --------------------------------------------------------------------------------------------------------------
def max_n():
    return int(os.environ.get("RSX_FUZZ_MAXN", "300001"))


def _seams(feature, dt, with_idx):
    """the sizes at which the feature's own code takes another path, each from its lib"""
    kb = ol.DTYPE_SIZE[dt]
    if feature == "topk":
        return (tl.tile(kb), 2 * tl.tile(kb))
    if feature == "nth":
        return (nl.tile(kb), 2 * nl.tile(kb))
    if feature == "locate":
        return (rsa.LOCATE_TILE, rsa.LOCATE_TILE * rsa.LOCATE_SHARE_TILES)
    if feature == "partition":
        return (rsa.PARTITION_TILE, rsa.PARTITION_TILE * rsa.PARTITION_SHARE_TILES)
    if feature == "join":
        return (rsa.JOIN_ROW_TILE, rsa.JOIN_EXPAND_TILE)
    if feature == "segments":
        return tuple(x for x in sg.seam_lengths(sg.cap_of(dt, with_idx)) if x >= 2)
    return ()


def _size(rng, anchors, hi):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        n = int(rng.integers(2, 3001))
    elif kind == 1:
        n = int(anchors[int(rng.integers(0, len(anchors)))]) + int(rng.integers(-3, 4))
    else:
        n = int(rng.integers(3000, max(hi, 3001) + 1))
    return min(max(n, 2), max(hi, 2))


def _segment_lengths(seg_seed, target, cap, rows):
    """The segment lengths of a segments case: a mix of 0, 1, 2 .. 256, 257 .. 2048, 2049 .. cap, a few of cap + 1 .. 3 cap and the
    seams of segments_lib, together about `target` keys in at most some 1200 segments (the reference sorts them one by one);
    rows: that many equal rows instead."""
    rng = np.random.default_rng([29, seg_seed])
    if rows:
        return [target // rows] * rows
    seams = sg.seam_lengths(cap)
    out, left = [], target
    longs = 0
    while left > 0 and len(out) < 1200:
        kind = int(rng.choice(7, p=(0.08, 0.08, 0.3, 0.2, 0.16, 0.04, 0.14)))
        if kind == 6:
            length = int(seams[int(rng.integers(0, len(seams)))])
        elif kind == 5 and longs < 3:
            length = int(rng.integers(cap + 1, 3 * cap + 1))
        else:
            lo, hi = ((0, 0), (1, 1), (2, 256), (257, 2048), (2049, cap), (2049, cap))[kind]
            length = int(rng.integers(lo, hi + 1))
        length = min(length, left)
        longs += length > cap
        out.append(length)
        left -= length
    while left > 0:      # (the segment count is spent: the rest in pieces the LDS route still takes)
        length = min(left, int(rng.integers(2049, cap + 1)))
        out.append(length)
        left -= length
    return out


def cases(seed=DEFAULT_SEED, chunk=0):
    """The cases of one chunk: CASES_PER_CHUNK / 11 of every feature, the features taking turns."""
    rng = np.random.default_rng([17, int(seed), int(chunk)])
    per = CASES_PER_CHUNK // len(FEATURES)
    out = []
    for i in range(CASES_PER_CHUNK):
        out.append(_make_case(FEATURES[i % len(FEATURES)], int(chunk) * per + i // len(FEATURES), rng))
    return out


def _make_case(feature, j, rng):
    """The j-th case of a feature: dtype, order and output subset rotate with j (so that each type meets both orders and every
    subset occurs within few cases), everything else is drawn."""
    dt = j % 10
    order = (j // 10 + j) & 1
    outputs = SUBSETS[feature][(j + j // len(SUBSETS[feature])) % len(SUBSETS[feature])]
    if feature == "reduce":
        outputs = SUBSETS[feature][j % 32]
    idx_bytes = int(rng.choice([4, 8]))
    form = "host" if rng.random() < 0.125 else "device"
    stream = "side" if form == "device" and rng.random() < 0.25 else "default"
    with_idx = "idx" in outputs
    hi = min(max_n(), HOST_MAXN) if form == "host" else max_n()
    n = _size(rng, ANCHORS + _seams(feature, dt, with_idx), hi)
    if j % 24 == 11:      # (one case in 24 has n of 0 or 1, in turn: a draw could leave a feature without either)
        n = (j // 24) & 1
    draw = _STYLE_DRAW_BITS if feature in ("unique", "group", "rankdata", "reduce", "join") else _STYLE_DRAW
    style = int(draw[int(rng.integers(0, len(draw)))])
    seed = int(rng.integers(1, 1 << 30))
    switches = {}
    for name, values in SWITCHES[feature].items():
        v = values[int(rng.integers(0, len(values)))]
        if v == "small":
            v = str(int(rng.integers(1, 65)))
        if v:
            switches[name] = v
    params = {}
    if feature == "topk":
        params["k_kind"] = ("one", "two", "draw", "tie", "n-1", "n", "capacity")[int(rng.integers(0, 7))]
    elif feature == "nth":
        params["m"] = int(rng.choice([1, 2, 3, 9, 33, 64, 65, 70, int(rng.integers(1, 71))]))
        if n >= 200000 and rng.random() < 0.5:
            params["m"] = 70      # (more than 64 distinct ranks: only a large n is sure to have them)
    elif feature == "locate":
        params["m"] = int(rng.choice([0, 1, 2, int(rng.integers(3, 300)), int(rng.integers(300, 5001))]))
        params["below"] = int(rng.integers(0, 2))
    elif feature == "partition":
        params["m"] = int(rng.choice([0, 1, 2, 3, 4, 6, 7, int(rng.integers(8, 301)), int(rng.integers(1, 301))]))
        params["below"] = int(rng.integers(0, 2))
    elif feature == "lex":
        ncols = int(rng.integers(1, 6))
        cols = [(dt, order, 0)]
        for c in range(1, ncols):
            if rng.random() < 0.2:      # (a column again, perhaps in the other order)
                src = int(rng.integers(0, c))
                cols.append((cols[src][0], int(rng.integers(0, 2)), cols[src][2]))
            else:
                cols.append((int(rng.integers(0, 10)), int(rng.integers(0, 2)), c))
        params["cols"] = tuple(cols)
    elif feature == "reduce":
        params["val_dt"] = rl.VAL_DTYPES[(j + j // 6) % 6]
        params["vals"] = ("full" if params["val_dt"] not in rl.FLOATS else ("small_ints", "general")[int(rng.integers(0, 2))])
        if params["vals"] == "general" and style in (0, 1, 2, 4, 6, REVERSED, SPECIALS, FEW24):
            n = min(n, 30000)      # (fsum_bound walks the groups one by one: many distinct keys only in a small case)
    elif feature == "join":
        params["how"] = ("inner", "left")[int(rng.integers(0, 2))]
        params["m"] = int(rng.choice([0, 1, int(rng.integers(2, 3000)), int(rng.integers(2, max(n, 3))), _size(rng, ANCHORS, hi)]))
        params["overlap"] = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0]))
        params["dups"] = int(rng.choice([1, 1, 2, 3, 5]))
    elif feature == "segments":
        params["seg_seed"] = int(rng.integers(1, 1 << 30))
        params["local"] = int(rng.integers(0, 2))
        params["target"] = n
        params["rows"] = 0
        if rng.random() < 0.2 and n >= 2:
            cap = sg.cap_of(dt, with_idx)
            length = int(rng.choice([1, 2, 64, 255, 256, 257, 2048, 2049, int(rng.integers(2, 3000)), cap, cap + 1]))
            length = min(length, n)
            params["rows"] = max(n // length, 1)
        n = sum(_segment_lengths(params["seg_seed"], n, sg.cap_of(dt, with_idx), params["rows"]))
    return Case(feature, dt, order, n, style, seed, params, outputs, idx_bytes, switches, stream, form)


def describe(case):
    """One line that names every field."""
    return "%s[%s %s n=%d style=%d(%s) seed=%d params=%s outputs=%s idx=%d switches=%s stream=%s form=%s]" % (
        case.feature, ol.DTYPE_NAMES[case.dt], "desc" if case.order else "asc", case.n, case.style, STYLE_NAMES[case.style], case.seed,
        sorted(case.params.items()), "+".join(case.outputs), case.idx_bytes, sorted(case.switches.items()), case.stream, case.form)


def tag(case, seed, chunk, number):
    return "RSX_FUZZ_SEED=%d RSX_FUZZ_CASE=%d:%d %s" % (seed, chunk, number, describe(case))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def few_bits_mask(kb, lo, hi, rng):
    """A mask of lo .. hi set bits (as many as the width takes) in one to four runs."""
    width = 8 * kb
    p = min(int(rng.integers(lo, hi + 1)), width) if rng.random() < 0.5 else min(hi, width) - int(rng.integers(0, 2))
    runs = int(rng.integers(1, min(4, p) + 1))
    cuts = sorted(rng.choice(np.arange(1, p), size=runs - 1, replace=False).tolist()) if runs > 1 else []
    lens = np.diff([0] + cuts + [p]).tolist()
    gaps = rng.multinomial(width - p, [1.0 / (runs + 1)] * (runs + 1)).tolist()
    mask, at = 0, 0
    for r in range(runs):
        at += gaps[r]
        mask |= ((1 << lens[r]) - 1) << at
        at += lens[r]
    return mask


def keys_for(n, dt, style, seed, order):
    """The keys of a style (bit patterns): seq_lib.keys_for's 0 .. 5; 6 / 7 those in order of the derived key / against it;
    SPECIALS inner_lib.with_specials for floats, the extremes for integers; FEW*: random keys in which only the bits of a random
    mask vary."""
    if n == 0:
        return np.zeros(0, dtype=ol.NP_BITS[dt])
    if style <= 5:
        return sl.keys_for(n, dt, style, seed)
    kb = ol.DTYPE_SIZE[dt]
    rng = np.random.default_rng([19, seed])
    if style in (6, REVERSED):
        a = sl.keys_for(n, dt, seed % 4, seed)
        a = a[ol.stable_argsort_by_kdf(a, dt, order)]
        return a[::-1].copy() if style == REVERSED else a
    if style == SPECIALS:
        a = sl.keys_for(n, dt, 0, seed)
        if dt in FLOATS:
            return il.with_specials(a, dt, seed, every=7) if n > 17 else a
        top = 1 << (8 * kb - 1)
        full = (1 << (8 * kb)) - 1
        sp = np.array([top, top - 1, full, 0, 1] if dt in SIGNED else [0, full, 1, full - 1], dtype=ol.NP_BITS[dt])
        at = np.arange(min(3, n - 1), n, 7)
        a[at] = sp[rng.integers(0, sp.size, at.size)]
        return a
    mask = few_bits_mask(kb, *FEW_BITS[style], rng)
    full = (1 << (8 * kb)) - 1
    const = int(rng.integers(0, full, dtype=np.uint64, endpoint=True)) & ~mask & full
    return ol.splitmix_fill(n, dt, seed, mask) | ol.NP_BITS[dt](const)


def _values_like(keys, m, dt, order, rng):
    """m values for locate / partition: from the keys, from their neighbours in KDF space, from outside their range and (floats)
    from the specials; unsorted, with repeats."""
    ut = ol.NP_BITS[dt]
    if m == 0:
        return np.zeros(0, dtype=ut)
    kb = ol.DTYPE_SIZE[dt]
    full = (1 << (8 * kb)) - 1
    pool = []
    if keys.size:
        kd = ol.kdf_keys(keys, dt, order)
        pick = kd[rng.integers(0, kd.size, m)]
        pool.append(ll.from_kdf(pick, dt, order))
        near = pick.astype(np.uint64)
        step = np.where(rng.integers(0, 2, m) == 1, np.uint64(1), np.uint64(full))      # (+1 or -1 modulo the width)
        pool.append(ll.from_kdf(((near + step) & np.uint64(full)).astype(ut), dt, order))
        lo, hi = int(kd.min()), int(kd.max())
        outside = [v for v in (lo - 1, lo - 2, hi + 1, hi + 2, 0, full) if 0 <= v <= full and not lo <= v <= hi]
        if outside:
            pool.append(ll.from_kdf(np.array(outside, dtype=ut)[rng.integers(0, len(outside), max(m // 8, 1))], dt, order))
    pool.append(ol.splitmix_fill(max(m // 4, 1), dt, int(rng.integers(1, 1 << 30))))
    if dt in FLOATS:
        pool.append(il.float_specials(dt))
    allv = np.concatenate(pool).astype(ut)
    return allv[rng.integers(0, allv.size, m)].copy()


def _vals_for_reduce(case):
    vdt, n = case.params["val_dt"], case.n
    if case.params["vals"] == "small_ints":
        return rl.small_ints(n, vdt, case.seed + 5)
    if case.params["vals"] == "general":
        rng = np.random.default_rng([23, case.seed])
        x = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))
        return np.ascontiguousarray(x, dtype=ol.NP_DTYPES[vdt]).view(ol.NP_BITS[vdt])
    return ol.splitmix_fill(n, vdt, case.seed + 5)


def _join_sides(case):
    """(left, right): the right side m draws from a pool of distinct keys of the case's style (each about `dups` times), the left
    side n rows of which the share `overlap` comes from the pool and the rest from keys that are none of it; the pool shrinks until
    the join has at most MAX_PAIRS pairs."""
    n, m, dt = case.n, case.params["m"], case.dt
    rng = np.random.default_rng([31, case.seed])
    ut = ol.NP_BITS[dt]
    if m == 0:
        return keys_for(n, dt, case.style, case.seed, case.order), np.zeros(0, dtype=ut)
    pool = np.unique(keys_for(max(m // case.params["dups"], 1) + 8, dt, case.style, case.seed + 1, case.order))
    at_right = rng.integers(0, pool.size, m)
    strangers = ol.splitmix_fill(n + 8, dt, case.seed + 2)
    strangers = strangers[~np.isin(strangers, pool)]
    from_pool = rng.random(n) < case.params["overlap"]
    if strangers.size == 0:      # (one-byte keys: the pool may be every key there is)
        from_pool[:] = True
        strangers = pool
    at_left = rng.integers(0, pool.size, n)
    left = np.where(from_pool, pool[at_left], strangers[rng.integers(0, strangers.size, n)]).astype(ut)
    # the pairs are known before anything is joined: a left row from the pool meets every right row drawn from the same key.  The
    # right side is redrawn as its own first half until they fit.
    while m > 1 and int(np.bincount(at_right[:m], minlength=pool.size)[at_left[from_pool]].sum()) > MAX_PAIRS - n:
        m //= 2
    return left, pool[at_right[:m]].astype(ut)


def _tie_middle_rank(kd_sorted):
    """the 1-based rank of the middle of the longest run of equal derived keys (ties straddle it)"""
    n = kd_sorted.size
    heads = np.flatnonzero(np.r_[True, kd_sorted[1:] != kd_sorted[:-1]])
    lens = np.diff(np.r_[heads, n])
    j = int(np.argmax(lens))
    return int(heads[j] + (lens[j] + 1) // 2)


def inputs(case):
    """The call's inputs, from the case alone (numpy bit patterns): `keys` always (join: the left side), then by feature `k`,
    `ranks`, `vals`, `edges`, `cols`, `right`, `offsets`."""
    f, n, dt = case.feature, case.n, case.dt
    rng = np.random.default_rng([37, case.seed])
    d = {}
    if f == "join":
        d["keys"], d["right"] = _join_sides(case)
    elif f == "lex":
        arrays = {}
        ncols = len(case.params["cols"])
        for c, (cdt, _, src) in enumerate(case.params["cols"]):
            if src not in arrays:
                a = keys_for(n, cdt, case.style if src == 0 else (case.style + src) % 5, case.seed + 7 * src, case.order)
                if c < ncols - 1 and n:      # (few distinct values in the leading columns, so that the later ones decide)
                    pool = a[:int(rng.integers(1, 6))]
                    a = pool[rng.integers(0, pool.size, n)].copy()
                arrays[src] = a
        d["cols"] = [arrays[src] for _, _, src in case.params["cols"]]
        d["keys"] = d["cols"][0]
    else:
        d["keys"] = keys_for(n, dt, case.style, case.seed, case.order)
    a = d["keys"]
    if f == "topk":
        kind = case.params["k_kind"]
        if n == 0:
            d["k"] = 0
        else:
            drawn = int(rng.integers(1, n + 1))
            tie = _tie_middle_rank(np.sort(ol.kdf_keys(a, dt, case.order)))
            k = {"one": 1, "two": 2, "draw": drawn, "tie": tie, "n-1": n - 1, "n": n, "capacity": tl.capacity(n) + int(rng.integers(-1, 2))}[kind]
            d["k"] = min(max(k, 1), n)
    elif f == "nth":
        m = case.params["m"] if n else 0
        r = rng.integers(0, max(n, 1), m).astype(np.uint64)
        if m >= 2:
            r[int(rng.integers(0, m))] = 0
            r[int(rng.integers(0, m))] = n - 1
        if m >= 4:
            r[1] = r[2]      # (a rank twice)
        if m > 64 and n >= 200000:
            r = rng.permutation(np.arange(m, dtype=np.uint64) * np.uint64(n // m))     # (more than 64 DISTINCT ranks)
            r[0], r[1] = 0, n - 1
        d["ranks"] = np.ascontiguousarray(r, dtype=np.uint64)
    elif f == "locate":
        d["vals"] = _values_like(a, case.params["m"], dt, case.order, rng)
    elif f == "partition":
        d["edges"] = _values_like(a, case.params["m"], dt, case.order, rng)
    elif f == "reduce":
        d["vals"] = _vals_for_reduce(case)
    elif f == "segments":
        lengths = _segment_lengths(case.params["seg_seed"], case.params["target"], sg.cap_of(dt, "idx" in case.outputs), case.params["rows"])
        assert sum(lengths) == n, (sum(lengths), n)
        d["offsets"] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    for v in d.values():
        for arr in (v if isinstance(v, list) else [v]):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
    return d


# ---- what a case must deliver ---------------------------------------------------------------------------------------------------
def _u64(x):
    return np.ascontiguousarray(x).astype(np.uint64)


def general_floats(case):
    return case.feature == "reduce" and case.params["vals"] == "general"


def reference(case, inp):
    """{name: value} of everything the call must deliver (module docstring); only the outputs the case wants."""
    f, dt, order, n, a = case.feature, case.dt, case.order, case.n, inp["keys"]
    w = {}
    if f == "unique":
        keys, counts = ul.want_unique(a, dt, order)
        w.update(keys=keys, counts=_u64(counts), n_out=int(keys.size))
    elif f == "group":
        inverse, keys, counts, first = grl.want_group(a, dt, order)
        w.update(inverse=_u64(inverse), keys=keys, counts=_u64(counts), first=_u64(first), n_out=int(keys.size))
    elif f == "rankdata":
        place, less, equal = rdl.want_rankdata(a, dt, order)
        w.update(place=_u64(place), less=_u64(less), equal=_u64(equal))
    elif f == "topk":
        k = inp["k"]
        if k:
            w["_want"] = tl.Want(a, dt, order)
            keys, idx, kth, less, equal = w["_want"].first(k)
            w.update(keys=keys, idx=_u64(idx), kth_key=int(kth), n_less=int(less), n_equal=int(equal))
        else:
            w.update(keys=a[:0], idx=np.zeros(0, dtype=np.uint64))
    elif f == "nth":
        r = inp["ranks"]
        if r.size:
            w["_want"] = nl.Want(a, dt, order)
            keys, idx, less, equal = w["_want"].at(r)
            w.update(keys=keys, idx=_u64(idx), n_less=_u64(less), n_equal=_u64(equal))
        else:
            w.update(keys=a[:0], idx=np.zeros(0, dtype=np.uint64), n_less=np.zeros(0, dtype=np.uint64), n_equal=np.zeros(0, dtype=np.uint64))
    elif f == "locate":
        want = ll.Want(a, dt, order)
        less, equal = want.at(inp["vals"])
        w.update(less=_u64(less), equal=_u64(equal), _want=want)
        if "bins" in case.outputs:
            w["bins"] = _u64(want.bins(inp["vals"], bool(case.params["below"])))
    elif f == "partition":
        w["_want"] = pl.Want(a, dt, order)
        idx, keys, offsets = w["_want"].split(inp["edges"], bool(case.params["below"]))
        w.update(keys=keys, idx=_u64(idx), offsets=_u64(offsets))
    elif f == "lex":
        cols = case.params["cols"]
        w.update(perm=_u64(lex_lib.want_perm(inp["cols"], [c[0] for c in cols], [c[1] for c in cols])))
    elif f == "reduce":
        vdt = case.params["val_dt"]
        grp = rl.groups(a, dt, order)
        keys, counts, total, lo, hi = rl.want_reduce(grp, inp["vals"], vdt)
        w.update(keys=keys, counts=_u64(counts), sum=_u64(total), min=lo, max=hi, n_out=int(keys.size))
        if general_floats(case) and "sum" in case.outputs:
            w["sum_bound"] = rl.fsum_bound(grp, inp["vals"], vdt) + 2.0 ** -53 * np.abs(np.ascontiguousarray(total).view(np.float64))
    elif f == "join":
        left_join = case.params["how"] == "left"
        want = jl.Want(a, inp["right"], dt, order)
        li, ri = want.pairs(left_join)
        if n == 0:      # (include/rsx.h, trivial cases: without left rows the right side is not sorted, right_perm is an iota)
            want.perm = np.arange(want.right.size, dtype=np.uint64)
        w.update(start=_u64(want.start), count=_u64(want.count), right_perm=_u64(want.perm), n_pairs=want.n_pairs(left_join),
                 pairs_left=li, pairs_right=ri, _want=want)
    elif f == "segments":
        want = sg.Want(a, dt, inp["offsets"], order)
        w.update(keys=want.keys, idx=_u64(want.local if case.params["local"] else want.idx), _want=want)
    else:
        raise ValueError(f)
    optional = set(SUBSETS[f][-1]) | {n for s in SUBSETS[f] for n in s}
    for name in optional - set(case.outputs):
        w.pop(name, None)
    # the inputs the call must leave as they were (rsx_sort_unique* consumes its src)
    if f != "unique":
        w["in:keys"] = a
    for name in ("right", "vals", "edges", "offsets"):
        if name in inp:
            w["in:" + name] = inp[name]
    if f == "lex":       # (a column that repeats is one buffer)
        for (_, _, s), col in zip(case.params["cols"], inp["cols"]):
            if s:
                w["in:src%d" % s] = col
    w["tails"] = "clean"
    return w


def _same(got, want):
    if isinstance(want, np.ndarray):
        g = np.ascontiguousarray(got)
        if g.dtype.itemsize != want.dtype.itemsize:
            return False
        g = g.view(want.dtype) if g.dtype != want.dtype else g
        return g.shape == want.shape and bool(np.array_equal(g, want))
    return int(got) == int(want)


def mismatches(case, got, want):
    """The names of what `got` gets wrong ([] = all right)."""
    bad = []
    for name, w in want.items():
        if name == "sum_bound" or name.startswith("_"):
            continue
        if name not in got:
            bad.append(name + " (missing)")
        elif name == "tails":
            if not bool(np.all(np.asarray(got[name]) == FILL)):
                bad.append(name)
        elif name == "start":       # (unspecified where count == 0)
            g = np.ascontiguousarray(got[name])
            on = want["count"] > 0 if "count" in want else got["_count_for_start"] > 0
            if g.shape != w.shape or not np.array_equal(g[on], w[on]):
                bad.append(name)
        elif name == "sum" and "sum_bound" in want:
            g = np.ascontiguousarray(got[name])
            if g.shape != w.shape:
                bad.append(name)
            else:
                err = np.abs(g.view(np.float64) - w.view(np.float64))
                if not bool(np.all(err <= want["sum_bound"])):
                    bad.append("%s (largest error / bound = %.3g)" % (name, float(np.max(err / np.maximum(want["sum_bound"], 1e-300)))))
        elif not _same(got[name], w):
            bad.append(name)
    return bad


def check(case, got, want, where=""):
    bad = mismatches(case, got, want)
    assert not bad, "%s: wrong %s" % (where or describe(case), ", ".join(bad))


def clean_answer(case, want):
    """The reference's own answer in the form run() reports it."""
    got = {k: v for k, v in want.items() if k != "sum_bound"}
    got["tails"] = np.full(PAD * 8, FILL, dtype=np.uint8)
    if case.feature == "join" and "count" not in want:
        got["_count_for_start"] = jl.Want(want["in:keys"], want["in:right"], case.dt, case.order).count
    return got


# ---- the routes include/rsx.h's rules allow ---------------------------------------------------------------------------------------
def vary_of(a, dt, order):
    """(vary mask, varying bits, varying byte columns, runs of contiguous varying bits, in order already) of the derived keys"""
    k = ol.kdf_keys(a, dt, order)
    v = int(np.bitwise_or.reduce(k ^ k[0])) if k.size else 0
    runs = bin(v & ~(v << 1)).count("1")
    ncols = sum(1 for b in range(8) if (v >> (8 * b)) & 0xFF)
    return v, bin(v).count("1"), ncols, runs, bool(np.all(k[1:] >= k[:-1]))


class _SortedKeys(nl.Want):
    """nth_lib.Want.course on np.sort of the derived keys (the course reads nothing else)"""

    def __init__(self, bits, dt, order):
        self.bits, self.dt, self.order = bits, dt, order
        self.kd = np.sort(ol.kdf_keys(bits, dt, order))


def expected_routes(case, inp=None):
    """The set of rsa.<FEATURE>_* routes include/rsx.h's rule allows for this input under these switches -- a failed allocation
    aside, which the rules all send to the sort route --, or None where there is no route (lex) or the rule cannot be restated
    from inputs and switches alone."""
    inp = inputs(case) if inp is None else inp
    f, n, dt, order, a, sw = case.feature, case.n, case.dt, case.order, inp["keys"], case.switches
    kb = ol.DTYPE_SIZE[dt]
    if f == "lex":
        return None
    if f in ("unique", "group", "rankdata", "reduce"):
        if n < 2:
            return {0}      # (TRIVIAL is 0 in all four)
        v, vbits, ncols, runs, in_order = vary_of(a, dt, order)
        if f == "reduce":
            if sw.get("RSX_REDUCE_FORCE") == "2":
                return {rsa.REDUCE_SORT}
            if v == 0:
                return {rsa.REDUCE_TRIVIAL}
            if vbits <= int(sw.get("RSX_REDUCE_MAX_BITS", REDUCE_LDS_BITS)) and runs <= MAX_RUNS:
                return {rsa.REDUCE_CELLS_LDS if vbits <= REDUCE_LDS_BITS else rsa.REDUCE_CELLS_GLOBAL}
            return {rsa.REDUCE_SORT}
        if v == 0:
            return {0}
        if f == "unique":
            counts = "counts" in case.outputs
            if sw.get("RSX_UNIQUE_MAX_BITS") == "0":
                return {rsa.UNIQUE_SORT}
            if ncols == 1:
                return {rsa.UNIQUE_TABLE}
            if kb == 2 and counts:
                return {rsa.UNIQUE_SORT if in_order else rsa.UNIQUE_TABLE}
            if not counts and vbits <= DEFAULT_MAX_BITS and runs <= MAX_RUNS:
                return {rsa.UNIQUE_BITMAP_LDS if vbits <= UNIQUE_LDS_BITS else rsa.UNIQUE_BITMAP_GLOBAL}
            return {rsa.UNIQUE_SORT}
        if f == "group":
            counts, first = "counts" in case.outputs, "first" in case.outputs
            if sw.get("RSX_GROUP_MAX_BITS") == "0":
                return {rsa.GROUP_SORT}
            if ncols == 1 and not first:
                return {rsa.GROUP_TABLE}
            if not counts and not first and vbits <= DEFAULT_MAX_BITS and runs <= MAX_RUNS:
                return {rsa.GROUP_RANK_LDS if vbits <= GROUP_LDS_BITS else rsa.GROUP_RANK_GLOBAL}
            return {rsa.GROUP_SORT}
        place = "place" in case.outputs
        if sw.get("RSX_RANKDATA_NO_TABLES") == "1":
            return {rsa.RANKDATA_SORT}
        if ncols == 1:
            return {rsa.RANKDATA_TABLE}
        if not place and kb >= 2 and vbits <= COUNT16_BITS and runs <= MAX_RUNS:
            return {rsa.RANKDATA_COUNT16}
        return {rsa.RANKDATA_SORT}
    if f == "topk":
        k, force = inp["k"], sw.get("RSX_TOPK_FORCE")
        if k == 0 or n < 2:
            return {rsa.TOPK_TRIVIAL}
        if force == "2":
            return {rsa.TOPK_SORT}
        if force == "1" or (n >= TOPK_MIN_N and k <= n // TOPK_MAX_K_DIV):
            return {rsa.TOPK_SELECT}
        return {rsa.TOPK_SORT}
    if f == "nth":
        r, force = inp["ranks"], sw.get("RSX_NTH_FORCE")
        if r.size == 0 or n < 2:
            return {rsa.NTH_TRIVIAL}
        distinct = np.unique(r).size
        if force == "2" or distinct > rsa.NTH_MAX_SELECT_RANKS or (force != "1" and n < NTH_MIN_N):
            return {rsa.NTH_SORT}
        falls = _SortedKeys(a, dt, order).course(r, "idx" in case.outputs).falls_to_sort
        return {rsa.NTH_SORT if falls else rsa.NTH_SELECT}
    if f == "locate":
        vals = inp["vals"]
        if n == 0 or vals.size == 0:
            return {rsa.LOCATE_TRIVIAL}
        if sw.get("RSX_LOCATE_FORCE") == "2":
            return {rsa.LOCATE_SORT}
        if kb <= 2:
            return {rsa.LOCATE_TABLE}
        d, _, _ = ll.search_shape(vals, dt, order)
        return {rsa.LOCATE_SEARCH if d <= int(sw.get("RSX_LOCATE_MAX_VALUES", rsa.LOCATE_MAX_SEARCH_VALUES)) else rsa.LOCATE_SORT}
    if f == "partition":
        edges = inp["edges"]
        if n == 0 or edges.size == 0:
            return {rsa.PARTITION_TRIVIAL}
        if sw.get("RSX_PARTITION_FORCE") == "2":
            return {rsa.PARTITION_SORT}
        return {pl.natural_route(edges, dt, order, int(sw.get("RSX_PARTITION_MAX_EDGES", rsa.PARTITION_DEFAULT_MAX_EDGES)))}
    if f == "join":
        right, force = inp["right"], sw.get("RSX_JOIN_FORCE")
        m = right.size
        if n == 0 or m == 0:
            return {rsa.JOIN_TRIVIAL}
        if force == "2":
            return {rsa.JOIN_SEARCH}
        if force == "3":
            return {rsa.JOIN_MERGE}
        if sw.get("RSX_JOIN_NO_TABLE") != "1":
            if kb == 1:
                return {rsa.JOIN_TABLE}
            if m < 2:
                return None     # (one right key: rsx.h does not say whether "at most 16 bits vary" holds of none)
            _, vbits, _, runs, _ = vary_of(right, dt, order)
            if vbits <= JOIN_TABLE_BITS and runs <= MAX_RUNS:
                return {rsa.JOIN_TABLE}
        return {rsa.JOIN_SEARCH}      # (MERGE by its own rule: from 2^22 left rows on)
    if f == "segments":
        want = sg.Want(a, dt, inp["offsets"], order)
        return {want.natural_route("idx" in case.outputs, sw.get("RSX_SEGMENTS_FORCE"),
                                   int(sw.get("RSX_SEGMENTS_MAX_LONG", rsa.SEGMENTS_DEFAULT_MAX_LONG)))}
    raise ValueError(f)


# ---- wrong answers: each starts from the right one and must be refused; None: this case cannot show it ---------------------------
def _tied_positions(perm_keys_kd):
    at = np.flatnonzero(perm_keys_kd[1:] == perm_keys_kd[:-1])
    return int(at[at.size // 2]) if at.size else None


def _with(got, **changes):
    out = dict(got)
    out.update(changes)
    return out


def wrong_last_dropped(case, inp, want):
    """unique / group / reduce: the last group dropped, the count of groups one less"""
    if case.feature not in ("unique", "group", "reduce") or want.get("n_out", 0) < 1:
        return None
    got = clean_answer(case, want)
    for name in ("keys", "counts", "first", "sum", "min", "max"):
        if name in got:
            got[name] = got[name][:-1]
    got["n_out"] = want["n_out"] - 1
    return got


def wrong_count_off_by_one(case, inp, want):
    """a count one too high at one value: unique / group / reduce counts, rankdata / locate equal, join count, topk / nth n_equal"""
    name = {"unique": "counts", "group": "counts", "reduce": "counts", "rankdata": "equal", "locate": "equal", "join": "count",
            "topk": "n_equal", "nth": "n_equal"}.get(case.feature)
    if name is None or name not in want:
        return None
    got = clean_answer(case, want)
    if isinstance(want[name], np.ndarray):
        if want[name].size == 0:
            return None
        v = want[name].copy()
        v[v.size // 2] += 1
        got[name] = v
    else:
        got[name] = want[name] + 1
    return got


def wrong_ties_swapped(case, inp, want):
    """a sort that is not stable: two elements of equal keys exchanged in what travels with them -- group's first, rankdata's
    place, topk / nth / partition / segments idx, lex's perm, join's right_perm"""
    f, dt, order = case.feature, case.dt, case.order
    got = clean_answer(case, want)
    if f == "rankdata" and "place" in want:
        kd = ol.kdf_keys(inp["keys"], dt, order)
        perm = np.argsort(want["place"])
        j = _tied_positions(kd[perm])
        if j is None:
            return None
        v = want["place"].copy()
        v[[perm[j], perm[j + 1]]] = v[[perm[j + 1], perm[j]]]
        return _with(got, place=v)
    if f == "group" and "first" in want:
        counts = grl.want_group(inp["keys"], dt, order)[2]
        big = np.flatnonzero(counts > 1)
        if big.size == 0:
            return None
        g = int(big[0])
        inverse = grl.want_group(inp["keys"], dt, order)[0]
        v = want["first"].copy()
        v[g] = np.flatnonzero(inverse == g)[1]
        return _with(got, first=v)
    name, keys = {"topk": ("idx", inp["keys"]), "nth": ("idx", inp["keys"]), "partition": ("idx", None), "segments": ("idx", inp["keys"]),
                  "lex": ("perm", None), "join": ("right_perm", inp.get("right"))}.get(f, (None, None))
    if name is None or name not in want or want[name].size < 2:
        return None
    v = want[name].copy()
    if f == "partition":      # two neighbours of one part
        bins = ll.Want(inp["keys"], dt, order).bins(inp["edges"], bool(case.params["below"]))[v.astype(np.int64)]
        j = _tied_positions(bins)
    elif f == "lex":          # two neighbours equal in every column
        rows = v.astype(np.int64)
        same = np.ones(rows.size - 1, dtype=bool)
        for col in inp["cols"]:
            same &= col[rows][1:] == col[rows][:-1]
        at = np.flatnonzero(same)
        j = int(at[at.size // 2]) if at.size else None
    elif f == "segments":
        rows = (sg.Want(inp["keys"], dt, inp["offsets"], order).idx).astype(np.int64)
        kd = ol.kdf_keys(keys[rows], dt, order)
        seg = np.searchsorted(inp["offsets"].astype(np.int64), np.arange(rows.size), side="right")
        at = np.flatnonzero((kd[1:] == kd[:-1]) & (seg[1:] == seg[:-1]))
        j = int(at[at.size // 2]) if at.size else None
    elif f == "nth":
        j = None
        if "idx" in want and want["n_equal"].size and int(want["n_equal"].max()) > 1:
            q = int(np.argmax(want["n_equal"]))
            kd = ol.kdf_keys(inp["keys"], dt, order)
            others = np.flatnonzero(kd == kd[int(v[q])])
            v[q] = others[others != v[q]][0]
            return _with(got, idx=v)
    else:
        j = _tied_positions(ol.kdf_keys(keys[v.astype(np.int64)], dt, order))
    if j is None:
        return None
    v[[j, j + 1]] = v[[j + 1, j]]
    return _with(got, **{name: v})


def wrong_other_side(case, inp, want):
    """locate's bins / partition's offsets and order computed with the other meaning of `below`; segments' idx local where global
    was asked for (and the other way round); a left join's unmatched row given right index 0 instead of -1; topk: the k-th key's
    n_less one too low; reduce: min and max exchanged"""
    f, dt, order = case.feature, case.dt, case.order
    got = clean_answer(case, want)
    if f == "locate" and "bins" in want:
        v = _u64(ll.Want(inp["keys"], dt, order).bins(inp["vals"], not case.params["below"]))
        return None if np.array_equal(v, want["bins"]) else _with(got, bins=v)
    if f == "partition":
        idx, keys, offsets = pl.Want(inp["keys"], dt, order).split(inp["edges"], not case.params["below"])
        alt = {"keys": keys, "idx": _u64(idx), "offsets": _u64(offsets)}
        alt = {k: v for k, v in alt.items() if k in want}
        return None if all(np.array_equal(alt[k], want[k]) for k in alt) else _with(got, **alt)
    if f == "segments" and "idx" in want:
        w = sg.Want(inp["keys"], dt, inp["offsets"], order)
        v = _u64(w.idx if case.params["local"] else w.local)
        return None if np.array_equal(v, want["idx"]) else _with(got, idx=v)
    if f == "join":
        v = want["pairs_right"].copy()
        if not (v == -1).any():
            return None
        v[v == -1] = 0
        return _with(got, pairs_right=v)
    if f == "topk" and "n_less" in want:
        return _with(got, n_less=want["n_less"] - 1 if want["n_less"] else 1)
    if f == "nth" and want["n_less"].size:
        v = want["n_less"].copy()
        v[0] += 1
        return _with(got, n_less=v)
    if f == "reduce" and "min" in want and "max" in want:
        return None if np.array_equal(want["min"], want["max"]) else _with(got, min=want["max"], max=want["min"])
    return None


def wrong_neighbours_exchanged(case, inp, want):
    """two neighbouring entries of the main output exchanged: keys across a segment boundary (segments), two distinct keys (unique,
    group, reduce, topk, nth, partition), two group numbers (group's inverse), two less counts (rankdata, locate), two rows that
    differ (lex), a row's start (join), a sum one unit in the last place off (reduce)"""
    f = case.feature
    got = clean_answer(case, want)
    if f == "segments" and "keys" in want:
        off = inp["offsets"].astype(np.int64)
        v = want["keys"].copy()
        for b in off[1:-1]:
            if 0 < b < v.size and v[b - 1] != v[b]:
                v[[b - 1, b]] = v[[b, b - 1]]
                return _with(got, keys=v)
        return None
    if f == "join" and "start" in want:
        on = np.flatnonzero(want["count"] > 0) if "count" in want else np.flatnonzero(got["_count_for_start"] > 0)
        if on.size == 0:
            return None
        v = want["start"].copy()
        v[on[on.size // 2]] += 1
        return _with(got, start=v)
    if f == "reduce" and "sum" in want and want["sum"].size and "sum_bound" not in want:
        v = want["sum"].copy()
        v[v.size // 2] ^= np.uint64(1)
        return _with(got, sum=v)
    name = {"unique": "keys", "group": "inverse", "reduce": "keys", "topk": "keys", "nth": "keys", "partition": "keys", "rankdata": "less",
            "locate": "less", "lex": "perm"}.get(f)
    if name == "inverse" and name not in want:
        name = "keys"
    if name is None or name not in want or want[name].size < 2:
        return None
    v = want[name].copy()
    at = np.flatnonzero(v[1:] != v[:-1])
    if at.size == 0:
        return None
    j = int(at[at.size // 2])
    v[[j, j + 1]] = v[[j + 1, j]]
    return _with(got, **{name: v})


def wrong_tail_written(case, inp, want):
    """everything asked for is right, and one byte behind it was written"""
    got = clean_answer(case, want)
    t = got["tails"].copy()
    t[t.size // 2] ^= 0xFF
    return _with(got, tails=t)


def wrong_input_written(case, inp, want):
    """an input the call must leave alone comes back changed"""
    names = [k for k in want if k.startswith("in:") and isinstance(want[k], np.ndarray) and want[k].size]
    if not names:
        return None
    got = clean_answer(case, want)
    v = want[names[-1]].copy()
    v[v.size // 2] ^= v.dtype.type(1)
    return _with(got, **{names[-1]: v})


WRONG = (wrong_last_dropped, wrong_count_off_by_one, wrong_ties_swapped, wrong_other_side, wrong_neighbours_exchanged,
         wrong_tail_written, wrong_input_written)


# ---- running a case on the GPU ------------------------------------------------------------------------------------------------
class _Dev:
    """device buffers: seq_lib.Bufs (n + PAD elements of FILL bytes between guard bands) addressed by name"""

    def __init__(self):
        self.b = sl.Bufs(1 << 16)
        self.t = {}

    def new(self, name, n, size, data=None):
        self.t[name] = (self.b.new(name, n, size, data), size)
        return self.b.ptr(name)

    def names(self):
        return list(self.t)

    def read(self, name, count=None):
        t, size = self.t[name]
        a = np.ascontiguousarray(t.detach().cpu().numpy()).view(UINT[size])
        return a if count is None else a[:count]

    def tails(self):
        return self.b.tails()

    def check_guards(self):
        self.b.check_guards()


class _Host:
    """host buffers of the same shape (no guard bands: the tails alone tell)"""

    def __init__(self):
        self.a = {}

    def new(self, name, n, size, data=None):
        raw = np.full((n + PAD) * size, FILL, dtype=np.uint8)
        if data is not None:
            d = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert d.size == n * size, (name, d.size, n, size)
            raw[:d.size] = d
        self.a[name] = (raw, n, size)
        return raw.ctypes.data

    def names(self):
        return list(self.a)

    def read(self, name, count=None):
        raw, n, size = self.a[name]
        a = raw[:n * size].view(UINT[size]).copy()
        return a if count is None else a[:count]

    def tails(self):
        return np.concatenate([raw[n * size:] for raw, n, size in self.a.values()]) if self.a else np.zeros(0, dtype=np.uint8)

    def check_guards(self):
        pass


class Session:
    """One context for the cases of a chunk: the default stream's, and one side stream's for the side-stream cases (released by
    close())."""

    def __init__(self):
        import torch
        self.side = torch.cuda.Stream()

    def close(self):
        import torch
        torch.cuda.synchronize()
        rsa.lib().rsx_release_stream(C.c_void_p(self.side.cuda_stream))


def run(case, inp, session):
    """Make the call.  Returns (got, mem, info): `got` in the shape of reference(), `mem` for the guards."""
    import torch
    if case.form == "host":
        return _run(case, inp, _Host(), None)
    if case.stream == "side":
        with torch.cuda.stream(session.side):
            return _run(case, inp, _Dev(), session.side)
    return _run(case, inp, _Dev(), torch.cuda.current_stream())


def _run(case, inp, M, stream):
    f, dt, order, n, ib = case.feature, case.dt, case.order, case.n, case.idx_bytes
    kb = ol.DTYPE_SIZE[dt]
    lib = rsa.lib()
    device = stream is not None
    fn = lambda name: getattr(lib, name + ("_device" if device else ""))
    S = [C.c_void_p(stream.cuda_stream)] if device else []      # (the stream argument: the device forms have it, the host forms do not)
    wants = lambda name: name in case.outputs
    out = lambda name, count, size: M.new(name, count, size) if wants(name) else None
    got, info = {}, None
    a = inp["keys"]
    src = M.new("in:keys", n, kb, a)

    def sync():
        if device:
            stream.synchronize()

    if f == "unique":
        aux = M.new("aux", n, kb)
        counts = out("counts", n, ib)
        res, nu, info = C.c_void_p(), C.c_size_t(0), rsa.UniqueInfo()
        rsa.check(fn("rsx_sort_unique")(src, aux, n, dt, order, counts, ib if counts else 0, *S, C.byref(res), C.byref(nu), C.byref(info)))
        sync()
        g = nu.value
        assert res.value in (src, aux) or n == 0, "the result is neither src nor aux"
        got.update(n_out=g, keys=M.read("aux" if res.value == aux and n else "in:keys", g))
        if counts:
            got["counts"] = _u64(M.read("counts", g))
    elif f == "group":
        o = [out("inverse", n, ib), out("keys", n, kb), out("counts", n, ib), out("first", n, ib)]
        ng, info = C.c_size_t(0), rsa.GroupInfo()
        rsa.check(fn("rsx_sort_group")(src, n, dt, order, o[0], o[1], o[2], o[3], ib, *S, C.byref(ng), C.byref(info)))
        sync()
        g = ng.value
        got["n_out"] = g
        for name, count in (("inverse", n), ("keys", g), ("counts", g), ("first", g)):
            if wants(name):
                got[name] = M.read(name, count) if name == "keys" else _u64(M.read(name, count))
    elif f == "rankdata":
        o = [out(name, n, ib) for name in ("place", "less", "equal")]
        info = rsa.RankdataInfo()
        rsa.check(fn("rsx_sort_rankdata")(src, n, dt, order, o[0], o[1], o[2], ib, *S, C.byref(info)))
        sync()
        for name in case.outputs:
            got[name] = _u64(M.read(name, n))
    elif f == "topk":
        k = inp["k"]
        ko, io = out("keys", k, kb), out("idx", k, ib)
        info = rsa.TopkInfo()
        rsa.check(fn("rsx_sort_topk")(src, n, k, dt, order, ko, io, ib, *S, C.byref(info)))
        sync()
        if k:
            got.update(kth_key=info.kth_key, n_less=info.n_less, n_equal=info.n_equal)
        if ko:
            got["keys"] = M.read("keys", k)
        if io:
            got["idx"] = _u64(M.read("idx", k))
    elif f == "nth":
        r = inp["ranks"]
        m = r.size
        ko, io = out("keys", m, kb), out("idx", m, ib)
        ranks = np.array(r, dtype=np.uint64)
        less, equal = np.full(m, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(m, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        info = rsa.NthInfo()
        rsa.check(fn("rsx_sort_nth")(src, n, rsa._u64p(ranks), m, dt, order, ko, io, ib, rsa._u64p(less), rsa._u64p(equal), *S, C.byref(info)))
        sync()
        got.update(n_less=less, n_equal=equal)
        assert np.array_equal(ranks, r), "the ranks were written"
        if ko:
            got["keys"] = M.read("keys", m)
        if io:
            got["idx"] = _u64(M.read("idx", m))
    elif f in ("locate", "partition"):
        vals = inp["vals" if f == "locate" else "edges"]
        m = vals.size
        vp = M.new("in:vals" if f == "locate" else "in:edges", m, kb, vals)
        if f == "locate":
            o = [out("less", m, ib), out("equal", m, ib), out("bins", n, ib)]
            info = rsa.LocateInfo()
            rsa.check(fn("rsx_sort_locate")(src, n, vp, m, dt, order, o[0], o[1], o[2], ib, rsa.LOCATE_BINS_BELOW if case.params["below"] else 0,
                                            *S, C.byref(info)))
            counts = {"less": m, "equal": m, "bins": n}
        else:
            o = [out("keys", n, kb), out("idx", n, ib), out("offsets", m + 2, ib)]
            info = rsa.PartitionInfo()
            rsa.check(fn("rsx_sort_partition")(src, n, vp, m, dt, order, o[0], o[1], o[2], ib, rsa.PARTITION_BELOW if case.params["below"] else 0,
                                               *S, C.byref(info)))
            counts = {"keys": n, "idx": n, "offsets": m + 2}
        sync()
        for name in case.outputs:
            got[name] = M.read(name, counts[name]) if name == "keys" else _u64(M.read(name, counts[name]))
    elif f == "lex":
        cols = case.params["cols"]
        ptrs = {0: src}
        for c, (cdt, _, s) in enumerate(cols):
            if s not in ptrs:
                ptrs[s] = M.new("in:src%d" % s, n, ol.DTYPE_SIZE[cdt], inp["cols"][c])
        arr = lex_lib.lex_cols([ptrs[s] for _, _, s in cols], [c[0] for c in cols], [c[1] for c in cols])
        po = M.new("perm", n, ib)
        info = rsa.LexInfo()
        rsa.check(fn("rsx_sort_lex")(arr, len(cols), n, po, ib, *S, C.byref(info)))
        sync()
        got["perm"] = _u64(M.read("perm", n))
    elif f == "reduce":
        vdt = case.params["val_dt"]
        vb = ol.DTYPE_SIZE[vdt]
        vp = M.new("in:vals", n, vb, inp["vals"])
        o = [out("keys", n, kb), out("counts", n, ib), out("sum", n, 8), out("min", n, vb), out("max", n, vb)]
        ops = (rsa.REDUCE_SUM if o[2] else 0) | (rsa.REDUCE_MIN if o[3] else 0) | (rsa.REDUCE_MAX if o[4] else 0)
        ng, info = C.c_size_t(0), rsa.ReduceInfo()
        rsa.check(fn("rsx_sort_reduce")(src, vp, n, dt, order, vdt, ops, o[0], o[1], ib, o[2], o[3], o[4], *S, C.byref(ng), C.byref(info)))
        sync()
        g = ng.value
        got["n_out"] = g
        for name in case.outputs:
            got[name] = _u64(M.read(name, g)) if name in ("counts", "sum") else M.read(name, g)
    elif f == "join":
        right = inp["right"]
        m = right.size
        rp = M.new("in:right", m, kb, right)
        o = [out("start", n, ib), out("count", n, ib), out("right_perm", m, ib)]
        flags = rsa.JOIN_LEFT if case.params["how"] == "left" else 0
        pairs, info = C.c_uint64(0xDEAD), rsa.JoinInfo()
        rsa.check(fn("rsx_sort_join")(src, n, rp, m, dt, order, o[0], o[1], o[2], ib, flags, *S, C.byref(pairs), C.byref(info)))
        sync()
        got["n_pairs"] = int(pairs.value)
        for name, count in (("start", n), ("count", n), ("right_perm", m)):
            if wants(name):
                got[name] = _u64(M.read(name, count))
        # phase 2 into buffers of exactly n_pairs entries: from the arrays phase 1 wrote, the reference's where one was not asked for
        want = jl.Want(a, right, dt, order)
        got["_count_for_start"] = want.count
        total = want.n_pairs(bool(flags))
        it = UINT[ib]
        p2 = [o[0] or M.new("start (reference)", n, ib, want.start.astype(it)), o[1] or M.new("count (reference)", n, ib, want.count.astype(it)),
              o[2] or M.new("right_perm (reference)", m, ib, want.perm.astype(it))]
        lo, ro = M.new("pairs_left", total, ib), M.new("pairs_right", total, ib)
        pairs2 = C.c_uint64(0xDEAD)
        rsa.check((lib.rsx_join_pairs_device if device else lib.rsx_join_pairs)(p2[0], p2[1], p2[2], n, m, ib, flags, lo, ro, total, *S,
                                                                                 C.byref(pairs2)))
        sync()
        assert int(pairs2.value) == total, ("rsx_join_pairs counts %d pairs, the reference %d" % (int(pairs2.value), total))
        signed = {4: np.int32, 8: np.int64}[ib]
        got["pairs_left"] = M.read("pairs_left", total).view(signed).astype(np.int64)
        got["pairs_right"] = M.read("pairs_right", total).view(signed).astype(np.int64)
    elif f == "segments":
        offsets = inp["offsets"]
        m = offsets.size - 1
        op = None
        if not case.params["rows"]:
            op = M.new("in:offsets", m + 1, ib, offsets.astype(UINT[ib]))
        ko, io = out("keys", n, kb), out("idx", n, ib)
        info = rsa.SegmentsInfo()
        rsa.check(fn("rsx_sort_segments")(src, n, op, m, ib, dt, order, ko, io, rsa.SEGMENTS_LOCAL_IDX if case.params["local"] else 0, *S,
                                          C.byref(info)))
        sync()
        if ko:
            got["keys"] = M.read("keys", n)
        if io:
            got["idx"] = _u64(M.read("idx", n))
        if op is None:
            got["in:offsets"] = offsets
    else:
        raise ValueError(f)
    for name in M.names():
        if name.startswith("in:") and not (f == "unique" and name == "in:keys"):
            v = M.read(name)
            got[name] = _u64(v) if name == "in:offsets" else v
    got["tails"] = M.tails()
    got["route"] = getattr(info, "route", None)
    return got, M, info
