"""Shared by tests/test_gpu_inner_routes.py and tests/test_inner_lib_cpu.py: inputs that send the sort INSIDE a feature (unique,
group, rankdata, topk, nth, lex, locate, reduce, join, partition) down a chosen route of the plain sorts, what the two samples
that decide those routes see of them, and wrong results that a comparison against the oracle has to refuse.

The inner sort of 4-byte keys with a 4-byte payload or index goes by one pass per column (rsx_info.hybrid == 0), by one MSB
pass and leaves (1: up to about a million pairs, three kept columns or more), without a histogram (5: from 2^22 pairs on, keys
alone from 7.5 Mi 4-byte or 4.5 Mi 8-byte keys on) or, after a level-1 slot of that route has overflowed, from the first buffers
again.  Every expectation comes from the existing oracles (oracle_lib, reduce_lib, join_lib, lex_lib, nth_lib, topk_lib,
locate_lib, partition_lib); nothing here looks at the library's results.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import nth_lib as nl
import oracle_lib as ol
import pairs_lib as pl
import topk_lib as tl

N22 = (1 << 22) + 3          # the first sizes of the sort without a histogram for pairs and ranks ...
N23 = (1 << 23) + 3          # ... and for 4-byte keys alone (floor: 7.5 Mi)
N64 = 9 * (1 << 19) + 5      # ... and for 8-byte keys alone (floor: 4.5 Mi)
N_ONE_LEVEL = 300001         # one MSB pass and leaves
JOIN_LEFT, JOIN_RIGHT, JOIN_RIGHT_BIG = (1 << 22) + 5, (1 << 20) + 3, (1 << 22) + 7
JOIN_MAX_PAIRS = 1 << 23     # a condition on the join sides, not a measurement
UNIQUE_SAMPLE = 4096         # rsx_unique_sample_kernel: that many keys, n / 4096 apart


# ---- what the library computes from n alone, restated from the text of radix_sorting_amd/csrc/rsx_route_levels.hpp -----------------
def slot_cap(mean):
    """slot_cap_for: 1.25 times the mean, at least seven standard deviations (and eight keys) above it, rounded up to 256 keys."""
    r = int(np.floor(np.sqrt(mean)))
    while (r + 1) * (r + 1) <= mean:
        r += 1
    while r * r > mean:
        r -= 1
    need = max(mean + mean // 4, mean + 7 * (r + 1) + 8)
    return (need + 255) // 256 * 256


def level1_slot(n):
    """The capacity of one of the 256 level-1 slots of a key + payload or rank sort without a histogram."""
    return slot_cap(n >> 8)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def wide(n, dt, seed):
    """Full-width splitmix keys: every byte column varies, nothing is in order."""
    return ol.splitmix_fill(n, dt, seed)


def distinct_wide(count, dt, seed):
    """`count` distinct full-width keys in no order."""
    extra = count // 64 + 64
    while True:
        u = np.unique(ol.splitmix_fill(count + extra, dt, seed))
        if u.size >= count:
            return np.random.default_rng(seed).permutation(u)[:count].copy()
        extra *= 2


def wide_ties(n, dt, seed):
    """n draws from a pool of n / 2 + 3 distinct full-width keys: ties everywhere, in no pattern."""
    pool = distinct_wide(n // 2 + 3, dt, seed)
    return pool[np.random.default_rng(seed + 1).integers(0, pool.size, n)]


def float_specials(dt):
    """+-0.0, +-inf, quiet and signalling-range NaNs of both signs with and without a payload, and the keys next to zero."""
    assert dt in (ol.F32, ol.F64)
    nb = 8 * ol.DTYPE_SIZE[dt]
    top = 1 << (nb - 1)
    if dt == ol.F32:
        inf, qnan = 0x7F800000, 0x7FC00000
    else:
        inf, qnan = 0x7FF0000000000000, 0x7FF8000000000000
    vals = [0, top, inf, inf | top, qnan, qnan | top, qnan | 5, qnan | 5 | top, inf | 1, inf | 1 | top, 1, top | 1]
    return np.array(vals, dtype=ol.NP_BITS[dt])


def with_specials(a, dt, seed, every=16411):
    """A copy of `a` with every `every`-th element, from element 17 on, replaced by one of float_specials(dt): each occurs a few
    dozen times in 2^22 keys -- and no more, for neighbours among them (0 and the smallest denormal, inf and the first NaN) share
    their top sixteen bits, and a level-2 slot holds four times its mean of 64 keys (slots_fit)."""
    sp = float_specials(dt)
    out = np.array(a, dtype=ol.NP_BITS[dt], copy=True)
    at = np.arange(17, out.size, every)
    out[at] = sp[np.random.default_rng(seed).integers(0, sp.size, at.size)]
    return out


def raw_top_byte(digit, dt):
    """The top byte of a raw u32 / f32 key whose DERIVED key (ascending) has the top digit `digit`."""
    if dt == ol.U32:
        return digit
    assert dt == ol.F32
    return (digit ^ 0x80) if digit >= 0x80 else (~digit & 0xFF)


def overflowing(n, seed, digit, dt=ol.U32):
    """wide() u32 / f32 keys with 0.45 of a 1 / 256 share of extra keys moved onto the top digit `digit` of the derived key -- every
    seventh key from element 1000 on, as test_attempt_called_off_after_the_spare_buffers_were_written places them: both samples
    pass them by, and the digit's level-1 slot of 1.25 shares overflows after the slots of the digits below it were written.
    (Digit 0x05's slot lies in the second buffers and 0xF3's in scratch memory where a slot holds a tile of the pass -- 32 Ki
    elements, from about 6.7 Mi pairs on; at 2^22 + 3 a slot holds 20480 and all 256 lie in scratch memory.)"""
    a = wide(n, dt, seed).view(np.uint32).copy()
    extra = int(0.45 * n / 256) + 1
    idx = np.arange(1000, 1000 + extra * 7, 7)
    assert idx[-1] < n
    a[idx] = (a[idx] & np.uint32(0x00FFFFFF)) | np.uint32(raw_top_byte(digit, dt) << 24)
    return a


def digit_share(a, dt, digit, order=ol.ASC):
    """How many times its 1 / 256 share the top digit `digit` of the derived keys holds."""
    k = ol.kdf_keys(a, dt, order)
    shift = 8 * (ol.DTYPE_SIZE[dt] - 1)
    return float(np.count_nonzero((k >> k.dtype.type(shift)) == digit)) * 256.0 / k.size


def join_sides(n, m, dt, seed, specials=False):
    """(left, right): `right` holds m rows -- m - 5 distinct wide keys, five of them twice --, `left` n rows, half of them drawn
    from the right keys and half from wide keys that are none of them, shuffled.  specials (float keys): float_specials on both
    sides, each several times on the left."""
    pool = distinct_wide(m - 5, dt, seed)
    right = np.concatenate([pool, pool[:5]])
    rng = np.random.default_rng(seed + 1)
    half = n // 2
    strangers = wide(n - half + (n - half) // 256 + 64, dt, seed + 2)
    strangers = strangers[~np.isin(strangers, pool)][:n - half]
    assert strangers.size == n - half
    left = np.concatenate([pool[rng.integers(0, pool.size, half)], strangers])
    if specials:
        sp = float_specials(dt)
        right = right.copy()
        right[np.arange(sp.size) * 1009 + 7] = sp          # (each once; two of them once more below)
        right[[3001, 6007]] = sp[[0, 4]]
        left[np.arange(sp.size * 6) * 4099 + 11] = np.tile(sp, 6)
    return rng.permutation(left).astype(ol.NP_BITS[dt]), rng.permutation(right).astype(ol.NP_BITS[dt])


def slots_fit(a, dt, order=ol.ASC):
    """Does every top digit of the derived 4-byte keys fit a level-1 slot, and every pair of top digits a level-2 slot?  (Keys that do
    not are sorted all the same: the attempt without a histogram is called off, which is what overflowing() is for.)"""
    k = ol.kdf_keys(a, dt, order).astype(np.int64)
    n = k.size
    return (int(np.bincount(k >> 24, minlength=256).max()) <= slot_cap(n >> 8) and
            int(np.bincount(k >> 16, minlength=65536).max()) <= slot_cap(n >> 16))


def varying_bits(a, dt, order=ol.ASC):
    k = ol.kdf_keys(a, dt, order)
    return bin(int(np.bitwise_or.reduce(k ^ k[0]))).count("1")


def nth_ranks(kd_sorted, count=65):
    """`count` distinct ranks for radix_sort_nth, in no order: 0, n - 1, both ends of the longest run of equal keys (and the ranks
    next to it), the rest spread evenly.  `kd_sorted`: the derived keys in order."""
    n = kd_sorted.size
    heads = np.flatnonzero(np.r_[True, kd_sorted[1:] != kd_sorted[:-1]])
    lens = np.diff(np.r_[heads, n])
    j = int(np.argmax(lens))
    lo, hi = int(heads[j]), int(heads[j] + lens[j] - 1)
    assert hi > lo, "no key occurs twice"
    ranks = {0, n - 1, lo, hi, max(lo - 1, 0), min(hi + 1, n - 1)}
    step = n // (count + 3)
    i = 1
    while len(ranks) < count:
        ranks.add(i * step + (i % 7))
        i += 1
    return np.random.default_rng(n).permutation(np.array(sorted(ranks), dtype=np.uint64)), (lo, hi)


# ---- what the samples see ---------------------------------------------------------------------------------------------------------
def unique_sample_index(n):
    """rsx_unique_sample_kernel: 4096 keys, n / 4096 apart."""
    step = max(n // UNIQUE_SAMPLE, 1)
    i = np.arange(UNIQUE_SAMPLE, dtype=np.int64) * step
    return i[i < n]


def blind_sample_index(n):
    """rsx_blind_precheck_kernel: 64 places (n - 128) / 63 apart, 128 consecutive keys at each."""
    assert n >= 1 << 20
    place = np.arange(64, dtype=np.int64) * ((n - 128) // 63)
    return (place[:, None] + np.arange(128, dtype=np.int64)[None, :]).ravel()


def columns_varying(a, dt, index, order=ol.ASC):
    """How many byte columns of the derived keys a[index] hold two different bytes or more."""
    k = ol.kdf_keys(np.asarray(a)[index], dt, order)
    return sum(1 for c in range(ol.DTYPE_SIZE[dt]) if np.unique((k >> k.dtype.type(8 * c)) & k.dtype.type(0xFF)).size >= 2)


def sample_sees_descent(a, dt, index, order=ol.ASC):
    """Does one key of the blind sample stand below its left neighbour (inside a place)?"""
    k = ol.kdf_keys(np.asarray(a)[index], dt, order).reshape(64, 128)
    return bool((k[:, 1:] < k[:, :-1]).any())


# ---- the oracle's stable order, once per input ------------------------------------------------------------------------------------
class Ranked(nl.Want):
    """nth_lib.Want (and, through first(), topk_lib.Want) on the stable ranks of oracle_lib.want_ranks: the C restatement up to
    pairs_lib.BIG 4-byte keys, the sorted (key, index) compounds pinned against it in tests/test_oracle.py above."""

    def __init__(self, bits, dt, order=ol.ASC):
        assert ol.DTYPE_SIZE[dt] == 4
        self.bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
        self.dt, self.order = dt, order
        self.ranks = ol.want_ranks(self.bits, dt, order, big=pl.BIG)[0].astype(np.uint64)
        self.sorted = self.bits[self.ranks]
        self.kd = ol.kdf_keys(self.sorted, dt, order)

    first = tl.Want.first


class FirstK:
    """What topk_lib.check reads of a Want, for ONE k of an array too large for a full argsort: the k-th derived key by
    np.partition, the stable argsort of the elements at or below it, the first k of those."""

    def __init__(self, bits, dt, k, order=ol.ASC):
        self.bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
        self.dt, self.order, self.k = dt, order, k
        kd = ol.kdf_keys(self.bits, dt, order)
        kth = np.partition(kd, k - 1)[k - 1]
        at = np.flatnonzero(kd <= kth)                               # (ascending positions: a stable sort keeps ties in input order)
        by_key = at[np.argsort(kd[at], kind="stable")]
        self.idx = by_key[:k].astype(np.uint64)
        self.n_less = int(np.count_nonzero(kd < kth))
        self.n_equal = int(at.size - self.n_less)
        self.kth_raw = int(self.bits[by_key[k - 1]])

    def first(self, k):
        assert k == self.k
        return self.bits[self.idx], self.idx, self.kth_raw, self.n_less, self.n_equal


# ---- comparisons that are not in one of the libraries -----------------------------------------------------------------------------
def same(tag, name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s has %d entries, the oracle %d" % (tag, name, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %s differs from the oracle in %d of %d places, first at %d: %#x != %#x" % (
        tag, name, bad.size, want.size, bad[0], int(got[bad[0]]), int(want[bad[0]]))


def compare_reduce(tag, got, want):
    """(keys, counts, sum, min, max) as bit patterns against reduce_lib.want_reduce's; None on either side: not compared."""
    for name, g, w in zip(("keys", "counts", "sum", "min", "max"), got, want):
        if g is not None and w is not None:
            same(tag, name, g, w)


# ---- wrong results, modelled on the host (tests/test_inner_lib_cpu.py: does every comparison refuse them?) ------------------------
def tied_pair(bits, dt, perm, order=ol.ASC):
    """A position j of the stable order `perm` whose key equals the next one's (the middle one of all of them)."""
    k = ol.kdf_keys(np.asarray(bits)[np.asarray(perm).astype(np.int64)], dt, order)
    at = np.flatnonzero(k[1:] == k[:-1])
    assert at.size, "no two keys tie"
    return int(at[at.size // 2])


def wrong_ties_swapped(bits, dt, perm, order=ol.ASC):
    """(a) a sort that is not stable: the order `perm` with two neighbours of equal keys exchanged.  The keys read through it are
    still in order -- only what travels WITH them (payloads, values, indices) tells."""
    j = tied_pair(bits, dt, perm, order)
    out = np.array(perm, copy=True)
    out[[j, j + 1]] = out[[j + 1, j]]
    return out


def wrong_slot_overwritten(first_buffer, slot, cap, seed=1):
    """(b) a called-off attempt that wrote where the sort behind it starts: a copy of the feature's first key, payload or value
    buffer with the `cap` elements from slot * cap on replaced by other bits."""
    out = np.array(first_buffer, copy=True)
    lo = min(slot * cap, max(out.size - cap, 0))
    junk = ol.splitmix_fill(cap, ol.U64 if out.dtype.itemsize == 8 else ol.U32, 0xBAD0 + seed).astype(out.dtype)
    out[lo:lo + cap] = junk[:out[lo:lo + cap].size] | out.dtype.type(1)
    return out
