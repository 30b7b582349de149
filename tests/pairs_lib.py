"""Payloads that are NOT the input position, key inputs that tie, and the expectation of a key + payload sort.

TEST INFRASTRUCTURE ONLY (as oracle_lib.py): imported by tests/test_pairs_lib_cpu.py, tests/test_gpu_payloads.py and the
key + payload halves of tests/test_gpu_routes.py / tests/test_gpu_async_routes.py.

Why: a payload of arange(n) * a + b ascends with the input position and has no high bit set, so a sort that breaks ties by
payload VALUE, that loses a payload's top bits, or that writes the element's index where the payload belongs gives the same
bytes as a correct one.  The families below each tell at least one of those wrong sorts from the right one
(tests/test_pairs_lib_cpu.py shows which), and the expectation never comes from the library:
perm = the stable order of the derived keys (radix_sort_basic_kdf.hpp:19-46), want_keys = a[perm], want_vals = vals[perm].
"""
import numpy as np

import oracle_lib as ol

FAMILIES = ("random", "reversed", "edges", "keybound")
_UT = {4: np.uint32, 8: np.uint64}
_CODE = {4: ol.U32, 8: ol.U64}
# 4-byte keys above this many take oracle_lib.want_ranks' sorted (key, index) compounds instead of numpy's stable argsort
BIG = 1 << 22


def full_mask(dt):
    return (1 << (8 * ol.DTYPE_SIZE[dt])) - 1


def payload_seed(seed):
    """The seed of the `random` family: another splitmix64 stream than the keys' (which use `seed` itself)."""
    return 0x5EED0000 + 7919 * seed + 1


# ---- payload families: deterministic functions of (n, width, seed) -- and of the keys for `keybound` ------------------------
def payloads(family, n, width, seed=0, keys=None):
    """n payloads of `width` bytes (4 or 8) as an unsigned array.
    random    splitmix64 bits of the payload's width: every bit position used, nothing index-like
    reversed  n - 1 - i: descends with the position, so the order inside every run of equal keys flips if ties go by value
    edges     0, ~0, 1 << (w-1), (1 << (w-1)) - 1, 1, ~1 by i % 6: top bit and sign of the carrier
    keybound  the key's own bits (zero-extended or truncated) ^ 0xA5.., rotated left by 7: wrong per element beside another key"""
    ut = _UT[width]
    w = 8 * width
    full = (1 << w) - 1
    if family == "random":
        return ol.splitmix_fill(n, _CODE[width], payload_seed(seed))
    if family == "reversed":
        return (np.uint64(n - 1) - np.arange(n, dtype=np.uint64)).astype(ut) if n else np.zeros(0, dtype=ut)
    if family == "edges":
        cycle = np.array([0, full, 1 << (w - 1), (1 << (w - 1)) - 1, 1, full - 1], dtype=ut)
        return cycle[np.arange(n) % 6]
    if family == "keybound":
        assert keys is not None and len(keys) == n
        k = (np.asarray(keys).astype(np.uint64) & np.uint64(full)).astype(ut)
        k ^= ut(0xA5A5A5A5A5A5A5A5 & full)
        return (k << ut(7)) | (k >> ut(w - 7))
    raise ValueError(family)


def increasing(n, width, a=7, b=3):
    """The family the suite had before: arange(n) * a + b (kept to show what it cannot see)."""
    return (np.arange(n, dtype=np.uint64) * np.uint64(a) + np.uint64(b)).astype(_UT[width])


# ---- key inputs with ties -----------------------------------------------------------------------------------------------
def every_key_twice(n, dt, seed, mask=None):
    """A half-length splitmix array behind itself: ties everywhere, half the array apart, every byte column still spread."""
    base = ol.splitmix_fill(n - n // 2, dt, seed, full_mask(dt) if mask is None else mask)
    return np.concatenate([base[: n // 2], base])


def runs_of_four(n, dt, seed, mask=None):
    """Every key at i, i + 1, i + 2, i + 3."""
    base = ol.splitmix_fill((n + 3) // 4, dt, seed, full_mask(dt) if mask is None else mask)
    return np.repeat(base, 4)[:n].copy()


def tied_fraction(a):
    """The share of the elements whose key another element has too."""
    s = np.sort(np.ascontiguousarray(a))
    if s.size < 2:
        return 0.0
    eq = s[1:] == s[:-1]
    tied = np.zeros(s.size, dtype=bool)
    tied[1:] |= eq
    tied[:-1] |= eq
    return float(tied.sum()) / s.size


def assert_ties(a):
    f = tied_fraction(a)
    assert f >= 0.5, "only %.1f %% of the keys tie: stability would hardly show" % (100 * f)
    return a


# ---- the expectation ---------------------------------------------------------------------------------------------------
class Order:
    """What the reference decides about the keys `a` alone: the stable permutation, the buffer the result ends in
    (radix_sort.hpp:92), the kept columns (:64-70) and the early exit (:60-62)."""

    def __init__(self, a, dt, order=ol.ASC):
        a = np.ascontiguousarray(a).view(ol.NP_BITS[dt])
        self.a, self.dt, self.order = a, dt, order
        if ol.DTYPE_SIZE[dt] == 4 and a.size > BIG:
            self.perm = ol.want_ranks(a, dt, order, big=BIG)[0]
        else:
            self.perm = ol.stable_argsort_by_kdf(a, dt, order)
        _, self.in_aux, winfo = ol.oracle_sort(a, dt, order)
        self.cols = list(winfo.cols[:winfo.ncols])
        self.early_exit = int(winfo.early_exit)
        self.keys = a[self.perm]

    def vals(self, vals):
        return np.ascontiguousarray(vals)[self.perm]


def _bits(x, ut):
    if hasattr(x, "detach"):           # a torch tensor (bit patterns travel in same-width signed tensors)
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).view(ut)


def _first_difference(got, want, name, what):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    return "%s: %d of %d %s differ, first at %d: got %#x, want %#x" % (what, bad.size, want.size, name, i, int(got[i]), int(want[i]))


def compare(want, vals, got_keys, got_vals, info=None, route=None, want_route=None, not_route=None, what=""):
    """The one comparison of all key + payload tests.  `want`: an Order; `vals`: the payloads as given to the sort; `got_*`: the
    arrays the sort returned (numpy or torch); `info`: the rsx_info of a blocking call (device-scheduled calls have none: their
    result is always in the first buffers); `route`: what rsx_async_route said, where there is no info.
    Bit for bit: keys, payloads; result_in_aux, kept columns and early exit against the oracle; the route where one is named."""
    gk = _bits(got_keys, ol.NP_BITS[want.dt])
    wv = want.vals(vals)
    gv = _bits(got_vals, wv.dtype)
    r = route if route is not None else (int(info.hybrid) if info is not None else None)
    what = (what, "route", r)
    assert gk.shape == want.keys.shape and gv.shape == wv.shape, what
    if not np.array_equal(gk, want.keys):
        raise AssertionError(_first_difference(gk, want.keys, "keys", what))
    if not np.array_equal(gv, wv):
        raise AssertionError(_first_difference(gv, wv, "payloads", what))
    if info is not None:
        assert info.result_in_aux == want.in_aux, (what, info.result_in_aux, want.in_aux)
        assert info.kept_columns() == want.cols, (what, info.kept_columns(), want.cols)
        assert info.early_exit == want.early_exit, (what, info.early_exit, want.early_exit)
    if want_route is not None:
        assert r == want_route, (what, "wanted route", want_route)
    if not_route is not None:
        assert r is not None and r != not_route, (what, "wanted any route but", not_route)


# ---- three wrong sorts, modelled on the host (tests/test_pairs_lib_cpu.py: does a family tell them from the right one?) ----
def wrong_tie_break_by_value(a, dt, vals, order=ol.ASC):
    """(a) equal keys ordered by payload value: a sort of (key, payload) compounds where (key, position) ones belong."""
    perm = np.lexsort((np.ascontiguousarray(vals), ol.kdf_keys(a, dt, order)))
    return np.ascontiguousarray(vals)[perm]


def wrong_top_bits_lost(want_vals):
    """(b) the payloads' top four bits cleared: a carrier that keeps something else there."""
    w = 8 * want_vals.itemsize
    return want_vals & want_vals.dtype.type((1 << (w - 4)) - 1)


def wrong_index_for_payload(want):
    """(c) the element's input index written where its payload belongs (what a rank sort writes)."""
    return want.perm


# ---- the same expectation on the device, for arrays the host does not sort in seconds -------------------------------------
def device_expectation(keys, vals, dt, order=ol.ASC):
    """(want_keys, want_vals, share of the keys that tie) of 4-byte keys as torch tensors: the derived keys (radix_sort_basic_kdf.hpp:19-46) as int64, a
    stable torch.sort for the permutation, two gathers.  torch.sort is only the reference here; nothing of the library runs."""
    import torch
    assert ol.DTYPE_SIZE[dt] == 4 and keys.dtype == torch.int32
    k = keys.to(torch.int64)
    k &= 0xFFFFFFFF
    if dt == ol.I32:
        k ^= 0x80000000
    elif dt == ol.F32:
        k = torch.where(k >= 0x80000000, k ^ 0xFFFFFFFF, k ^ 0x80000000)
    else:
        assert dt == ol.U32
    if order == ol.DESC:
        k ^= 0xFFFFFFFF
    k, perm = torch.sort(k, stable=True)
    eq = k[1:] == k[:-1]
    tied = torch.zeros(k.numel(), dtype=torch.bool, device=k.device)
    tied[1:] |= eq
    tied[:-1] |= eq
    share = float(tied.sum().item()) / max(1, k.numel())
    del k, eq, tied
    return keys[perm], vals[perm], share
