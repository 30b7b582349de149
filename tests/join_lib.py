"""Shared by tests/test_gpu_join*.py and tests/test_join_lib_cpu.py: the equi-join of two key columns from NumPy on the ORACLE's
derived keys (never from the code under test) -- a stable argsort of the right derived keys, np.searchsorted left / right of the
left derived keys over them, the pairs by np.repeat and offset arithmetic --, and one way to call rsx_sort_join_device and
rsx_join_pairs_device.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import radix_sorting_amd as rsa


class Want:
    """What NumPy says about joining `left` with `right` (bit patterns of dtype `dt`)."""

    def __init__(self, left, right, dt, order=ol.ASC):
        self.dt, self.order = dt, order
        self.left = np.ascontiguousarray(left, dtype=ol.NP_BITS[dt])
        self.right = np.ascontiguousarray(right, dtype=ol.NP_BITS[dt])
        kl = ol.kdf_keys(self.left, dt, order)
        kr = ol.kdf_keys(self.right, dt, order)
        self.perm = np.argsort(kr, kind="stable").astype(np.uint64)
        sr = kr[self.perm.astype(np.int64)]
        self.start = np.searchsorted(sr, kl, side="left").astype(np.uint64)
        self.count = (np.searchsorted(sr, kl, side="right").astype(np.uint64) - self.start).astype(np.uint64)

    def n_pairs(self, left_join=False):
        return int(np.maximum(self.count, 1).sum()) if left_join else int(self.count.sum())

    def pairs(self, left_join=False):
        return pairs_of(self.start, self.count, self.perm, left_join)


def pairs_of(start, count, perm, left_join=False):
    """(left_idx, right_idx) int64 of ranges as phase 1 writes them, ordered by left row, then by right row; -1: no match."""
    start, count, perm = (np.asarray(a).astype(np.int64) for a in (start, count, perm))
    eff = np.maximum(count, 1) if left_join else count
    total = int(eff.sum())
    li = np.repeat(np.arange(count.size, dtype=np.int64), eff)
    first = np.cumsum(eff) - eff                     # the position of every row's first pair
    t = np.arange(total, dtype=np.int64) - np.repeat(first, eff)
    at = np.repeat(start, eff) + t
    matched = np.repeat(count > 0, eff)
    ri = np.full(total, -1, dtype=np.int64)
    ri[matched] = perm[at[matched]]
    return li, ri


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def call_device(left_t, n, right_t, m, dt, order, idx_bytes, start_t=None, count_t=None, perm_t=None, flags=0, stream=None):
    """rsx_sort_join_device on device tensors (None: that output is not asked for).  Returns (rc, n_pairs, info)."""
    info, pairs = rsa.JoinInfo(), C.c_uint64(0xDEAD)
    p = lambda t: None if t is None else t.data_ptr()
    rc = rsa.lib().rsx_sort_join_device(p(left_t), n, p(right_t), m, dt, order, p(start_t), p(count_t), p(perm_t), idx_bytes, flags,
                                        _stream(stream), C.byref(pairs), C.byref(info))
    return rc, int(pairs.value), info


def call_pairs(start_t, count_t, perm_t, n, m, idx_bytes, flags, out_left_t, out_right_t, capacity, stream=None):
    """rsx_join_pairs_device on device tensors.  Returns (rc, n_pairs)."""
    pairs = C.c_uint64(0xDEAD)
    p = lambda t: None if t is None else t.data_ptr()
    rc = rsa.lib().rsx_join_pairs_device(p(start_t), p(count_t), p(perm_t), n, m, idx_bytes, flags, p(out_left_t), p(out_right_t), capacity,
                                         _stream(stream), C.byref(pairs))
    return rc, int(pairs.value)


def host(t):
    """An index output (device tensor or numpy array, 4 or 8 bytes wide) as uint64."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64).astype(np.uint64)


def signed(t):
    """... as int64, all ones -> -1."""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.int32 if a.itemsize == 4 else np.int64).astype(np.int64)


def check(tag, want, start_t, count_t, perm_t, n_pairs, info, left_join=False, route=None, left_t=None, right_t=None):
    """Phase 1's outputs (of exactly n resp. m elements, or None) against NumPy: start only where count > 0; the inputs unchanged."""
    n, m = want.left.size, want.right.size
    if count_t is not None:
        got = host(count_t)
        assert got.size == n and np.array_equal(got, want.count), (tag, "count", np.flatnonzero(got != want.count)[:8], got[:8], want.count[:8])
    if start_t is not None:
        got = host(start_t)
        on = want.count > 0
        assert got.size == n and np.array_equal(got[on], want.start[on]), (tag, "start", np.flatnonzero((got != want.start) & on)[:8])
    if perm_t is not None:
        got = host(perm_t)
        assert got.size == m and np.array_equal(got, want.perm), (tag, "right_perm", np.flatnonzero(got != want.perm)[:8])
    assert n_pairs == want.n_pairs(left_join), (tag, "n_pairs", n_pairs, want.n_pairs(left_join))
    if left_t is not None:
        assert np.array_equal(left_t.cpu().numpy().view(ol.NP_BITS[want.dt]), want.left), (tag, "left was written")
    if right_t is not None:
        assert np.array_equal(right_t.cpu().numpy().view(ol.NP_BITS[want.dt]), want.right), (tag, "right was written")
    if route is not None:
        assert info.route == route, (tag, "route", info.route)
    assert info.key_bytes == ol.DTYPE_SIZE[want.dt], tag
    assert info.left_sorted == (1 if info.route == rsa.JOIN_MERGE and n >= 2 else 0), (tag, info.left_sorted)
    if info.route == rsa.JOIN_TABLE:
        assert info.table_bytes == (1024 if ol.DTYPE_SIZE[want.dt] == 1 else 512 * 1024), (tag, info.table_bytes)
    else:
        assert info.table_bytes == 0, tag
