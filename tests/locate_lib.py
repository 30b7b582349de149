"""Shared by tests/test_gpu_locate.py, tests/test_gpu_locate_bounds.py and tests/test_locate_lib_cpu.py: where given values fall in
the sorted order of the keys, from NumPy on the ORACLE's derived keys (never from the code under test) -- np.sort and
np.searchsorted left / right over ol.kdf_keys of keys and values --, the search route's shape restated from
radix_sorting_amd/csrc/rsx_locate_shape.hpp, and one way to call rsx_sort_locate_device.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import radix_sorting_amd as rsa

TILE = rsa.LOCATE_TILE                          # keys of one tile of the search kernel
SHARE = rsa.LOCATE_SHARE_TILES * rsa.LOCATE_TILE    # keys of the smallest share of a workgroup


class Want:
    """What NumPy says about the keys `bits`: their derived keys, sorted once and shared by every list of values."""

    def __init__(self, bits, dt, order=ol.ASC):
        self.bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
        self.dt, self.order = dt, order
        self.kd = ol.kdf_keys(self.bits, dt, order)
        self.sorted = np.sort(self.kd)

    def at(self, vals):
        """(less, equal) of every value, uint64"""
        kv = ol.kdf_keys(np.ascontiguousarray(vals, dtype=ol.NP_BITS[self.dt]), self.dt, self.order)
        lo = np.searchsorted(self.sorted, kv, side="left").astype(np.uint64)
        hi = np.searchsorted(self.sorted, kv, side="right").astype(np.uint64)
        return lo, hi - lo

    def bins(self, vals, below):
        """the bin of every key, uint64: the values at or below it (below: strictly below it)"""
        kv = np.sort(ol.kdf_keys(np.ascontiguousarray(vals, dtype=ol.NP_BITS[self.dt]), self.dt, self.order))
        return np.searchsorted(kv, self.kd, side="left" if below else "right").astype(np.uint64)


def from_kdf(kd, dt, order=ol.ASC):
    """The bit patterns whose derived keys are `kd`: the inverse of ol.kdf_keys."""
    t = ol.NP_BITS[dt]
    k = np.asarray(kd, dtype=t)
    nb = ol.DTYPE_SIZE[dt] * 8
    top = t(1 << (nb - 1))
    if order == ol.DESC:
        k = ~k
    if dt in (ol.I8, ol.I16, ol.I32, ol.I64):
        return (k ^ top).astype(t)
    if dt in (ol.F32, ol.F64):
        positive = (k >> t(nb - 1)).astype(bool)          # the derived keys of non-negative floats have the top bit set
        return np.where(positive, k ^ top, ~k).astype(t)
    return k.astype(t)


def search_shape(vals, dt, order=ol.ASC):
    """(D, shift, search_steps) of the values by rsx_locate_shape.hpp's rule: the digit is the eight bits behind the leading bits
    the first and the last edge share (locate_shift); the spans are counted over all edges but the last (locate_start_entry);
    search_steps is the smallest s with 2^s > the largest span (locate_steps)."""
    edges = np.unique(ol.kdf_keys(np.ascontiguousarray(vals, dtype=ol.NP_BITS[dt]), dt, order))
    x = int(edges[0]) ^ int(edges[-1])
    shift = max(x.bit_length() - 8, 0)
    digits = [(int(e) >> shift) & 0xFF for e in edges[:-1]]
    span = max(np.bincount(digits, minlength=256)) if digits else 0
    return edges.size, shift, int(span).bit_length()


def call_device(src_t, n, vals_t, m, dt, order, idx_bytes, less_t=None, equal_t=None, bin_t=None, flags=0, stream=None):
    """rsx_sort_locate_device on device tensors (None: that output is not asked for).  Returns (rc, info)."""
    import torch
    info = rsa.LocateInfo()
    s = stream if stream is not None else torch.cuda.current_stream()
    p = lambda t: None if t is None else t.data_ptr()
    rc = rsa.lib().rsx_sort_locate_device(p(src_t), n, p(vals_t), m, dt, order, p(less_t), p(equal_t), p(bin_t), idx_bytes, flags,
                                          C.c_void_p(s.cuda_stream), C.byref(info))
    return rc, info


def _host(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64).astype(np.uint64)


def check(tag, want, vals, src_t, vals_t, less_t, equal_t, bin_t, below, info, route=None):
    """The outputs (device tensors / numpy arrays of exactly m resp. n elements, or None) against NumPy; src and vals unchanged."""
    vals = np.ascontiguousarray(vals, dtype=ol.NP_BITS[want.dt])
    m, n = vals.size, want.bits.size
    if less_t is not None or equal_t is not None:
        wless, wequal = want.at(vals)
        if less_t is not None:
            got = _host(less_t)
            assert got.size == m and np.array_equal(got, wless), (tag, "less", got[:8], wless[:8])
        if equal_t is not None:
            got = _host(equal_t)
            assert got.size == m and np.array_equal(got, wequal), (tag, "equal", got[:8], wequal[:8])
    if bin_t is not None:
        got = _host(bin_t)
        wbin = want.bins(vals, below)
        assert got.size == n and np.array_equal(got, wbin), (tag, "bins", np.flatnonzero(got != wbin)[:8], got[:8], wbin[:8])
    if src_t is not None:
        assert np.array_equal(src_t.cpu().numpy().view(ol.NP_BITS[want.dt]), want.bits), (tag, "src was written")
    if vals_t is not None:
        assert np.array_equal(vals_t.cpu().numpy().view(ol.NP_BITS[want.dt]), vals), (tag, "vals was written")
    if route is not None:
        assert info.route == route, (tag, "route", info.route)
    assert info.key_bytes == ol.DTYPE_SIZE[want.dt], tag
    if info.route == rsa.LOCATE_SEARCH:
        d, _, steps = search_shape(vals, want.dt, want.order)
        assert info.input_reads == 1 and info.distinct_values == d and info.search_steps == steps, (tag, info.distinct_values, d, info.search_steps, steps)
        assert 0 <= info.search_steps <= 12 and 1 <= info.counter_sets <= 32, (tag, info.search_steps, info.counter_sets)
    elif info.route == rsa.LOCATE_TABLE:
        assert info.input_reads == (1 if less_t is not None or equal_t is not None else 0) + (1 if bin_t is not None else 0), (tag, info.input_reads)
    else:
        assert (info.input_reads, info.search_steps, info.counter_sets) == (0, 0, 0), tag
