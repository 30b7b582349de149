"""Shared by tests/test_gpu_nth.py and tests/test_gpu_nth_bounds.py: what stands at given ranks of the sorted order, from the
ORACLE's stable ranks (never from the code under test), the course the select route has to take on those keys counted from
the oracle's sorted keys, and one way to call rsx_sort_nth_device.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import radix_sorting_amd as rsa


def tile(kb):
    """Elements of one tile of the select kernels: NTH_ITER (4) sweeps of NTH_THREADS (512) threads x one 16-byte vector
    (radix_sorting_amd/csrc/rsx_nth.hpp, `enum : u32 { NTH_THREADS = 512, NTH_ITER = 4, ...` and nth_tile())."""
    return 4 * 512 * (16 // kb)


def capacity(n):
    """The candidate buffer's capacity (radix_sorting_amd/csrc/rsx_nth_api.hpp, nth_cap): active buckets that together hold more stay
    in the input for another digit."""
    return n // 8 + 1024


class Course:
    """What the select route does for one rank list (rsx_nth_info of a forced select)."""

    def __init__(self, digit_passes, active_buckets, from_prefix, candidates, falls_to_sort):
        self.digit_passes, self.active_buckets = digit_passes, active_buckets
        self.from_prefix, self.candidates, self.falls_to_sort = from_prefix, candidates, falls_to_sort


class Want:
    """What the oracle says about the keys `bits`: its stable ranks, and from them everything an nth call reports."""

    def __init__(self, bits, dt, order=ol.ASC):
        self.bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
        self.dt, self.order = dt, order
        self.ranks = ol.oracle_rank(self.bits, dt, 4, order)[0].astype(np.uint64)
        self.sorted = self.bits[self.ranks]                      # the oracle's sorted array
        self.kd = ol.kdf_keys(self.sorted, dt, order)            # ... its derived keys, ascending

    def at(self, ranks):
        """(keys, indices, n_less, n_equal) at the positions `ranks` of the sorted order, in the order of `ranks`"""
        r = np.asarray(ranks, dtype=np.uint64)
        idx = self.ranks[r]
        kd = self.kd[r]
        lo = np.searchsorted(self.kd, kd, side="left").astype(np.uint64)
        hi = np.searchsorted(self.kd, kd, side="right").astype(np.uint64)
        return self.bits[idx], idx, lo, hi - lo

    def course(self, ranks, want_idx):
        """The rule of DESIGN.md 4k counted on the oracle's sorted derived keys: level by level (8 bits, most significant
        first) the buckets that hold a wanted rank; the first level at which they together hold at most capacity(n) elements
        moves them to the candidates.  After the last digit nothing is moved unless indices are wanted and the buckets fit;
        buckets that do not fit then cannot give indices (the call falls to the sort route)."""
        kb = ol.DTYPE_SIZE[self.dt]
        n = self.bits.size
        want = np.unique(np.asarray(ranks, dtype=np.uint64))
        kd = self.kd.astype(np.uint64)
        for level in range(1, kb + 1):
            shift = np.uint64(8 * (kb - level))
            prefixes = kd >> shift                                # (ascending, as kd is)
            active = np.unique(prefixes[want])
            total = int((np.searchsorted(prefixes, active, side="right") - np.searchsorted(prefixes, active, side="left")).sum())
            if level < kb and total <= capacity(n):
                return Course(level, active.size, 0, total, False)
        if want_idx and total <= capacity(n):
            return Course(kb, active.size, 0, total, False)
        return Course(kb, active.size, 1, 0, want_idx)


def call_device(src_t, n, ranks, dt, order, idx_bytes, keys_t=None, idx_t=None, stream=None, host_arrays=(True, True)):
    """rsx_sort_nth_device on device tensors (None: that output is not asked for).  Returns (rc, info, n_less, n_equal); the
    host arrays are prefilled with 0xA5 bytes (host_arrays: which of the two are passed at all)."""
    import torch
    info = rsa.NthInfo()
    s = stream if stream is not None else torch.cuda.current_stream()
    r = np.ascontiguousarray(ranks, dtype=np.uint64)
    n_less = np.full(r.size, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    n_equal = np.full(r.size, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    p64 = C.POINTER(C.c_uint64)
    rc = rsa.lib().rsx_sort_nth_device(src_t.data_ptr(), n, r.ctypes.data_as(p64), r.size, dt, order,
                                       None if keys_t is None else keys_t.data_ptr(), None if idx_t is None else idx_t.data_ptr(),
                                       idx_bytes, n_less.ctypes.data_as(p64) if host_arrays[0] else None,
                                       n_equal.ctypes.data_as(p64) if host_arrays[1] else None, C.c_void_p(s.cuda_stream),
                                       C.byref(info))
    return rc, info, n_less, n_equal


def check(tag, want, ranks, keys_t, idx_t, n_less, n_equal, info, route=None, host_arrays=(True, True)):
    """The outputs (device tensors / numpy arrays of exactly m elements, or None) and the host arrays against the oracle."""
    wkeys, widx, wless, wequal = want.at(ranks)
    m = len(ranks)
    if keys_t is not None:
        got = (keys_t.cpu().numpy() if hasattr(keys_t, "cpu") else keys_t).view(ol.NP_BITS[want.dt])
        assert got.size == m and np.array_equal(got, wkeys), (tag, "keys")
    if idx_t is not None:
        got = idx_t.cpu().numpy() if hasattr(idx_t, "cpu") else idx_t
        got = got.view(np.uint32 if got.itemsize == 4 else np.uint64).astype(np.uint64)
        assert got.size == m and np.array_equal(got, widx), (tag, "indices")
    if host_arrays[0]:
        assert np.array_equal(n_less, wless), (tag, "n_less", n_less[:8], wless[:8])
    else:
        assert (n_less == 0xA5A5A5A5A5A5A5A5).all(), (tag, "n_less was not passed but written")
    if host_arrays[1]:
        assert np.array_equal(n_equal, wequal), (tag, "n_equal", n_equal[:8], wequal[:8])
    else:
        assert (n_equal == 0xA5A5A5A5A5A5A5A5).all(), (tag, "n_equal was not passed but written")
    if route is not None:
        assert info.route == route, (tag, "route", info.route)
    kb = ol.DTYPE_SIZE[want.dt]
    assert info.key_bytes == kb, tag
    if info.route == rsa.NTH_SELECT:
        # the documented bound (include/rsx.h) and what the fields mean
        assert 1 <= info.digit_passes <= kb and info.input_reads <= kb + 2, (tag, info.digit_passes, info.input_reads)
        assert info.input_reads == info.digit_passes + (0 if info.from_prefix else 2), (tag, info.input_reads, info.digit_passes)
        assert 1 <= info.active_buckets <= min(len(set(int(r) for r in ranks)), rsa.NTH_MAX_SELECT_RANKS), (tag, info.active_buckets)
        assert (info.candidates == 0) == (info.from_prefix == 1) and info.candidates <= capacity(want.bits.size), tag
    else:
        assert (info.input_reads, info.digit_passes, info.active_buckets, info.from_prefix, info.candidates) == (0, 0, 0, 0, 0), tag


def check_course(tag, want, ranks, want_idx, info):
    """A forced select against the course counted from the oracle's keys (also: that it gave up where it has to)."""
    c = want.course(ranks, want_idx)
    if c.falls_to_sort:
        assert info.route == rsa.NTH_SORT, (tag, "a key too frequent for the candidates, with indices wanted: the sort route")
        return c
    assert info.route == rsa.NTH_SELECT, (tag, info.route)
    got = (info.digit_passes, info.active_buckets, info.from_prefix, info.candidates)
    assert got == (c.digit_passes, c.active_buckets, c.from_prefix, c.candidates), (tag, got, vars(c))
    return c
