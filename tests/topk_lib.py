"""Shared by tests/test_gpu_topk.py and tests/test_gpu_topk_bounds.py: the expected first k of the sorted order from the
ORACLE's stable ranks (never from the code under test), and one way to call rsx_sort_topk_device.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import radix_sorting_amd as rsa


def tile(kb):
    """Elements of one tile of the select kernels: TOPK_ITER (4) sweeps of TOPK_THREADS (512) threads x one 16-byte vector
    (radix_sorting_amd/csrc/rsx_topk.hpp, `enum : u32 { TOPK_THREADS = 512, TOPK_ITER = 4, ...` and topk_tile())."""
    return 4 * 512 * (16 // kb)


def capacity(n):
    """The candidate buffer's capacity (radix_sorting_amd/csrc/rsx_topk_api.hpp, topk_cap): a larger selected bucket stays in the input."""
    return n // 8 + 1024


class Want:
    """What the oracle says about the keys `bits`: its stable ranks, and from them everything a top-k call reports."""

    def __init__(self, bits, dt, order=ol.ASC):
        self.bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
        self.dt, self.order = dt, order
        self.ranks = ol.oracle_rank(self.bits, dt, 4, order)[0].astype(np.uint64)
        self.sorted = self.bits[self.ranks]                      # the oracle's sorted array
        self.kd = ol.kdf_keys(self.sorted, dt, order)            # ... its derived keys, ascending

    def first(self, k):
        """(keys, indices, kth_key, n_less, n_equal) of the first k"""
        idx = self.ranks[:k]
        keys = self.bits[idx]
        lo = int(np.searchsorted(self.kd, self.kd[k - 1], side="left"))
        hi = int(np.searchsorted(self.kd, self.kd[k - 1], side="right"))
        return keys, idx, int(self.sorted[k - 1]), lo, hi - lo


def call_device(src_t, n, k, dt, order, idx_bytes, keys_t=None, idx_t=None, stream=None):
    """rsx_sort_topk_device on device tensors (None: that output is not asked for).  Returns (rc, info)."""
    import torch
    info = rsa.TopkInfo()
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = rsa.lib().rsx_sort_topk_device(src_t.data_ptr(), n, k, dt, order, None if keys_t is None else keys_t.data_ptr(),
                                        None if idx_t is None else idx_t.data_ptr(), idx_bytes, C.c_void_p(s.cuda_stream),
                                        C.byref(info))
    return rc, info


def check(tag, want, k, keys_t, idx_t, info, route=None):
    """The outputs (device tensors of exactly k elements, or None) and the info fields against the oracle."""
    wkeys, widx, wkth, wless, wequal = want.first(k)
    if keys_t is not None:
        got = keys_t.cpu().numpy().view(ol.NP_BITS[want.dt])
        assert got.size == k and np.array_equal(got, wkeys), (tag, "keys")
    if idx_t is not None:
        got = idx_t.cpu().numpy()
        got = got.view(np.uint32 if got.itemsize == 4 else np.uint64).astype(np.uint64)
        assert got.size == k and np.array_equal(got, widx), (tag, "indices")
    if route is not None:
        assert info.route == route, (tag, "route", info.route)
    assert info.key_bytes == ol.DTYPE_SIZE[want.dt], tag
    assert (info.kth_key, info.n_less, info.n_equal) == (wkth, wless, wequal), \
        (tag, (info.kth_key, info.n_less, info.n_equal), (wkth, wless, wequal))
    assert info.n_less < k <= info.n_less + info.n_equal, tag
    if info.route == rsa.TOPK_SELECT:
        kb = ol.DTYPE_SIZE[want.dt]
        assert 1 <= info.input_reads <= kb + 1 and info.digit_passes == kb, (tag, info.input_reads, info.digit_passes)
    else:
        assert info.input_reads == 0 and info.digit_passes == 0, tag
