"""Shared by tests/test_gpu_unique.py and tests/test_gpu_unique_bounds.py: the expected distinct keys from the ORACLE's sort
(never from the code under test), and the bit tricks the route tests build their inputs with.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle_lib as ol

SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def want_unique(bits, dt, order=ol.ASC):
    """(distinct keys in KDF order, their counts) read off the oracle's sorted array: heads are s[i] != s[i-1] on bit patterns,
    counts the differences of the head positions."""
    s = ol.oracle_sort(bits, dt, order)[0]
    if s.size == 0:
        return s, np.zeros(0, dtype=np.uint64)
    head = np.r_[True, s[1:] != s[:-1]]
    pos = np.flatnonzero(head)
    return s[head].copy(), np.diff(np.r_[pos, s.size]).astype(np.uint64)


def deposit(packed, mask):
    """The inverse of the library's key compaction: bit j of `packed` goes to the j-th lowest set bit of `mask`."""
    packed = np.asarray(packed, dtype=np.uint64)
    out = np.zeros_like(packed)
    j = 0
    for b in range(64):
        if (mask >> b) & 1:
            out |= ((packed >> np.uint64(j)) & np.uint64(1)) << np.uint64(b)
            j += 1
    return out


def strictly_ascending_by_kdf(bits, dt, order=ol.ASC):
    k = ol.kdf_keys(bits, dt, order)
    return bool(np.all(k[1:] > k[:-1]))
