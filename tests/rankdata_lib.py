"""Shared by the radix_sort_rankdata tests: every expected value from the ORACLE side (never from the code under test).  The
place is the oracle-side stable argsort inverted, less and equal are two searches of the sorted derived keys.  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

import oracle_lib as ol


def want_rankdata(bits, dt, order=ol.ASC):
    """(place, less, equal), all uint64 and 0-based: place[i] = where element i stands in the stable sorted order, less[i] = how
    many derived keys are below element i's, equal[i] = how many equal it (itself included)."""
    bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    n = bits.size
    if n == 0:
        z = np.zeros(0, dtype=np.uint64)
        return z, z.copy(), z.copy()
    perm = np.asarray(ol.stable_argsort_by_kdf(bits, dt, order)).astype(np.int64)
    place = np.empty(n, dtype=np.uint64)
    place[perm] = np.arange(n, dtype=np.uint64)
    k = ol.kdf_keys(bits, dt, order)
    ks = np.sort(k, kind="stable")
    lo = np.searchsorted(ks, k, side="left")
    hi = np.searchsorted(ks, k, side="right")
    return place, lo.astype(np.uint64), (hi - lo).astype(np.uint64)


def by_method(place, less, equal, method):
    """The 0-based rank of a tie method from the three arrays (float64 for "average")."""
    if method == "ordinal":
        return place
    if method == "min":
        return less
    if method == "max":
        return less + equal - np.uint64(1)
    if method == "average":
        return less.astype(np.float64) + (equal.astype(np.float64) - 1.0) / 2.0
    raise ValueError(method)
