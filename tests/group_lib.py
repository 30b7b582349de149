"""Shared by the radix_sort_group tests: every expected value from the ORACLE (never from the code under test).  Keys and counts
are unique_lib.want_unique's (the oracle's sorted array), the inverse is each key's place among them by derived key, the first
indices are the oracle-side stable argsort read at the head positions.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import oracle_lib as ol
import unique_lib as ul


def want_group(bits, dt, order=ol.ASC):
    """(inverse, keys, counts, first), all uint64 but the keys (bit patterns)."""
    bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    keys, counts = ul.want_unique(bits, dt, order)
    if bits.size == 0:
        z = np.zeros(0, dtype=np.uint64)
        return z, keys, counts, z
    inverse = np.searchsorted(ol.kdf_keys(keys, dt, order), ol.kdf_keys(bits, dt, order)).astype(np.uint64)
    perm = ol.stable_argsort_by_kdf(bits, dt, order)
    heads = np.r_[0, np.cumsum(counts)[:-1]].astype(np.int64)
    first = perm[heads].astype(np.uint64)
    return inverse, keys, counts, first
