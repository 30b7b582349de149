"""Shared by the radix_sort_reduce tests: every expected value from the ORACLE (never from the code under test).  The groups are
unique_lib.want_unique's (the oracle's sorted array) and each element's place among them by derived key; integer sums wrap
modulo 2^64 in numpy's uint64, float sums are math.fsum per group, min and max are the values at the arg-min / arg-max of
ol.kdf_keys(vals, val_dt, ASC) within the group.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

import oracle_lib as ol
import unique_lib as ul

VAL_DTYPES = (ol.U32, ol.I32, ol.F32, ol.U64, ol.I64, ol.F64)
FLOATS = (ol.F32, ol.F64)
SUM, MIN, MAX = 1, 2, 4


def groups(kbits, dt, order=ol.ASC):
    """(keys, counts, inverse): the distinct keys in KDF order, their sizes (uint64) and every element's group."""
    kbits = np.ascontiguousarray(kbits, dtype=ol.NP_BITS[dt])
    keys, counts = ul.want_unique(kbits, dt, order)
    if kbits.size == 0:
        return keys, counts, np.zeros(0, dtype=np.int64)
    inverse = np.searchsorted(ol.kdf_keys(keys, dt, order), ol.kdf_keys(kbits, dt, order)).astype(np.int64)
    return keys, counts, inverse


def as_f64(vbits, vdt):
    vbits = np.ascontiguousarray(vbits, dtype=ol.NP_BITS[vdt])
    return vbits.view(np.float32).astype(np.float64) if vdt == ol.F32 else vbits.view(np.float64)


def extended(vbits, vdt):
    """Integer values sign- or zero-extended to 64 bits, as uint64 bit patterns."""
    vbits = np.ascontiguousarray(vbits, dtype=ol.NP_BITS[vdt])
    if vdt == ol.I32:
        return vbits.view(np.int32).astype(np.int64).view(np.uint64)
    return vbits.astype(np.uint64)


def want_reduce(grp, vbits, vdt, float_sums=True):
    """(keys, counts, sum, min, max) for groups `grp` = groups(...): sum as uint64 bit patterns (of the u64 / i64 sum modulo
    2^64, or of the float64 math.fsum of the group; None where `float_sums` is off and the values are floats -- fsum refuses
    infinities of both signs), min / max as bit patterns of the value type."""
    keys, counts, inverse = grp
    vbits = np.ascontiguousarray(vbits, dtype=ol.NP_BITS[vdt])
    G = keys.size
    if G == 0:
        z = np.zeros(0, dtype=np.uint64)
        return keys, counts, z, vbits[:0], vbits[:0]
    starts = np.r_[0, np.cumsum(counts)[:-1]].astype(np.int64)
    by_group = np.argsort(inverse, kind="stable")
    if vdt in FLOATS:
        total = None
        if float_sums:
            f = as_f64(vbits, vdt)[by_group]
            ends = np.r_[starts[1:], f.size]
            total = f[starts] + 0.0                   # (a group of one: math.fsum([v]) is 0.0 + v; millions of them cost no loop)
            many = np.flatnonzero(ends - starts > 1)
            total[many] = [math.fsum(f[a:b]) for a, b in zip(starts[many], ends[many])]
            total = total.view(np.uint64)
    else:
        with np.errstate(over="ignore"):
            total = np.add.reduceat(extended(vbits, vdt)[by_group], starts).astype(np.uint64)
    kv = ol.kdf_keys(vbits, vdt, ol.ASC)
    by_value = np.lexsort((kv, inverse))          # by group, then by the value's derived key
    lo = vbits[by_value[starts]]
    hi = vbits[by_value[np.r_[starts[1:], vbits.size] - 1]]
    return keys, counts, total, lo, hi


def fsum_bound(grp, vbits, vdt):
    """Per group of c finite values the bound of the issue: recursive summation in any order is within
    ((c - 1) u / (1 - (c - 1) u)) * sum|v_i| of the exact sum (u = 2^-53), and math.fsum within u * |fsum| of it."""
    keys, counts, inverse = grp
    u = 2.0 ** -53
    starts = np.r_[0, np.cumsum(counts)[:-1]].astype(np.int64)
    a = np.abs(as_f64(vbits, vdt))[np.argsort(inverse, kind="stable")]
    sabs = np.array([math.fsum(a[s:e]) for s, e in zip(starts, np.r_[starts[1:], a.size])])
    c = counts.astype(np.float64)
    return ((c - 1) * u / (1 - (c - 1) * u)) * sabs


def small_ints(n, vdt, seed, bits=24):
    """Integers of magnitude below 2^bits in the value type's encoding (both signs where it has one): every partial sum of up
    to 2^21 of them is below 2^45, exact in f64 -- any order of additions gives the same bits."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-(1 << bits) + 1, 1 << bits, n)
    if vdt in (ol.U32, ol.U64):
        x = np.abs(x)
    np_t = {ol.U32: np.uint32, ol.I32: np.int32, ol.F32: np.float32, ol.U64: np.uint64, ol.I64: np.int64, ol.F64: np.float64}[vdt]
    return np.ascontiguousarray(x.astype(np_t)).view(ol.NP_BITS[vdt])
