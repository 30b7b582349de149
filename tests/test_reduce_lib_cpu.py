"""tests/reduce_lib.py against a plain dict loop: the groups, the wrapping integer sums, the fsum float sums and the min / max by the
value's derived key, for every value type, both orders, float keys with both zeros, and values with NaNs and infinities."""
import math
import struct

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa
import reduce_lib as rl


def test_the_helper_speaks_of_the_library_it_checks():
    assert (rl.SUM, rl.MIN, rl.MAX) == (rsa.REDUCE_SUM, rsa.REDUCE_MIN, rsa.REDUCE_MAX)
    assert rl.VAL_DTYPES == (rsa.U32, rsa.I32, rsa.F32, rsa.U64, rsa.I64, rsa.F64)
    assert all(hasattr(rsa.lib(), name) for name in ("rsx_sort_reduce", "rsx_sort_reduce_device"))


def _dict_loop(kbits, dt, vbits, vdt, order):
    kk = ol.kdf_keys(kbits, dt, order)
    kv = ol.kdf_keys(vbits, vdt, ol.ASC)
    g = {}
    for i in range(kbits.size):
        e = g.setdefault(int(kk[i]), [int(kbits[i]), 0, [], i, i])
        e[1] += 1
        e[2].append(i)
        if int(kv[i]) < int(kv[e[3]]):
            e[3] = i
        if int(kv[i]) > int(kv[e[4]]):
            e[4] = i
    out = []
    for k in sorted(g):
        key, cnt, idx, lo, hi = g[k]
        if vdt in rl.FLOATS:
            fmt = "<f" if vdt == ol.F32 else "<d"
            width = "<I" if vdt == ol.F32 else "<Q"
            s = math.fsum(struct.unpack(fmt, struct.pack(width, int(vbits[i])))[0] for i in idx)
            sbits = struct.unpack("<Q", struct.pack("<d", s))[0]
        else:
            s = 0
            for i in idx:
                x = int(vbits[i])
                if vdt == ol.I32 and x >= 1 << 31:
                    x -= 1 << 32
                s += x
            sbits = s % (1 << 64)
        out.append((key, cnt, sbits, int(vbits[lo]), int(vbits[hi])))
    return out


@pytest.mark.parametrize("vdt", rl.VAL_DTYPES)
@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
def test_against_a_dict_loop(vdt, order):
    rng = np.random.default_rng(100 + vdt)
    for dt, mask in ((ol.U32, 0x00F0F00F), (ol.I8, 0xFF), (ol.F32, 0x80000003), (ol.U64, 0xFFFFFFFFFF)):
        n = 3001
        kbits = ol.splitmix_fill(n, dt, 7 + dt, mask)
        kbits[:40] = kbits[0]
        if vdt in rl.FLOATS:
            vbits = rl.small_ints(n, vdt, 9 + dt)
            vbits[::7] = np.ascontiguousarray((rng.standard_normal(vbits[::7].size) * 1e3).astype(np.float32 if vdt == ol.F32 else np.float64)).view(ol.NP_BITS[vdt])
        else:
            vbits = ol.splitmix_fill(n, vdt, 11 + dt)           # full-range: the sums wrap
        grp = rl.groups(kbits, dt, order)
        keys, counts, total, lo, hi = rl.want_reduce(grp, vbits, vdt)
        want = _dict_loop(kbits, dt, vbits, vdt, order)
        assert keys.size == len(want) == counts.size
        got = list(zip(map(int, keys), map(int, counts), map(int, total), map(int, lo), map(int, hi)))
        assert got == want


def test_min_max_of_special_floats_by_bit_pattern():
    for vdt, w in ((ol.F32, np.float32), (ol.F64, np.float64)):
        vals = np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -2.5], dtype=w).view(ol.NP_BITS[vdt]).copy()
        nb = ol.DTYPE_SIZE[vdt] * 8
        qnan = (0x7FC00000 if vdt == ol.F32 else 0x7FF8000000000000)
        vals = np.r_[vals, np.array([qnan, qnan | (1 << (nb - 1))], dtype=ol.NP_BITS[vdt])]
        keys = np.zeros(vals.size, dtype=np.uint32)
        grp = rl.groups(keys, ol.U32)
        _, counts, total, lo, hi = rl.want_reduce(grp, vals, vdt, float_sums=False)
        assert total is None and int(counts[0]) == vals.size
        assert int(lo[0]) == qnan | (1 << (nb - 1)) and int(hi[0]) == qnan      # -NaN below -inf, +NaN above +inf
        _, _, _, lo, hi = rl.want_reduce(rl.groups(keys[:2], ol.U32), vals[:2], vdt)
        assert int(lo[0]) == 1 << (nb - 1) and int(hi[0]) == 0                  # -0.0 < +0.0


def test_small_ints_are_exact_in_any_order():
    for vdt in rl.VAL_DTYPES:
        v = rl.small_ints(1000, vdt, 3)
        f = rl.as_f64(v, vdt) if vdt in rl.FLOATS else None
        if f is not None:
            assert np.all(f == np.round(f)) and np.abs(f).max() < 2 ** 24
            assert math.fsum(f) == float(np.sum(f[::-1]))


def test_fsum_bound_is_the_issues():
    kbits = np.zeros(5, dtype=np.uint32)
    v = np.array([1.0, -2.0, 4.0, 8.0, -16.0], dtype=np.float64).view(np.uint64)
    b = rl.fsum_bound(rl.groups(kbits, ol.U32), v, ol.F64)
    u = 2.0 ** -53
    assert b.size == 1 and b[0] == (4 * u / (1 - 4 * u)) * 31.0
