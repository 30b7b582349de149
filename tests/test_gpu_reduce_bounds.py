"""Where rsx_sort_reduce_device writes: every route once at 256-byte aligned and once at element-aligned-only residues, with keys,
values and all five outputs between guard bands (tests/guard_lib.py).  Each case asserts the outputs against the oracle, the route
it was written for, that keys and values hold what they held (they are const) and that both bands of every buffer are intact
afterwards: the vector loads of keys and values that start at different residues, the compacted stores of the read-out and the
stores of the runs and seams kernels are what these cases are for."""
import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa
import reduce_lib as rl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 1 << 20
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def residues(aligned, kb, vb, ib):
    """(keys, vals, out keys, counts, sum, min, max) residues mod 256: all aligned, or one element / 64 bytes + one element off --
    keys and values at DIFFERENT distances from a 16-byte boundary"""
    return (0,) * 7 if aligned else (kb, 64 + 3 * vb if vb == 4 else 64 + vb, 64 + kb, ib, 128 + 8, vb, 192 + vb)


def reduce_guarded(k, dt, v, vdt, order, ib, aligned, route, what):
    kb, vb = ol.DTYPE_SIZE[dt], ol.DTYPE_SIZE[vdt]
    k = np.ascontiguousarray(k, dtype=ol.NP_BITS[dt])
    v = np.ascontiguousarray(v, dtype=ol.NP_BITS[vdt])
    want = rl.want_reduce(rl.groups(k, dt, order), v, vdt)
    res = residues(aligned, kb, vb, ib)
    n = k.size
    keys, vals = gl.guarded(n, _T[kb], res[0], GUARD), gl.guarded(n, _T[vb], res[1], GUARD)
    keys.load(k)
    vals.load(v)
    okeys, cnt = gl.guarded(n, _T[kb], res[2], GUARD), gl.guarded(n, _T[ib], res[3], GUARD)
    sm = gl.guarded(n, torch.float64 if vdt in rl.FLOATS else torch.int64, res[4], GUARD)
    mn, mx = gl.guarded(n, _T[vb], res[5], GUARD), gl.guarded(n, _T[vb], res[6], GUARD)
    out = rsa.radix_sort_reduce(keys.t, vals.t, dtype=dt, val_dtype=vdt, order=order, idx_dtype=_T[ib], sum=sm.t, min=mn.t, max=mx.t,
                                counts=cnt.t, keys_out=okeys.t)
    torch.cuda.synchronize()
    tag = "%s (%s)" % (what, "aligned" if aligned else "element-aligned")
    info = out[5]
    assert info.route == route, (tag, info.route)
    assert np.array_equal(keys.t.cpu().numpy().view(ol.NP_BITS[dt]), k), tag + ": keys were written"
    assert np.array_equal(vals.t.cpu().numpy().view(ol.NP_BITS[vdt]), v), tag + ": values were written"
    views = (ol.NP_BITS[dt], np.uint32 if ib == 4 else np.uint64, np.uint64, ol.NP_BITS[vdt], ol.NP_BITS[vdt])
    for name, t, w, view in zip(("keys", "counts", "sum", "min", "max"), out[:5], want, views):
        g = t.cpu().numpy().view(view)
        assert np.array_equal(g.astype(np.uint64) if name == "counts" else g, w), "%s: %s differs from the oracle" % (tag, name)
    gl.check_all((tag + " keys", keys), (tag + " vals", vals), (tag + " out keys", okeys), (tag + " counts", cnt), (tag + " sum", sm),
                 (tag + " min", mn), (tag + " max", mx))
    return info


N = (1 << 19) + 3


@pytest.mark.parametrize("aligned", [True, False])
def test_trivial(aligned):
    a = np.full(3 * 8192 + 5, 0x01020304, dtype=np.uint32)
    reduce_guarded(a, ol.U32, rl.small_ints(a.size, ol.F32, 9501), ol.F32, ol.ASC, 8, aligned, rsa.REDUCE_TRIVIAL, "all equal")
    reduce_guarded(a[:1], ol.U32, rl.small_ints(1, ol.I64, 9502), ol.I64, ol.ASC, 4, aligned, rsa.REDUCE_TRIVIAL, "one key")


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt,mask,vdt", [(ol.U32, 0x00F0F00F, ol.F32), (ol.U8, 0xFF, ol.U64), (ol.U64, 0xFFF, ol.I32), (ol.U16, 0x0FF0, ol.F64)])
def test_cells_lds(dt, mask, vdt, aligned):
    a = ol.splitmix_fill(N, dt, 9503, mask)
    v = rl.small_ints(N, vdt, 9504)
    reduce_guarded(a, dt, v, vdt, ol.ASC, 4, aligned, rsa.REDUCE_CELLS_LDS, "LDS cells, mask %#x" % mask)
    reduce_guarded(a[:77], dt, v[:77], vdt, ol.DESC, 8, aligned, rsa.REDUCE_CELLS_LDS, "LDS cells, 77 keys")


@pytest.mark.parametrize("aligned", [True, False])
def test_cells_global(aligned, monkeypatch):
    monkeypatch.setenv("RSX_REDUCE_MAX_BITS", "16")      # (the route is off by default)
    rsa.reload_env()
    a = ol.splitmix_fill(N, ol.U32, 9505, 0x00F0FF0F)
    reduce_guarded(a, ol.U32, rl.small_ints(N, ol.F64, 9506), ol.F64, ol.ASC, 4, aligned, rsa.REDUCE_CELLS_GLOBAL, "cells in device memory")
    b = ol.splitmix_fill(N, ol.U64, 9507, 0x1FFF00000)
    reduce_guarded(b, ol.I64, rl.small_ints(N, ol.U32, 9508), ol.U32, ol.DESC, 8, aligned, rsa.REDUCE_CELLS_GLOBAL, "cells in device memory, i64")


@pytest.mark.parametrize("aligned", [True, False])
def test_sort_route(aligned):
    a = ol.splitmix_fill(300001, ol.F32, 9509, 0xFFF000FF)
    reduce_guarded(a, ol.F32, rl.small_ints(a.size, ol.F32, 9510), ol.F32, ol.ASC, 8, aligned, rsa.REDUCE_SORT, "f32 mixed signs")
    reduce_guarded(a[:1000], ol.F32, rl.small_ints(1000, ol.I64, 9511), ol.I64, ol.DESC, 4, aligned, rsa.REDUCE_SORT, "1000 keys")
    b = np.sort(ol.splitmix_fill((1 << 18) + 9, ol.U32, 9512, 0x000FFFFF))
    info = reduce_guarded(b, ol.U32, rl.small_ints(b.size, ol.U64, 9513), ol.U64, ol.ASC, 4, aligned, rsa.REDUCE_SORT, "sorted input: no sort")
    assert info.sort.early_exit == 2
    d = ol.splitmix_fill((1 << 18) + 5, ol.U64, 9514, 0xFFFFFFFFFF)
    reduce_guarded(d, ol.U64, rl.small_ints(d.size, ol.I32, 9515), ol.I32, ol.ASC, 4, aligned, rsa.REDUCE_SORT, "u64 below 2^40")
