"""Where rsx_sort_group_device writes: every route once at 256-byte aligned and once at element-aligned-only residues, with src
and all four outputs between guard bands (tests/guard_lib.py).  Each case asserts the outputs against the oracle, the route it
was written for, that src holds what it held (it is const) and that both bands of every buffer are intact afterwards: the
scatter of the sort route and the vector stores of the lookup kernel are what these cases are for."""
import numpy as np
import pytest

import group_lib as gr
import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa

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


def residues(aligned, kb, ib):
    """(src, inverse, keys, counts, first) residues mod 256: all aligned, or one element / 64 bytes + one element off"""
    return (0, 0, 0, 0, 0) if aligned else (kb, 64 + ib, 64 + kb, ib, 128 + ib)


def group_guarded(a, dt, order, ib, aligned, route, what, counts=True, first=True):
    kb = ol.DTYPE_SIZE[dt]
    a = np.ascontiguousarray(a, dtype=ol.NP_BITS[dt])
    want = gr.want_group(a, dt, order)
    rs, ri, rk, rc, rf = residues(aligned, kb, ib)
    src = gl.guarded(a.size, _T[kb], rs, GUARD)
    src.load(a)
    inv = gl.guarded(a.size, _T[ib], ri, GUARD)
    keys = gl.guarded(a.size, _T[kb], rk, GUARD)
    cnt = gl.guarded(a.size, _T[ib], rc, GUARD) if counts else None
    fst = gl.guarded(a.size, _T[ib], rf, GUARD) if first else None
    out = rsa.radix_sort_group(src.t, dtype=dt, order=order, idx_dtype=_T[ib], inverse=inv.t, keys=keys.t,
                               counts=cnt.t if counts else False, first=fst.t if first else False)
    torch.cuda.synchronize()
    tag = "%s (%s)" % (what, "aligned" if aligned else "element-aligned")
    info = out[4]
    assert info.route == route, (tag, info.route)
    assert np.array_equal(src.t.cpu().numpy().view(ol.NP_BITS[dt]), a), tag + ": src was written"
    idt = np.uint32 if ib == 4 else np.uint64
    for name, t, w in zip(("inverse", "keys", "counts", "first"), out[:4], want):
        if t is None:
            continue
        g = t.cpu().numpy()
        g = g.view(ol.NP_BITS[dt]) if name == "keys" else g.view(idt).astype(np.uint64)
        assert np.array_equal(g, w), "%s: %s differs from the oracle" % (tag, name)
    pairs = [(tag + " src", src), (tag + " inverse", inv), (tag + " keys", keys)]
    pairs += [(tag + " counts", cnt)] if counts else []
    pairs += [(tag + " first", fst)] if first else []
    gl.check_all(*pairs)
    return info


@pytest.mark.parametrize("aligned", [True, False])
def test_trivial(aligned):
    a = np.full(70001, 0x01020304, dtype=np.uint32)
    group_guarded(a, ol.U32, ol.ASC, 8, aligned, rsa.GROUP_TRIVIAL, "all equal")
    group_guarded(a[:1], ol.U32, ol.ASC, 4, aligned, rsa.GROUP_TRIVIAL, "one key")


@pytest.mark.parametrize("aligned", [True, False])
def test_table(aligned):
    a = ol.splitmix_fill((1 << 20) + 3, ol.U32, 9401, 0x00FF0000)
    group_guarded(a, ol.U32, ol.ASC, 4, aligned, rsa.GROUP_TABLE, "one kept column", first=False)
    b = ol.splitmix_fill((1 << 20) + 7, ol.U8, 9402)
    group_guarded(b, ol.I8, ol.DESC, 8, aligned, rsa.GROUP_TABLE, "1-byte keys", first=False)
    group_guarded(b, ol.U8, ol.ASC, 4, aligned, rsa.GROUP_TABLE, "1-byte keys, 4-byte indices", first=False)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt,mask", [(ol.U32, 0x00F0FF0F), (ol.U64, 0x3FFFF), (ol.U16, 0xFFFF)])
def test_rank_lds(dt, mask, aligned):
    a = ol.splitmix_fill((1 << 20) + 3, dt, 9403, mask)
    for ib in (4, 8):
        group_guarded(a, dt, ol.ASC, ib, aligned, rsa.GROUP_RANK_LDS, "LDS cells, mask %#x, ib %d" % (mask, ib), counts=False, first=False)
    group_guarded(a[:77], dt, ol.DESC, 4, aligned, rsa.GROUP_RANK_LDS, "LDS cells, 77 keys", counts=False, first=False)


@pytest.mark.parametrize("aligned", [True, False])
def test_rank_global(aligned):
    a = ol.splitmix_fill((1 << 21) + 5, ol.U32, 9404, 0x00FFFFFF)
    group_guarded(a, ol.U32, ol.ASC, 4, aligned, rsa.GROUP_RANK_GLOBAL, "cells in device memory", counts=False, first=False)
    b = ol.splitmix_fill((1 << 21) + 1, ol.U64, 9405, 0x3FFFFF00000)
    group_guarded(b, ol.I64, ol.DESC, 8, aligned, rsa.GROUP_RANK_GLOBAL, "cells in device memory, i64", counts=False, first=False)


@pytest.mark.parametrize("aligned", [True, False])
def test_sort_route(aligned, monkeypatch):
    a = ol.splitmix_fill(300001, ol.F32, 9406, 0xFFF000FF)
    group_guarded(a, ol.F32, ol.ASC, 8, aligned, rsa.GROUP_SORT, "f32 mixed signs")
    group_guarded(a[:1000], ol.F32, ol.DESC, 4, aligned, rsa.GROUP_SORT, "1000 keys")
    b = np.sort(ol.splitmix_fill((1 << 20) + 9, ol.U32, 9407, 0x000FFFFF))
    info = group_guarded(b, ol.U32, ol.ASC, 4, aligned, rsa.GROUP_SORT, "sorted input: heads only")
    assert info.sort.early_exit == 2
    c = ol.splitmix_fill((1 << 20) + 3, ol.U16, 9408)
    group_guarded(c, ol.U16, ol.ASC, 4, aligned, rsa.GROUP_SORT, "u16 + first")
    d = ol.splitmix_fill((1 << 20) + 5, ol.U64, 9409, 0xFFFFFFFFFF)
    group_guarded(d, ol.U64, ol.ASC, 4, aligned, rsa.GROUP_SORT, "u64 below 2^40")
    monkeypatch.setenv("RSX_GROUP_MAX_BITS", "0")
    e = ol.splitmix_fill((1 << 20) + 11, ol.U8, 9410)
    group_guarded(e, ol.U8, ol.ASC, 4, aligned, rsa.GROUP_SORT, "u8, MAX_BITS=0", counts=False, first=False)
    f = ol.splitmix_fill((1 << 20) + 3, ol.U32, 9411, 0x00F0FF0F)
    group_guarded(f, ol.U32, ol.ASC, 4, aligned, rsa.GROUP_SORT, "u32 bitmap input, MAX_BITS=0", counts=False, first=False)
