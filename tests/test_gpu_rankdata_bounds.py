"""Where rsx_sort_rankdata_device writes: every route once at 256-byte aligned and once at element-aligned-only residues, with src
and the three outputs -- of exactly n entries each -- between guard bands (tests/guard_lib.py).  Each case asserts the outputs
against the oracle side, the route it was written for, that src holds what it held (it is const) and that both bands of every
buffer are intact afterwards: the vector stores of the lookup kernel, the last round of the place kernel and the scatter of the
sort route are what these cases are for."""
import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa
import rankdata_lib as rl
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 1 << 20
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
ALL, NO_PLACE, PLACE = (True, True, True), (False, True, True), (True, False, False)


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
    """(src, place, less, equal) residues mod 256: all aligned, or one element / 64 bytes + one element off"""
    return (0, 0, 0, 0) if aligned else (kb, 64 + ib, ib, 128 + ib)


def rankdata_guarded(a, dt, order, ib, aligned, route, tag, what=ALL):
    kb = ol.DTYPE_SIZE[dt]
    a = np.ascontiguousarray(a, dtype=ol.NP_BITS[dt])
    want = rl.want_rankdata(a, dt, order)
    res = residues(aligned, kb, ib)
    src = gl.guarded(a.size, _T[kb], res[0], GUARD)
    src.load(a)
    outs = [gl.guarded(a.size, _T[ib], r, GUARD) if w else None for w, r in zip(what, res[1:])]
    arg = [o.t if o is not None else False for o in outs]
    got = rsa.radix_sort_rankdata(src.t, dtype=dt, order=order, idx_dtype=_T[ib], place=arg[0], less=arg[1], equal=arg[2])
    torch.cuda.synchronize()
    tag = "%s (%s)" % (tag, "aligned" if aligned else "element-aligned")
    info = got[3]
    assert info.route == route, (tag, info.route)
    assert np.array_equal(src.t.cpu().numpy().view(ol.NP_BITS[dt]), a), tag + ": src was written"
    idt = np.uint32 if ib == 4 else np.uint64
    pairs = [(tag + " src", src)]
    for name, o, t, w in zip(("place", "less", "equal"), outs, got[:3], want):
        assert (t is None) == (o is None)
        if o is None:
            continue
        assert t.numel() == a.size
        assert np.array_equal(t.cpu().numpy().view(idt).astype(np.uint64), w), "%s: %s differs from the oracle" % (tag, name)
        pairs.append((tag + " " + name, o))
    gl.check_all(*pairs)
    return info


@pytest.mark.parametrize("aligned", [True, False])
def test_trivial(aligned):
    a = np.full(70001, 0x01020304, dtype=np.uint32)
    rankdata_guarded(a, ol.U32, ol.ASC, 8, aligned, rsa.RANKDATA_TRIVIAL, "all equal")
    rankdata_guarded(a, ol.U32, ol.ASC, 4, aligned, rsa.RANKDATA_TRIVIAL, "all equal, 4-byte indices")
    rankdata_guarded(a[:1], ol.U32, ol.ASC, 4, aligned, rsa.RANKDATA_TRIVIAL, "one key")


@pytest.mark.parametrize("aligned", [True, False])
def test_table(aligned):
    a = ol.splitmix_fill((1 << 20) + 3, ol.U32, 9501, 0x00FF0000)
    rankdata_guarded(a, ol.U32, ol.ASC, 4, aligned, rsa.RANKDATA_TABLE, "one kept column")
    rankdata_guarded(a[:2049], ol.U32, ol.DESC, 8, aligned, rsa.RANKDATA_TABLE, "one kept column, a tile and a key")
    b = ol.splitmix_fill((1 << 20) + 7, ol.U8, 9502)
    rankdata_guarded(b, ol.I8, ol.DESC, 8, aligned, rsa.RANKDATA_TABLE, "1-byte keys")
    rankdata_guarded(b, ol.U8, ol.ASC, 4, aligned, rsa.RANKDATA_TABLE, "1-byte keys, 4-byte indices")
    rankdata_guarded(b[:6149], ol.U8, ol.ASC, 4, aligned, rsa.RANKDATA_TABLE, "1-byte keys, less + equal", what=NO_PLACE)
    c = ol.splitmix_fill(70001, ol.U64, 9503, 0xFF << 40)
    rankdata_guarded(c, ol.U64, ol.ASC, 4, aligned, rsa.RANKDATA_TABLE, "8-byte keys")
    d = ol.splitmix_fill(70003, ol.U16, 9504, 0xFF00)
    rankdata_guarded(d, ol.I16, ol.ASC, 8, aligned, rsa.RANKDATA_TABLE, "2-byte keys")


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt,mask", [(ol.U32, 0x00F0FF0F), (ol.U64, 0xFFFF << 20), (ol.U16, 0xFFFF)])
def test_count16(dt, mask, aligned):
    a = ol.splitmix_fill((1 << 20) + 3, dt, 9505, mask)
    a[:4] = ul.deposit(np.array([0, 0x7FFF, 0x8000, 0xFFFF], dtype=np.uint64), mask).astype(a.dtype)
    for ib in (4, 8):
        rankdata_guarded(a, dt, ol.ASC, ib, aligned, rsa.RANKDATA_COUNT16, "count table, mask %#x, ib %d" % (mask, ib), what=NO_PLACE)
    rankdata_guarded(a[:77], dt, ol.DESC, 4, aligned, rsa.RANKDATA_COUNT16, "count table, 77 keys", what=NO_PLACE)


@pytest.mark.parametrize("aligned", [True, False])
def test_sort_route(aligned, monkeypatch):
    a = ol.splitmix_fill(300001, ol.F32, 9506, 0xFFF000FF)
    rankdata_guarded(a, ol.F32, ol.ASC, 8, aligned, rsa.RANKDATA_SORT, "f32 mixed signs")
    rankdata_guarded(a[:1000], ol.F32, ol.DESC, 4, aligned, rsa.RANKDATA_SORT, "1000 keys")
    rankdata_guarded(a[:8192], ol.F32, ol.ASC, 4, aligned, rsa.RANKDATA_SORT, "a tile of the heads pass, place alone", what=PLACE)
    b = np.sort(ol.splitmix_fill((1 << 20) + 9, ol.U32, 9507, 0x000FFFFF))
    info = rankdata_guarded(b, ol.U32, ol.ASC, 4, aligned, rsa.RANKDATA_SORT, "sorted input: runs only")
    assert info.sort.early_exit == 2
    info = rankdata_guarded(b[:70000], ol.U32, ol.ASC, 8, aligned, rsa.RANKDATA_SORT, "sorted input: an iota", what=PLACE)
    assert info.sort.early_exit == 2
    c = ol.splitmix_fill((1 << 20) + 3, ol.U16, 9508)
    rankdata_guarded(c, ol.U16, ol.ASC, 4, aligned, rsa.RANKDATA_SORT, "u16 with the place")
    d = ol.splitmix_fill((1 << 20) + 5, ol.U64, 9509, 0xFFFFFFFFFF)
    rankdata_guarded(d, ol.U64, ol.ASC, 4, aligned, rsa.RANKDATA_SORT, "u64 below 2^40")
    monkeypatch.setenv("RSX_RANKDATA_NO_TABLES", "1")
    rsa.reload_env()
    e = ol.splitmix_fill((1 << 20) + 11, ol.U8, 9510)
    rankdata_guarded(e, ol.U8, ol.ASC, 4, aligned, rsa.RANKDATA_SORT, "u8, NO_TABLES")
    f = ol.splitmix_fill((1 << 20) + 3, ol.U32, 9511, 0x00F0FF0F)
    rankdata_guarded(f, ol.U32, ol.ASC, 4, aligned, rsa.RANKDATA_SORT, "u32 count-table input, NO_TABLES", what=NO_PLACE)
