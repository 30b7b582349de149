"""Where rsx_sort_unique_device writes: every route once at 256-byte aligned and once at element-aligned-only residues, with
src, aux and counts between guard bands (tests/guard_lib.py).  Each case asserts the result against the oracle, the route it
was written for, and that both bands of every buffer are intact afterwards.  On the sort route at the sizes of the sort without
a histogram the guards are sized from guard_lib's slot geometry, as tests/test_gpu_bounds.py sizes them."""
import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 4 << 20
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
N24 = 1 << 24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def residues(aligned, kb, cb):
    """(src, aux, counts) residues mod 256: all aligned, or one element / 64 bytes + one element / one count off"""
    return (0, 0, 0) if aligned else (kb, 64 + kb, cb)


def unique_guarded(a, dt, order, cb, aligned, route, what, guard=GUARD):
    kb = ol.DTYPE_SIZE[dt]
    a = np.ascontiguousarray(a, dtype=ol.NP_BITS[dt])
    want, wcnt = ul.want_unique(a, dt, order)
    rs, ra, rc = residues(aligned, kb, cb)
    src = gl.guarded(a.size, _T[kb], rs, guard)
    src.load(a)
    aux = gl.guarded(a.size, _T[kb], ra, guard)
    counts = gl.guarded(a.size, _T[cb], rc, guard) if cb else None
    out, cnt, info = rsa.radix_sort_unique(src.t, aux.t, dtype=dt, order=order, counts=counts.t if cb else None)
    torch.cuda.synchronize()
    tag = "%s (%s)" % (what, "aligned" if aligned else "element-aligned")
    assert info.route == route, (tag, info.route)
    assert out.data_ptr() in (src.t.data_ptr(), aux.t.data_ptr()), tag
    assert np.array_equal(out.cpu().numpy().view(ol.NP_BITS[dt]), want), tag
    if cb:
        got = cnt.cpu().numpy().view(np.uint32 if cb == 4 else np.uint64).astype(np.uint64)
        assert np.array_equal(got, wcnt), tag
    pairs = [(tag + " src", src), (tag + " aux", aux)] + ([(tag + " counts", counts)] if cb else [])
    gl.check_all(*pairs)
    return info


@pytest.mark.parametrize("aligned", [True, False])
def test_trivial(aligned):
    a = np.full(70001, 0x01020304, dtype=np.uint32)
    unique_guarded(a, ol.U32, ol.ASC, 8, aligned, rsa.UNIQUE_TRIVIAL, "all equal")


@pytest.mark.parametrize("aligned", [True, False])
def test_table_one_column(aligned):
    a = ol.splitmix_fill((1 << 20) + 3, ol.U32, 9301, 0x00FF0000)
    unique_guarded(a, ol.U32, ol.ASC, 4, aligned, rsa.UNIQUE_TABLE, "one kept column")
    b = ol.splitmix_fill((1 << 20) + 7, ol.U8, 9302)
    unique_guarded(b, ol.I8, ol.DESC, 8, aligned, rsa.UNIQUE_TABLE, "1-byte keys")


@pytest.mark.parametrize("aligned", [True, False])
def test_table_joint16(aligned):
    a = ol.splitmix_fill((1 << 20) + 5, ol.I16, 9303)
    unique_guarded(a, ol.I16, ol.ASC, 4, aligned, rsa.UNIQUE_TABLE, "i16 + counts")


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt,mask", [(ol.U32, 0x00F0FF0F), (ol.U64, 0x3FFFF), (ol.U64, 0xFFFFF), (ol.U16, 0xFFFF)])
def test_bitmap_lds(dt, mask, aligned):
    a = ol.splitmix_fill((1 << 20) + 3, dt, 9304, mask)
    unique_guarded(a, dt, ol.ASC, 0, aligned, rsa.UNIQUE_BITMAP_LDS, "LDS bitmap, mask %#x" % mask)
    small = a[:77]
    unique_guarded(small, dt, ol.DESC, 0, aligned, rsa.UNIQUE_BITMAP_LDS, "LDS bitmap, 77 keys")


@pytest.mark.parametrize("aligned", [True, False])
def test_bitmap_global(aligned):
    a = ol.splitmix_fill((1 << 21) + 5, ol.U32, 9305, 0x00FFFFFF)
    unique_guarded(a, ol.U32, ol.ASC, 0, aligned, rsa.UNIQUE_BITMAP_GLOBAL, "global bitmap")
    b = ol.splitmix_fill((1 << 21) + 1, ol.U64, 9306, 0x3FFFFF00000)
    unique_guarded(b, ol.I64, ol.DESC, 0, aligned, rsa.UNIQUE_BITMAP_GLOBAL, "global bitmap, i64")


@pytest.mark.parametrize("aligned", [True, False])
def test_sort_route_small_and_mid(aligned, monkeypatch):
    a = ol.splitmix_fill(300001, ol.F32, 9307, 0xFFF000FF)
    unique_guarded(a, ol.F32, ol.ASC, 8, aligned, rsa.UNIQUE_SORT, "f32 mixed signs + counts")
    unique_guarded(a[:1000], ol.F32, ol.DESC, 4, aligned, rsa.UNIQUE_SORT, "1000 keys")
    b = np.sort(ol.splitmix_fill((1 << 20) + 9, ol.U32, 9308, 0x000FFFFF))
    unique_guarded(b, ol.U32, ol.ASC, 4, aligned, rsa.UNIQUE_SORT, "sorted input: compaction only")
    c = ol.splitmix_fill((1 << 20) + 3, ol.U16, 9309)
    monkeypatch.setenv("RSX_UNIQUE_MAX_BITS", "0")
    unique_guarded(c, ol.U16, ol.ASC, 0, aligned, rsa.UNIQUE_SORT, "u16, MAX_BITS=0")
    d = ol.splitmix_fill((1 << 20) + 11, ol.U8, 9310)
    unique_guarded(d, ol.U8, ol.ASC, 4, aligned, rsa.UNIQUE_SORT, "u8, MAX_BITS=0")
    e = ol.splitmix_fill((1 << 20) + 3, ol.U32, 9311, 0x00F0FF0F)
    unique_guarded(e, ol.U32, ol.ASC, 0, aligned, rsa.UNIQUE_SORT, "u32 bitmap input, MAX_BITS=0")


@pytest.mark.parametrize("aligned", [True, False])
def test_sort_route_without_histogram(aligned):
    """Uniform u32 at 2^24: the sort's route 5 puts level-1 slots into aux; the guard exceeds a whole slot past the last one."""
    cap1, lo = gl.level1_geometry(N24, 4)
    worst = max(gl.level1_slot_overrun(N24, 4), cap1 * 4)
    assert GUARD > worst, (GUARD, worst, cap1, lo)
    a = ol.splitmix_fill(N24, ol.U32, 9312)
    info = unique_guarded(a, ol.U32, ol.ASC, 4, aligned, rsa.UNIQUE_SORT, "uniform u32, 2^24")
    assert info.sort.hybrid == 5
