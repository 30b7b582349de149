"""Where rsx_sort_topk_device writes: src, the keys and the indices between guard bands (tests/guard_lib.py), at 256-byte
aligned residues, one element off, and 64 bytes + one element off; both routes.  The outputs hold exactly k elements: a
write to element k lands in the back guard.  Each case asserts the result against the oracle, that src is bit-identical, and
that both bands of every buffer are intact."""
import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa
import topk_lib as tl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 1 << 20
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SIZES = [257, 65537, 300001]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(scope="module")
def wants():
    """The oracle's ranks, once per (dtype, n): shared by every residue, route and k."""
    out = {}
    for dt, ib in ((ol.U32, 4), (ol.F64, 8), (ol.U8, 4)):
        for n in SIZES:
            out[(dt, n)] = tl.Want(ol.splitmix_fill(n, dt, 6100 + n, 0xFFFFFFFFFFF000FF), dt, ol.ASC)
    return out


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_TOPK_FORCE", raising=False)
    rsa.reload_env()


@pytest.mark.parametrize("residue", ["aligned", "one element", "64 + one element"])
@pytest.mark.parametrize("value,route", [("1", rsa.TOPK_SELECT), ("2", rsa.TOPK_SORT)])
@pytest.mark.parametrize("dt,ib", [(ol.U32, 4), (ol.F64, 8), (ol.U8, 4)])
def test_guard_bands(dt, ib, value, route, residue, wants, monkeypatch):
    monkeypatch.setenv("RSX_TOPK_FORCE", value)
    rsa.reload_env()
    kb = ol.DTYPE_SIZE[dt]
    res = {"aligned": (0, 0), "one element": (kb, ib), "64 + one element": (64 + kb, 64 + ib)}[residue]
    for n in SIZES:
        want = wants[(dt, n)]
        src = gl.guarded(n, _T[kb], res[0], GUARD)
        src.load(want.bits)
        for k in (1, 257, n // 2):
            keys = gl.guarded(k, _T[kb], res[0], GUARD)
            idx = gl.guarded(k, _T[ib], res[1], GUARD)
            rc, info = tl.call_device(src.t, n, k, dt, ol.ASC, ib, keys.t, idx.t)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            tag = "%s n=%d k=%d %s force=%s" % (ol.DTYPE_NAMES[dt], n, k, residue, value)
            tl.check(tag, want, k, keys.t, idx.t, info, route)
            gl.check_all((tag + " keys", keys), (tag + " idx", idx))
        assert np.array_equal(src.t.cpu().numpy().view(ol.NP_BITS[dt]), want.bits), "src was written"
        gl.check_all(("src n=%d" % n, src))
