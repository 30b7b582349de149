"""Where rsx_sort_nth_device writes: src, the keys and the indices between guard bands (tests/guard_lib.py), at 256-byte aligned
residues and one element off; both routes.  The outputs hold exactly m elements: a write to element m lands in the back
guard.  Each case asserts the result against the oracle, that src is bit-identical, and that both bands of every buffer are
intact."""
import numpy as np
import pytest

import guard_lib as gl
import nth_lib as nl
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 1 << 20
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SIZES = [1001, 65537, 300001]
MS = [1, 2, 64, 65, 1000]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(scope="module")
def wants():
    """The oracle's ranks, once per (dtype, n): shared by every residue, route, m and choice of outputs."""
    out = {}
    for dt in (ol.U32, ol.F64, ol.U8):
        for n in SIZES:
            out[(dt, n)] = nl.Want(ol.splitmix_fill(n, dt, 8600 + n, 0xFFFFFFFFFFF000FF), dt, ol.ASC)
    return out


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_NTH_FORCE", raising=False)
    rsa.reload_env()


def ranks_for(n, m):
    """m ranks, distinct while m <= 65 (so that 64 selects and 65 cannot), the 1000 with repeats of 64 distinct ones"""
    if m <= 65:
        return [((2 * i + 1) * n) // (2 * m) for i in range(m)]
    return [(((i * 37) % 64) * n) // 64 for i in range(m)]


@pytest.mark.parametrize("residue", ["aligned", "one element"])
@pytest.mark.parametrize("value,route", [("1", rsa.NTH_SELECT), ("2", rsa.NTH_SORT)])
@pytest.mark.parametrize("dt,ib", [(ol.U32, 4), (ol.F64, 8), (ol.U8, 4), (ol.U32, 8)])
def test_guard_bands(dt, ib, value, route, residue, wants, monkeypatch):
    monkeypatch.setenv("RSX_NTH_FORCE", value)
    rsa.reload_env()
    kb = ol.DTYPE_SIZE[dt]
    res = {"aligned": (0, 0), "one element": (kb, ib)}[residue]
    for n in SIZES:
        want = wants[(dt, n)]
        src = gl.guarded(n, _T[kb], res[0], GUARD)
        src.load(want.bits)
        for m in MS:
            ranks = ranks_for(n, m)
            for outputs in ("both", "keys", "idx"):
                keys = gl.guarded(m, _T[kb], res[0], GUARD) if outputs != "idx" else None
                idx = gl.guarded(m, _T[ib], res[1], GUARD) if outputs != "keys" else None
                rc, info, n_less, n_equal = nl.call_device(src.t, n, ranks, dt, ol.ASC, ib, None if keys is None else keys.t,
                                                           None if idx is None else idx.t)
                assert rc == 0, rsa.lib().rsx_last_error()
                torch.cuda.synchronize()
                tag = "%s n=%d m=%d %s %s force=%s" % (ol.DTYPE_NAMES[dt], n, m, outputs, residue, value)
                expect = rsa.NTH_SORT if m == 65 else route
                if expect == rsa.NTH_SELECT and nl.check_course(tag, want, ranks, outputs != "keys", info).falls_to_sort:
                    expect = rsa.NTH_SORT
                nl.check(tag, want, ranks, None if keys is None else keys.t, None if idx is None else idx.t, n_less, n_equal, info, expect)
                gl.check_all(*[(tag + " " + name, g) for name, g in (("keys", keys), ("idx", idx)) if g is not None])
        assert np.array_equal(src.t.cpu().numpy().view(ol.NP_BITS[dt]), want.bits), "src was written"
        gl.check_all(("src n=%d" % n, src))
