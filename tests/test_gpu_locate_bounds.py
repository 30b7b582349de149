"""rsx_sort_locate_device writes inside its outputs only: less, equal (exactly m entries) and the bins (exactly n) between guard
bands (tests/guard_lib.py), at an aligned residue and one element off it, on every route -- the table route (u8), the search
route and the sort route (u32, f64; 4097 values always sort, every other list is also run with RSX_LOCATE_FORCE=2).  The
results are compared with NumPy as in tests/test_gpu_locate.py; src and vals lie between guards too."""
import itertools

import numpy as np
import pytest

import guard_lib as gl
import locate_lib as ll
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_T = {1: torch.int8, 4: torch.int32, 8: torch.int64}
GUARD = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    monkeypatch.delenv("RSX_LOCATE_FORCE", raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_LOCATE_FORCE", raising=False)
    rsa.reload_env()


def _values(want, m, seed):
    """m distinct-ish values, a third of them taken from the keys"""
    dt = want.dt
    v = np.unique(ol.splitmix_fill(m + m // 4 + 300, dt, seed))
    rng = np.random.default_rng(seed)
    if v.size >= m:
        v = rng.permutation(v)[:m]
    else:                                   # (one-byte keys: there are only 256 values)
        v = np.concatenate([v, v[rng.integers(0, v.size, size=m - v.size)]])
    k = min(m // 3, want.bits.size)
    if ol.DTYPE_SIZE[dt] > 1 and m != 4097 and m != 4096:
        v[:k] = want.bits[:k]
    return v


@pytest.mark.parametrize("dt", [ol.U32, ol.F64, ol.U8])
@pytest.mark.parametrize("n", [1001, 65537, 300001])
def test_outputs_between_guards(dt, n, monkeypatch):
    kb = ol.DTYPE_SIZE[dt]
    bits = ol.splitmix_fill(n, dt, 9500 + dt)
    want = ll.Want(bits, dt)
    rot = itertools.cycle([(4, 0, False), (8, 8, True), (4, 4, True), (8, 0, False)])     # idx bytes, the outputs' residue, BELOW
    for m in (1, 64, 4096, 4097):
        vals = _values(want, m, 9600 + m)
        distinct = np.unique(vals).size
        natural = rsa.LOCATE_TABLE if kb == 1 else rsa.LOCATE_SEARCH if distinct <= rsa.LOCATE_MAX_SEARCH_VALUES else rsa.LOCATE_SORT
        for force in (None, "2"):
            if force and natural == rsa.LOCATE_SORT:
                continue
            if force:
                monkeypatch.setenv("RSX_LOCATE_FORCE", force)
            else:
                monkeypatch.delenv("RSX_LOCATE_FORCE", raising=False)
            rsa.reload_env()
            ib, residue, below = next(rot)
            src_g = gl.guarded(n, _T[kb], kb if residue else 0, GUARD)
            vals_g = gl.guarded(m, _T[kb], 0, GUARD)
            src_g.load(bits)
            vals_g.load(vals)
            outs = [gl.guarded(c, torch.int32 if ib == 4 else torch.int64, residue, GUARD) for c in (m, m, n)]
            rc, info = ll.call_device(src_g.t, n, vals_g.t, m, dt, ol.ASC, ib, outs[0].t, outs[1].t, outs[2].t, rsa.LOCATE_BINS_BELOW if below else 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            tag = "%s n=%d m=%d ib=%d residue=%d below=%d force=%s" % (ol.DTYPE_NAMES[dt], n, m, ib, residue, below, force)
            gl.check_all(("src", src_g), ("vals", vals_g), ("less", outs[0]), ("equal", outs[1]), ("bins", outs[2]))
            ll.check(tag, want, vals, src_g.t, vals_g.t, outs[0].t, outs[1].t, outs[2].t, below, info, rsa.LOCATE_SORT if force else natural)
            # one output alone: the others' absence moves nothing
            alone = gl.guarded(n, torch.int32 if ib == 4 else torch.int64, ib if residue else 0, GUARD)
            rc, info = ll.call_device(src_g.t, n, vals_g.t, m, dt, ol.ASC, ib, None, None, alone.t, 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            gl.check_all(("src", src_g), ("vals", vals_g), ("bins alone", alone))
            ll.check(tag + " bins alone", want, vals, src_g.t, vals_g.t, None, None, alone.t, False, info)
