"""rsx_sort_join_device and rsx_join_pairs_device write inside their outputs only: start, count (exactly n entries), right_perm
(exactly m) and the pair lists (exactly n_pairs) between guard bands (tests/guard_lib.py), once at 256-byte-aligned residues and
once at residues that are element-aligned only, left and right at different distances from a 16-byte boundary, on every route
of phase 1 -- the table route (u8, u32 with few varying bits), the search and the merge route forced (u32, u64) -- and for the
expansion, inner and left.  The results are compared with NumPy as in tests/test_gpu_join.py; the inputs lie between guards too
and come back unchanged."""
import numpy as np
import pytest

import guard_lib as gl
import join_lib as jl
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_T = {1: torch.int8, 4: torch.int32, 8: torch.int64}
GUARD = 1 << 16
ENVS = ("RSX_JOIN_FORCE", "RSX_JOIN_NO_TABLE")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()


def _inputs(dt, n, m, seed):
    """Right keys with few varying bits (many to many), left keys half of which match."""
    kb = ol.DTYPE_SIZE[dt]
    if kb == 1:
        return ol.splitmix_fill(n, dt, seed), ol.splitmix_fill(m, dt, seed + 1) % np.uint8(120)
    t = ol.NP_BITS[dt]
    right = (ol.splitmix_fill(m, dt, seed + 1) & t(0x0FF0)) | t(0x00C00001)
    left = (ol.splitmix_fill(n, dt, seed) & t(0x1FF0)) | t(0x00C00001)
    return left, right


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt,force,route", [(ol.U8, None, rsa.JOIN_TABLE), (ol.U32, None, rsa.JOIN_TABLE), (ol.U64, None, rsa.JOIN_TABLE),
                                            (ol.U32, 2, rsa.JOIN_SEARCH), (ol.U64, 2, rsa.JOIN_SEARCH), (ol.U8, 2, rsa.JOIN_SEARCH),
                                            (ol.U32, 3, rsa.JOIN_MERGE), (ol.U64, 3, rsa.JOIN_MERGE)])
def test_both_phases_between_guards(dt, force, route, aligned, monkeypatch):
    if force:
        monkeypatch.setenv("RSX_JOIN_FORCE", str(force))
        rsa.reload_env()
    kb = ol.DTYPE_SIZE[dt]
    n, m = 20011, 3001
    left, right = _inputs(dt, n, m, 9800 + dt)
    want = jl.Want(left, right, dt)
    for ib, flags in ((4, 0), (8, rsa.JOIN_LEFT)):
        it = torch.int32 if ib == 4 else torch.int64
        # residues mod 256: all zero, or one element off for the outputs and 1 / 3 elements off for left / right
        res = (lambda k: 0) if aligned else (lambda k: k)
        left_g, right_g = gl.guarded(n, _T[kb], res(kb), GUARD), gl.guarded(m, _T[kb], res(3 * kb), GUARD)
        left_g.load(left)
        right_g.load(right)
        start_g, count_g, perm_g = gl.guarded(n, it, res(ib), GUARD), gl.guarded(n, it, res(64 + ib), GUARD), gl.guarded(m, it, res(2 * ib), GUARD)
        rc, pairs, info = jl.call_device(left_g.t, n, right_g.t, m, dt, ol.ASC, ib, start_g.t, count_g.t, perm_g.t, flags)
        assert rc == 0, rsa.lib().rsx_last_error()
        torch.cuda.synchronize()
        tag = "%s force=%s aligned=%d ib=%d flags=%d" % (ol.DTYPE_NAMES[dt], force, aligned, ib, flags)
        gl.check_all(("left", left_g), ("right", right_g), ("start", start_g), ("count", count_g), ("right_perm", perm_g))
        jl.check(tag, want, start_g.t, count_g.t, perm_g.t, pairs, info, bool(flags), route, left_g.t, right_g.t)
        # count alone: the others' absence moves nothing
        alone = gl.guarded(n, it, res(ib), GUARD)
        rc, pairs1, info = jl.call_device(left_g.t, n, right_g.t, m, dt, ol.ASC, ib, None, alone.t, None, flags)
        assert rc == 0 and pairs1 == pairs, rsa.lib().rsx_last_error()
        torch.cuda.synchronize()
        gl.check_all(("left", left_g), ("right", right_g), ("count alone", alone))
        jl.check(tag + " count alone", want, None, alone.t, None, pairs1, info, bool(flags), route, left_g.t, right_g.t)
        # phase 2 from the guarded arrays into guarded lists of exactly n_pairs entries
        before = [g.t.clone() for g in (start_g, count_g, perm_g)]
        outl_g, outr_g = gl.guarded(pairs, it, res(ib), GUARD), gl.guarded(pairs, it, res(128 + ib), GUARD)
        rc, got_pairs = jl.call_pairs(start_g.t, count_g.t, perm_g.t, n, m, ib, flags, outl_g.t, outr_g.t, pairs)
        assert rc == 0 and got_pairs == pairs, rsa.lib().rsx_last_error()
        torch.cuda.synchronize()
        gl.check_all(("start", start_g), ("count", count_g), ("right_perm", perm_g), ("out_left", outl_g), ("out_right", outr_g))
        wl, wr = want.pairs(bool(flags))
        assert np.array_equal(jl.signed(outl_g.t), wl) and np.array_equal(jl.signed(outr_g.t), wr), tag + " pairs"
        for g, b in zip((start_g, count_g, perm_g), before):
            assert torch.equal(g.t, b), tag + ": phase 2 wrote an input"
