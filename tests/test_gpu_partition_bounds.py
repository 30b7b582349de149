"""rsx_sort_partition_device writes inside its outputs only: out_keys, out_idx (exactly n entries) and offsets (exactly m + 2)
between guard bands (tests/guard_lib.py), at an aligned residue and one element off it, on both routes -- the scatter route (1, 64
and 255 edges, either ranking form) and the sort route (256 edges always sort, every other list is also run with
RSX_PARTITION_FORCE=2).  The results are compared with NumPy as in tests/test_gpu_partition.py; src and edges lie between guards
too and must come back unchanged."""
import itertools

import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import partition_lib as pl
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
    monkeypatch.delenv("RSX_PARTITION_FORCE", raising=False)
    monkeypatch.delenv("RSX_PARTITION_BALLOT_PARTS", raising=False)
    monkeypatch.setenv("RSX_PARTITION_MAX_EDGES", str(rsa.PARTITION_MAX_EDGES))     # (the cut-off pinned: the default is lower)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_PARTITION_FORCE", raising=False)
    monkeypatch.delenv("RSX_PARTITION_MAX_EDGES", raising=False)
    rsa.reload_env()


def _edges(want, m, seed):
    """m distinct edges, a third of them taken from the keys where those are wide enough to stay distinct"""
    dt = want.dt
    if ol.DTYPE_SIZE[dt] == 1:
        return np.random.default_rng(seed).permutation(np.arange(256, dtype=np.uint8))[:m]
    v = np.unique(ol.splitmix_fill(m + m // 4 + 300, dt, seed))
    v = np.random.default_rng(seed).permutation(v)[:m]
    k = min(m // 3, want.bits.size)
    v[:k] = want.bits[:k]
    return v


@pytest.mark.parametrize("dt", [ol.U32, ol.F64, ol.U8])
@pytest.mark.parametrize("n", [1001, 65537, 300001])
def test_outputs_between_guards(dt, n, monkeypatch):
    kb = ol.DTYPE_SIZE[dt]
    bits = ol.splitmix_fill(n, dt, 9500 + dt)
    want = pl.Want(bits, dt)
    rot = itertools.cycle([(4, 0, False), (8, 8, True), (4, 4, True), (8, 0, False)])     # idx bytes, the outputs' residue, BELOW
    for m in (1, 64, 255, 256):
        edges = _edges(want, m, 9600 + m)
        natural = pl.natural_route(edges, dt)
        for force in (None, "2"):
            if force and natural == rsa.PARTITION_SORT:
                continue
            if force:
                monkeypatch.setenv("RSX_PARTITION_FORCE", force)
            else:
                monkeypatch.delenv("RSX_PARTITION_FORCE", raising=False)
            rsa.reload_env()
            ib, residue, below = next(rot)
            it = torch.int32 if ib == 4 else torch.int64
            src_g = gl.guarded(n, _T[kb], kb if residue else 0, GUARD)
            edges_g = gl.guarded(m, _T[kb], 0, GUARD)
            src_g.load(bits)
            edges_g.load(edges)
            keys_g = gl.guarded(n, _T[kb], kb if residue else 0, GUARD)
            idx_g, off_g = gl.guarded(n, it, residue, GUARD), gl.guarded(m + 2, it, residue, GUARD)
            rc, info = pl.call_device(src_g.t, n, edges_g.t, m, dt, ol.ASC, ib, keys_g.t, idx_g.t, off_g.t, rsa.PARTITION_BELOW if below else 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            tag = "%s n=%d m=%d ib=%d residue=%d below=%d force=%s" % (ol.DTYPE_NAMES[dt], n, m, ib, residue, below, force)
            gl.check_all(("src", src_g), ("edges", edges_g), ("keys", keys_g), ("idx", idx_g), ("offsets", off_g))
            pl.check(tag, want, edges, src_g.t, edges_g.t, keys_g.t, idx_g.t, off_g.t, below, info, rsa.PARTITION_SORT if force else natural)
            # one output alone: the others' absence moves nothing
            alone = gl.guarded(n, it, ib if residue else 0, GUARD)
            rc, info = pl.call_device(src_g.t, n, edges_g.t, m, dt, ol.ASC, ib, None, alone.t, None, 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            gl.check_all(("src", src_g), ("edges", edges_g), ("idx alone", alone))
            pl.check(tag + " idx alone", want, edges, src_g.t, edges_g.t, None, alone.t, None, False, info)
