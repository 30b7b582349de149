"""rsx_sort_segments_device writes inside its outputs only: out_keys and out_idx (exactly n entries each) between guard bands
(tests/guard_lib.py), at an aligned residue and one element off it, on every route -- LDS (RSX_SEGMENTS_FORCE=1, no segment longer
than cap), MIXED (the same with segments of cap + 1 keys) and the composed route (RSX_SEGMENTS_FORCE=2).  The results are compared
with NumPy as in tests/test_gpu_segments.py; src and offsets lie between guards too and must come back unchanged."""
import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa
import segments_lib as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_T = {1: torch.int8, 4: torch.int32, 8: torch.int64}
GUARD = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_SEGMENTS_FORCE", raising=False)
    monkeypatch.delenv("RSX_SEGMENTS_MAX_LONG", raising=False)
    rsa.reload_env()


def _lengths(n, cap, with_long, seed):
    """mixed lengths that sum to n: cap (and cap + 1 where long segments are wanted) where they fit, every class, empty ones, a tail"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    for want in ([cap + 1] if with_long else []) + [cap, 0, 1, 2500, 257, 64, 0, 13] + ([cap + 1] if with_long else []):
        if want <= left:
            out.append(want)
            left -= want
    while left:
        x = min(left, int(rng.choice([0, 1, 7, 33, 256, 300, 2048, 2049])))
        out.append(x)
        left -= x
    out = list(rng.permutation(out))
    return np.concatenate([[0], np.cumsum(out)]).astype(np.int64)


@pytest.mark.parametrize("dt", [ol.U32, ol.F64, ol.U8])
@pytest.mark.parametrize("n", [1001, 65537, 300001])
def test_outputs_between_guards(dt, n, monkeypatch):
    kb = ol.DTYPE_SIZE[dt]
    bits = ol.splitmix_fill(n, dt, 9700 + dt)
    cap = sg.cap_of(dt, True)
    for ri, route in enumerate((rsa.SEGMENTS_LDS, rsa.SEGMENTS_MIXED, rsa.SEGMENTS_LEX)):
        with_long = route == rsa.SEGMENTS_MIXED
        if with_long and n <= cap:
            continue     # (no segment of n keys or fewer is too long for LDS)
        off = _lengths(n, cap, with_long, 9800 + n)
        m = off.size - 1
        want = sg.Want(bits, dt, off)
        monkeypatch.setenv("RSX_SEGMENTS_FORCE", "2" if route == rsa.SEGMENTS_LEX else "1")
        monkeypatch.setenv("RSX_SEGMENTS_MAX_LONG", "16")
        rsa.reload_env()
        # every route at the aligned residue and one element off it; the index width and local / global alternate with the
        # residue, and which of them meets which residue alternates with the route, the dtype and n
        for off_residue in (False, True):
            flip = (ri + dt + n + off_residue) % 2 == 1
            ib, local = (8, True) if flip else (4, False)
            it = torch.int32 if ib == 4 else torch.int64
            kres, ires = (kb, ib) if off_residue else (0, 0)     # the residues mod 256 of the key and of the index buffers
            src_g = gl.guarded(n, _T[kb], kres, GUARD)
            off_g = gl.guarded(m + 1, it, ires, GUARD)
            src_g.load(bits)
            off_g.load(off.astype(np.uint32 if ib == 4 else np.uint64))
            keys_g = gl.guarded(n, _T[kb], kres, GUARD)
            idx_g = gl.guarded(n, it, ires, GUARD)
            rc, info = sg.call_device(src_g.t, n, off_g.t, m, dt, ol.ASC, ib, keys_g.t, idx_g.t, rsa.SEGMENTS_LOCAL_IDX if local else 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            tag = "%s n=%d m=%d ib=%d off_residue=%d local=%d route=%d" % (ol.DTYPE_NAMES[dt], n, m, ib, off_residue, local, route)
            gl.check_all(("src", src_g), ("offsets", off_g), ("keys", keys_g), ("idx", idx_g))
            sg.check(tag, want, src_g.t, off_g.t, keys_g.t, idx_g.t, local, info, route)
            # one output alone: the other's absence moves nothing (keys alone: another cap, so other classes)
            alone_i = gl.guarded(n, it, ires, GUARD)
            rc, info = sg.call_device(src_g.t, n, off_g.t, m, dt, ol.ASC, ib, None, alone_i.t, 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            gl.check_all(("src", src_g), ("offsets", off_g), ("idx alone", alone_i))
            sg.check(tag + " idx alone", want, src_g.t, off_g.t, None, alone_i.t, False, info, route)
            alone_k = gl.guarded(n, _T[kb], kres, GUARD)
            rc, info = sg.call_device(src_g.t, n, off_g.t, m, dt, ol.ASC, ib, alone_k.t, None, 0)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            gl.check_all(("src", src_g), ("offsets", off_g), ("keys alone", alone_k))
            sg.check(tag + " keys alone", want, src_g.t, off_g.t, alone_k.t, None, False, info)
