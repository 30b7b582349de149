"""Where rsx_sort_lex_device writes: guard bands (tests/guard_lib.py) before and after out_idx and after every column, with n
around the pack kernel's quad (n % 4 in 0 .. 3) and workgroup (1023 .. 1025 rows, 256 threads x 4 rows) boundaries, both index
widths, the three packing limits, the buffers 256-byte aligned and one element off.  out_idx holds exactly n entries: a
write to entry n lands in the back guard.  Each case asserts the permutation against the oracle's, that every column is
bit-identical afterwards, and that both bands of every buffer are intact."""
import numpy as np
import pytest

import guard_lib as gl
import lex_lib as ll
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 1 << 16
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SIZES = [4, 5, 6, 7, 1023, 1024, 1025, 4099]
SHAPES = {
    "u32,u32": [ol.U32, ol.U32],
    "u8,u16,u8": [ol.U8, ol.U16, ol.U8],
    "f64,u8": [ol.F64, ol.U8],
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(scope="module")
def wants():
    """The columns and the oracle's permutation, once per (shape, n): shared by every residue, width and packing."""
    out = {}
    for name, dtypes in SHAPES.items():
        for n in SIZES:
            cols = [ol.splitmix_fill(n, dt, 8300 + n + j, 0x8000000000000007) for j, dt in enumerate(dtypes)]
            out[(name, n)] = (cols, ll.want_perm(cols, dtypes))
    return out


@pytest.fixture(autouse=True)
def _fresh_switches(monkeypatch):
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_LEX_PACK_BYTES", raising=False)
    rsa.reload_env()


@pytest.mark.parametrize("residue", ["aligned", "one element"])
@pytest.mark.parametrize("P", [1, 4, 8])
@pytest.mark.parametrize("ib", [4, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_guard_bands(shape, ib, P, residue, wants, monkeypatch):
    monkeypatch.setenv("RSX_LEX_PACK_BYTES", str(P))
    rsa.reload_env()
    dtypes = SHAPES[shape]
    for n in SIZES:
        cols, want = wants[(shape, n)]
        bufs = []
        for c, dt in zip(cols, dtypes):
            kb = ol.DTYPE_SIZE[dt]
            g = gl.guarded(n, _T[kb], kb if residue == "one element" else 0, GUARD)
            g.load(c)
            bufs.append(g)
        out = gl.guarded(n, _T[ib], ib if residue == "one element" else 0, GUARD)
        arr = ll.lex_cols([g.t.data_ptr() for g in bufs], dtypes)
        rc, err, info = ll.call_device_raw(arr, len(dtypes), n, out.t.data_ptr(), ib)
        tag = "%s n=%d ib=%d P=%d %s" % (shape, n, ib, P, residue)
        assert rc == 0, (tag, err)
        torch.cuda.synchronize()
        assert np.array_equal(out.t.cpu().numpy().astype(np.int64), want), tag
        assert info.groups() == ll.want_groups(dtypes, P), tag
        for g, c, dt in zip(bufs, cols, dtypes):
            assert np.array_equal(g.t.cpu().numpy().view(ol.NP_BITS[dt]), c), (tag, "a column was written")
        gl.check_all((tag + " out_idx", out), *[("%s column %d" % (tag, j), g) for j, g in enumerate(bufs)])
