"""What one call leaves for the next, with the partition among other calls on ONE context and stream:
a sort -> rsx_sort_partition_device -> rsx_sort_locate_device -> rsx_sort_partition_device (other dtype, other route) -> a sort, on
the default stream and on a side stream.  The partition shares the context with everything around it -- the sort route goes
through locate's own buffers and the index halves of the rank sort, the edges are sorted by the keys-only sort, the flags and
histograms are the sorts' -- and must need nothing of what the call before it left.  Each step is checked against its own
reference (tests/seq_lib.py as it is for the sorts, tests/partition_lib.py, tests/locate_lib.py)."""
import numpy as np
import pytest

import locate_lib as ll
import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa
import seq_lib as sl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in ("RSX_PARTITION_FORCE", "RSX_PARTITION_MAX_EDGES", "RSX_PARTITION_BALLOT_PARTS", "RSX_LOCATE_FORCE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("RSX_PARTITION_MAX_EDGES", str(rsa.PARTITION_MAX_EDGES))     # (the cut-off pinned: the default is lower)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_PARTITION_MAX_EDGES", raising=False)
    rsa.reload_env()


def _dev(bits, dt):
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).cuda()


def _sort_step(session, kind, j, pos, n, before=None):
    step = sl.make_step(kind, j, pos, n=n)
    got, bufs = sl.run(step, session)
    bufs.check_guards()
    sl.check(step, got, before=before)
    return step


def _partition_step(tag, session, stream, bits, dt, order, edges, ib, below, route):
    want = pl.Want(bits, dt, order)
    n, m = bits.size, edges.size
    src_t, edges_t = _dev(bits, dt), _dev(edges, dt)
    it = torch.int32 if ib == 4 else torch.int64
    keys_t = torch.full((n,), -7, dtype=src_t.dtype, device="cuda")
    idx_t, off_t = torch.full((n,), -7, dtype=it, device="cuda"), torch.full((m + 2,), -7, dtype=it, device="cuda")
    rc, info = pl.call_device(src_t, n, edges_t, m, dt, order, ib, keys_t, idx_t, off_t, rsa.PARTITION_BELOW if below else 0, stream=stream)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    session.sync()
    pl.check(tag, want, edges, src_t, edges_t, keys_t, idx_t, off_t, below, info, route)


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("first_route", [rsa.PARTITION_SCATTER, rsa.PARTITION_SORT])
def test_partition_among_its_neighbours(first_route, side_stream):
    stream = torch.cuda.Stream() if side_stream else None
    session = sl.Session(stream, with_graph=False)
    scatter_first = first_route == rsa.PARTITION_SCATTER
    a = ol.splitmix_fill(90001, ol.U32, 9801)
    b = ol.splitmix_fill(50003, ol.F64, 9802)
    few = lambda bits, k, seed: np.concatenate([bits[:k // 2], ol.splitmix_fill(k - k // 2, ol.U32 if bits.itemsize == 4 else ol.F64, seed)])
    many = lambda bits, dt, seed: np.unique(np.concatenate([bits[:300], ol.splitmix_fill(700, dt, seed)]))

    def on_stream():
        # 1. a sort
        first = _sort_step(session, "keys_mid", 2, 1, 70001)
        # 2. a partition of u32 keys
        _partition_step("step 2", session, stream, a, ol.U32, ol.ASC, few(a, 40, 9803) if scatter_first else many(a, ol.U32, 9804), 4, False, first_route)
        # 3. locate on other keys: its table, its copy of the values and its bins are its own again
        vals = np.concatenate([b[:100], ol.splitmix_fill(200, ol.F64, 9805)])
        lw = ll.Want(b, ol.F64, ol.DESC)
        bt, vt = _dev(b, ol.F64), _dev(vals, ol.F64)
        less_t, equal_t, bin_t = (torch.full((c,), -7, dtype=torch.int64, device="cuda") for c in (vals.size, vals.size, b.size))
        rc, linfo = ll.call_device(bt, b.size, vt, vals.size, ol.F64, ol.DESC, 8, less_t, equal_t, bin_t, 0, stream=stream)
        assert rc == 0, rsa.lib().rsx_last_error()
        session.sync()
        ll.check("step 3, locate", lw, vals, bt, vt, less_t, equal_t, bin_t, False, linfo, rsa.LOCATE_SEARCH)
        # 4. a partition of f64 keys on the other route, descending, 8-byte indices, BELOW
        other = rsa.PARTITION_SORT if scatter_first else rsa.PARTITION_SCATTER
        _partition_step("step 4", session, stream, b, ol.F64, ol.DESC, many(b, ol.F64, 9806) if scatter_first else few(b, 200, 9807), 8, True, other)
        # 5. a sort
        _sort_step(session, "pairs", 3, 5, 80001, before=first)

    if stream is None:
        on_stream()
    else:
        with torch.cuda.stream(stream):
            on_stream()
        stream.synchronize()
        rsa.lib().rsx_release_stream(stream.cuda_stream)
