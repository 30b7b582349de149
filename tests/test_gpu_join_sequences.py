"""What one call leaves for the next, with the two phases of the join among other calls on ONE context and stream:
a sort -> rsx_sort_join_device -> radix_sort_reduce -> rsx_join_pairs_device -> a sort, on the default stream and on a side stream.
The join's phases share the context with everything between them -- the copies of the keys, the index halves, the records of
tiles, the flags and histograms of the sorts -- and phase 2 must need nothing but the arrays phase 1 wrote.  Each step is checked
against its own reference (tests/seq_lib.py as it is for the sorts, tests/join_lib.py, tests/reduce_lib.py)."""
import numpy as np
import pytest

import join_lib as jl
import oracle_lib as ol
import radix_sorting_amd as rsa
import reduce_lib as rl
import seq_lib as sl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in ("RSX_JOIN_FORCE", "RSX_JOIN_NO_TABLE"):
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_JOIN_FORCE", raising=False)
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


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("force,route", [(None, rsa.JOIN_TABLE), (2, rsa.JOIN_SEARCH), (3, rsa.JOIN_MERGE)])
def test_join_among_its_neighbours(force, route, side_stream, monkeypatch):
    if force:
        monkeypatch.setenv("RSX_JOIN_FORCE", str(force))
        rsa.reload_env()
    stream = torch.cuda.Stream() if side_stream else None
    session = sl.Session(stream, with_graph=False)
    n, m = 90001, 40003
    right = ol.splitmix_fill(m, ol.U32, 9701, 0x0003FF00) | np.uint32(0x41000000)     # ten varying bits: about 39 right rows per key
    left = ol.splitmix_fill(n, ol.U32, 9702, 0x0007FF00) | np.uint32(0x41000000)      # half of the left rows match nothing
    want = jl.Want(left, right, ol.U32)
    vals = rl.small_ints(n, ol.I64, 9703)

    def on_stream():
        # 1. a sort
        first = _sort_step(session, "keys_mid", 2, 1, 70001)
        # 2. phase 1 of the join
        lt, rt = _dev(left, ol.U32), _dev(right, ol.U32)
        st, ct, pm = (torch.full((size,), -7, dtype=torch.int32, device="cuda") for size in (n, n, m))
        rc, pairs, info = jl.call_device(lt, n, rt, m, ol.U32, ol.ASC, 4, st, ct, pm, rsa.JOIN_LEFT, stream=stream)
        assert rc == 0, rsa.lib().rsx_last_error()
        session.sync()
        jl.check("step 2, phase 1", want, st, ct, pm, pairs, info, True, route, lt, rt)
        # 3. a reduce of other keys on its sort route: the copies of the keys, the index halves and the records of tiles are taken over
        keys = ol.splitmix_fill(n, ol.U32, 9704)
        keys[::3] = keys[0]
        ok, cn, sm, _, _, rinfo = rsa.radix_sort_reduce(_dev(keys, ol.U32), _dev(vals, ol.I64), dtype=ol.U32, val_dtype=ol.I64, counts=True, stream=stream)
        session.sync()
        wk, wc, ws, _, _ = rl.want_reduce(rl.groups(keys, ol.U32), vals, ol.I64)
        assert rinfo.route == rsa.REDUCE_SORT
        assert np.array_equal(ok.cpu().numpy().view(np.uint32), wk) and np.array_equal(cn.cpu().numpy().view(np.uint32).astype(np.uint64), wc)
        assert np.array_equal(sm.cpu().numpy().view(np.uint64), ws), "step 3, reduce: sum"
        # 4. phase 2 of the join, from the arrays of step 2 alone
        wl, wr = want.pairs(True)
        assert wl.size == pairs
        ol_t, or_t = (torch.full((pairs + 1,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        rc, got_pairs = jl.call_pairs(st, ct, pm, n, m, 4, rsa.JOIN_LEFT, ol_t, or_t, pairs, stream=stream)
        assert rc == 0 and got_pairs == pairs, rsa.lib().rsx_last_error()
        session.sync()
        assert np.array_equal(jl.signed(ol_t)[:-1], wl) and np.array_equal(jl.signed(or_t)[:-1], wr), "step 4, phase 2"
        assert int(ol_t[-1]) == -7 and int(or_t[-1]) == -7
        # 5. a sort
        _sort_step(session, "pairs", 3, 5, 80001, before=first)

    if stream is None:
        on_stream()
    else:
        with torch.cuda.stream(stream):
            on_stream()
        stream.synchronize()
        rsa.lib().rsx_release_stream(stream.cuda_stream)
