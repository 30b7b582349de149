"""What one call leaves for the next, with rsx_sort_segments_device among other calls on ONE context and stream:
a sort -> segments (LDS) -> a rank sort -> segments (MIXED: the long segments' sorts work in lex's buffers and the rank sort's
flags) -> rsx_sort_lex_device -> segments (the composed route: lex's buffers again, and the feature's own) -> a partition ->
segments (LDS, other dtype) -> a sort, on the default stream and on a side stream.  Each step is checked against its own
reference (tests/seq_lib.py as it is for the sorts and lex, tests/partition_lib.py, tests/segments_lib.py)."""
import numpy as np
import pytest

import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa
import segments_lib as sg
import seq_lib as sl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_NAMES = ("RSX_SEGMENTS_FORCE", "RSX_SEGMENTS_MAX_LONG", "RSX_PARTITION_FORCE", "RSX_PARTITION_MAX_EDGES")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in _NAMES:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    for name in _NAMES:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()


def _dev(bits):
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).cuda()


def _sort_step(session, kind, j, pos, n, before=None):
    step = sl.make_step(kind, j, pos, n=n)
    got, bufs = sl.run(step, session)
    bufs.check_guards()
    sl.check(step, got, before=before)
    return step


def _segments_step(tag, monkeypatch, session, stream, dt, order, lengths, ib, local, force, route, seed):
    monkeypatch.setenv("RSX_SEGMENTS_FORCE", force)
    monkeypatch.setenv("RSX_SEGMENTS_MAX_LONG", "4")
    rsa.reload_env()
    off = np.concatenate([[0], np.cumsum(lengths)])
    n = int(off[-1])
    want = sg.Want(ol.splitmix_fill(n, dt, seed), dt, off, order)
    src_t = _dev(want.bits)
    off_t = _dev(off.astype(np.uint32 if ib == 4 else np.uint64))
    it = torch.int32 if ib == 4 else torch.int64
    keys_t = torch.full((n,), -7, dtype=src_t.dtype, device="cuda")
    idx_t = torch.full((n,), -7, dtype=it, device="cuda")
    rc, info = sg.call_device(src_t, n, off_t, len(lengths), dt, order, ib, keys_t, idx_t, rsa.SEGMENTS_LOCAL_IDX if local else 0, stream=stream)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    session.sync()
    sg.check(tag, want, src_t, off_t, keys_t, idx_t, local, info, route)


def _partition_step(tag, session, stream, bits, dt, edges):
    want = pl.Want(bits, dt, ol.ASC)
    n, m = bits.size, edges.size
    src_t, edges_t = _dev(bits), _dev(edges)
    keys_t = torch.full((n,), -7, dtype=src_t.dtype, device="cuda")
    idx_t, off_t = torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((m + 2,), -7, dtype=torch.int32, device="cuda")
    rc, info = pl.call_device(src_t, n, edges_t, m, dt, ol.ASC, 4, keys_t, idx_t, off_t, 0, stream=stream)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    session.sync()
    pl.check(tag, want, edges, src_t, edges_t, keys_t, idx_t, off_t, False, info)


@pytest.mark.parametrize("side_stream", [False, True])
def test_segments_among_their_neighbours(side_stream, monkeypatch):
    stream = torch.cuda.Stream() if side_stream else None
    session = sl.Session(stream, with_graph=False)
    cap32, cap64 = sg.cap_of(ol.U32, True), sg.cap_of(ol.F64, True)
    a = ol.splitmix_fill(90001, ol.U32, 9901)

    def on_stream():
        first = _sort_step(session, "keys_mid", 2, 1, 70001)
        _segments_step("step 2, LDS", monkeypatch, session, stream, ol.U32, ol.ASC, [0, 1, 30, 300, 3000, cap32, 0, 64, 7], 4, False, "1",
                       rsa.SEGMENTS_LDS, 9902)
        _sort_step(session, "rank", 3, 3, 60001)
        _segments_step("step 4, MIXED", monkeypatch, session, stream, ol.F64, ol.DESC, [cap64 + 1, 12, 0, 2049, 3 * cap64, 1, 500], 8, True, "1",
                       rsa.SEGMENTS_MIXED, 9903)
        _sort_step(session, "lex", 2, 5, 50001)
        _segments_step("step 6, LEX", monkeypatch, session, stream, ol.I16, ol.ASC, [5, 0, 70000, 1, 258, 2], 4, True, "2", rsa.SEGMENTS_LEX, 9904)
        _partition_step("step 7, partition", session, stream, a, ol.U32, np.concatenate([a[:20], ol.splitmix_fill(20, ol.U32, 9905)]))
        _segments_step("step 8, LDS", monkeypatch, session, stream, ol.U8, ol.DESC, [256, 257, 0, 20000, 2, 2048, 63], 8, False, "1",
                       rsa.SEGMENTS_LDS, 9906)
        _sort_step(session, "pairs", 3, 9, 80001, before=first)

    if stream is None:
        on_stream()
    else:
        with torch.cuda.stream(stream):
            on_stream()
        stream.synchronize()
        rsa.lib().rsx_release_stream(stream.cuda_stream)
