"""Call sequences on one (device, stream) context: what one call leaves behind must not show in the next (seq_lib.py).

The library keeps state from call to call -- two alternating sets of flags and histograms, a third set for the device-scheduled
sorts, tables "zeroed for the next call", back-off counters, scratch buffers shared between features and grown by free +
reallocate.  Every other test file starts from a clean slate; here the order of the calls is the test:

 * test_circuit / test_circuit_side_stream walk the closed path that has every ordered pair of the eighteen kinds of calls
   exactly once (seq_lib.circuit), every step checked bit for bit against its own reference as it runs, inside guard bands;
 * the directed tests below are short sequences around one piece of state each.

The route floors are lowered ONCE for the module (seq_lib.ENV), so that 2^22 keys reach the sorts without a histogram and the
select routes of topk / nth run; nothing re-reads the environment, releases a context or empties torch's cache between steps
except where a test says so."""
import ctypes as C

import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa
import seq_lib as sq
from decide_lib import zipf_like

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WALK = sq.circuit(sq.KINDS)
PIECES = sq.pieces(WALK, sq.M)
EINVAL = sq.EINVAL


@pytest.fixture(scope="module", autouse=True)
def lowered_floors():
    rsa.require_gpu()
    mp = pytest.MonkeyPatch()
    for name, value in sq.ENV.items():
        mp.setenv(name, value)
    rsa.reload_env()
    yield
    mp.undo()
    rsa.reload_env()


def run_steps(steps, session, after_each=None, before=None):
    """Run and check the steps in order; a failure names the step and the one that ran directly before it."""
    for i, step in enumerate(steps):
        got, bufs = sq.run(step, session)
        try:
            bufs.check_guards()
        except gl.GuardDamage as e:
            raise AssertionError("%s after %s: %s" % (sq.describe(step), "nothing" if before is None else sq.describe(before), e))
        sq.check(step, got, before=before)
        if step.kind == "keys_nohist":
            # even keys of 2^22 and more under the lowered floors: the sample lets them through and no slot overflows, and
            # nothing in these sequences loses an attempt of the kind before them -- the kind has to be what its name says
            assert got["route"] == 5, "%s took route %d after %s" % (sq.describe(step), got["route"],
                                                                     "nothing" if before is None else sq.describe(before))
        before = step
        if after_each is not None:
            after_each(i, step)
    return before


def step(kind, j=0, n=None, **kw):
    return sq.make_step(kind, j, n=n)._replace(**kw)


# ---- a. the circuit on the default stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", range(len(PIECES)))
def test_circuit(piece):
    """Default stream, one host thread (the host-pointer sort shares this context).  The `replay` steps replay a graph of a
    stream of the session's own (the default stream cannot capture) in the default stream's order."""
    session = sq.Session(None)
    try:
        run_steps(sq.piece_steps(WALK, sq.M, piece), session)
    finally:
        torch.cuda.synchronize()
        session.graph = None
        rsa.release_stream(session.gstream)


# ---- b. the circuit on a fresh stream, with another context busy in between -------------------------------------------------
@pytest.mark.parametrize("piece", range(len(PIECES)))
def test_circuit_side_stream(piece):
    """The same walk without the host-pointer kind on a stream of its own, and the graph of the `replay` steps lives on that
    stream's context.  A graph on the library's own context is only valid while no scratch buffer of the context grows
    (INTEGRATION.md), so the session first runs every step of the piece once, unchecked, and captures then (seq_lib.Session):
    the checked walk reallocates nothing.  After every third step a step of another size runs on a second stream; the streams
    are synchronised between steps, and neither context may see the other."""
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    steps = [st for st in sq.piece_steps(WALK, sq.M, piece) if st.kind != "host"]
    session, other = sq.Session(s, sized_for=steps), sq.Session(s2, with_graph=False)
    others = ("keys_mid", "rank", "unique", "pairs", "keys_async", "rankdata")

    def in_between(i, before):
        if i % 3 == 2:
            o = sq.make_step(others[(i // 3 + piece) % len(others)], piece + i, pos=7000 + i, n=7001 + 1013 * ((piece + i) % 37))
            run_steps([o], other)
            torch.cuda.synchronize()

    try:
        run_steps(steps, session, in_between)
    finally:
        torch.cuda.synchronize()
        session.graph = None
        rsa.release_stream(s)
        rsa.release_stream(s2)


# ---- c. directed sequences ----------------------------------------------------------------------------------------------------------
GRAPH_N = 50000


class _Captured:
    """A device-scheduled sort of GRAPH_N keys captured into a graph on stream `s`, in guarded buffers."""

    def __init__(self, form, dt, order, s):
        self.form, self.dt, self.order, self.s = form, dt, order, s
        self.B = sq.Bufs(GRAPH_N * 4)
        n = GRAPH_N
        with torch.cuda.stream(s):
            if form == "keys":
                self.k, self.ks = self.B.new("buf", n, 4), self.B.new("scratch", n, 4)
            elif form == "rank":
                self.k, self.ib = self.B.new("src", n, 4), self.B.new("index buffer", 2 * n, 4)
            else:
                self.k, self.ks = self.B.new("keys", n, 4), self.B.new("keys scratch", n, 4)
                self.v, self.vs = self.B.new("vals", n, 4), self.B.new("vals scratch", n, 4)
            rsa.fill_splitmix(self.k, seed=1, stream=s)
            self.enqueue(s)             # (sizes the workspace outside the capture)
        s.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=s):
            self.enqueue(torch.cuda.current_stream())
        torch.cuda.synchronize()

    def enqueue(self, s):
        if self.form == "keys":
            rsa.radix_sort_inplace_async(self.k, self.ks, dtype=self.dt, order=self.order, stream=s)
        elif self.form == "rank":
            rsa.radix_sort_rank_inplace_async(self.k, self.ib, dtype=self.dt, order=self.order, stream=s)
        else:
            rsa.radix_sort_pairs_inplace_async(self.k, self.ks, self.v, self.vs, dtype=self.dt, order=self.order, stream=s)

    def replay_and_check(self, seed, what):
        a = ol.splitmix_fill(GRAPH_N, self.dt, seed, 0xFFFFFFFF if seed % 2 else 0x00FFFF0F)
        vals = ol.splitmix_fill(GRAPH_N, ol.U32, seed + 50)
        with torch.cuda.stream(self.s):
            self.k.copy_(torch.from_numpy(a.view(np.int32).copy()).cuda())
            if self.form == "pairs":
                self.v.copy_(torch.from_numpy(vals.view(np.int32).copy()).cuda())
            self.graph.replay()
        self.s.synchronize()
        self.B.check_guards()
        assert np.all(self.B.tails() == sq.FILL), (what, "written behind the n-th element")
        perm = ol.stable_argsort_by_kdf(a, self.dt, self.order)
        if self.form == "keys":
            assert np.array_equal(sq._bits(self.k, np.uint32), ol.oracle_sort(a, self.dt, self.order)[0]), what
        elif self.form == "rank":
            assert np.array_equal(sq._bits(self.ib[:GRAPH_N], np.uint32), ol.oracle_rank(a, self.dt, 4, self.order)[0]), what
            assert np.array_equal(sq._bits(self.k, np.uint32), a), what
        else:
            assert np.array_equal(sq._bits(self.k, np.uint32), a[perm]), what
            assert np.array_equal(sq._bits(self.v, np.uint32), vals[perm]), what


@pytest.mark.parametrize("n_blocking", [5000, GRAPH_N])
@pytest.mark.parametrize("dt,order", [(ol.U32, ol.ASC), (ol.F32, ol.DESC)], ids=["u32", "f32-desc"])
@pytest.mark.parametrize("form", ["keys", "rank", "pairs"])
def test_graph_replay_between_blocking_sorts(form, dt, order, n_blocking):
    """A graph captured from a device-scheduled sort on the library's own context keeps the addresses of the flags and the
    histogram it was enqueued with, and the host never sees a replay.  The blocking keys-only sorts alternate between two sets
    and trust the set they count into to have been zeroed by the sort before: 1. capture at gen = g, 2. blocking sort (gen ->
    g ^ 1, zeroes set g), 3. replay, 4. blocking sort (gen -> g: counts into set g).  Had the replay used set g, step 4 would
    count on top of the replay's histogram and read its `unsorted` flag -- wrong offsets (stores beyond n, hence the guards) or
    a missed early exit.  The device-scheduled sorts have a set of their own (Ctx::ASYNC_SET), so step 4 is right whatever was
    replayed before it: once on unsorted and once on sorted input (early exit, `aux` untouched), then the replay again.
    n_blocking = 5000 is the one-launch sort for these types (it uses neither set), 50 000 takes the fused histogram."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    cap = _Captured(form, dt, order, s)
    try:
        last = None
        for round_, style4 in enumerate((0, 6)):
            st2 = step("keys_mid", 2 * round_, n=n_blocking, dt=dt, order=order, style=0)
            st4 = step("presorted" if style4 == 6 else "keys_mid", 2 * round_ + 1, n=n_blocking, dt=dt, order=order, style=style4)
            last = run_steps([st2], session, before=last)
            cap.replay_and_check(100 + round_, (form, "replay between the blocking sorts", round_))
            last = run_steps([st4], session, before=last)
            if style4 == 6:
                assert sq.expect(st4)["early_exit"] == 2
            cap.replay_and_check(201 + round_, (form, "replay after the blocking sorts", round_))
    finally:
        torch.cuda.synchronize()
        cap.graph = None
        rsa.release_stream(s)


def _sptr(s):
    return C.c_void_p(s.cuda_stream)


def _refusals(s, src, out, n):
    """(name, kind of the valid call that follows, the refused call -> rc): RSX_EINVAL of every entry point that has one."""
    L = rsa.lib()
    p, o = src.data_ptr(), out.data_ptr()
    res, info, sz = C.c_void_p(), rsa.Info(), C.c_size_t(0)
    r3 = np.array([0, n, 1], dtype=np.uint64)
    less, equal = np.full(3, 0xA5, dtype=np.uint64), np.full(3, 0xA5, dtype=np.uint64)
    cols = (rsa.LexCol * 1)()
    cols[0].data, cols[0].dtype, cols[0].order = p, ol.U32, 0
    top = np.full(256, 0xA5, dtype=np.uint64)
    hsrc, haux = np.arange(64, dtype=np.uint32)[::-1].copy(), np.full(128, 0xA5A5A5A5, dtype=np.uint32)

    def host_untouched():
        assert np.all(less == 0xA5) and np.all(equal == 0xA5) and np.all(top == 0xA5), "a refused call wrote a host array"
        assert np.array_equal(hsrc, np.arange(64, dtype=np.uint32)[::-1]) and np.all(haux == 0xA5A5A5A5), "a refused call wrote a host buffer"

    def rank_async(j):
        st = _valid("sub_async", j)
        return st._replace(seed=st.seed & ~1)

    def pairs_async(j):
        st = _valid("sub_async", j)
        return st._replace(seed=st.seed | 1)

    return host_untouched, [
        ("sort: bad dtype", "keys_mid", lambda: L.rsx_sort_device(p, o, n, 99, 0, _sptr(s), C.byref(res), C.byref(info))),
        ("pairs: payload of 3 bytes", "pairs", lambda: L.rsx_sort_pairs_device(p, o, p, o, n, ol.U32, 3, 0, _sptr(s), C.byref(info))),
        ("rank: index of 3 bytes", "rank", lambda: L.rsx_sort_rank_device(p, o, n, ol.U32, 3, 0, _sptr(s), C.byref(res), C.byref(info))),
        ("inplace_async: bad dtype", "keys_async", lambda: L.rsx_sort_inplace_async(p, o, n, 99, 0, _sptr(s))),
        ("inplace_async_hint: bad dtype", lambda j: _valid_hint(s), lambda: L.rsx_sort_inplace_async_hint(p, o, n, 99, 0, _sptr(s), 1)),
        ("pairs_inplace_async: payload of 3 bytes", pairs_async, lambda: L.rsx_sort_pairs_inplace_async(p, o, p, o, n, ol.U32, 3, 0, _sptr(s))),
        ("histogram: bad dtype", lambda j: _valid_histogram(s), lambda: L.rsx_histogram_device(p, n, 99, 0, o, o, _sptr(s))),
        ("msd_split: no such column", lambda j: _valid_split(s, False), lambda: L.rsx_msd_split_device(p, o, n, ol.U32, 0, 4, top.ctypes.data,
                                                                                                     _sptr(s))),
        ("msd_split_async: no such column", lambda j: _valid_split(s, True), lambda: L.rsx_msd_split_async(p, o, n, ol.U32, 0, 4, o, _sptr(s))),
        ("host sort: bad dtype", "host", lambda: L.rsx_sort(hsrc.ctypes.data, haux.ctypes.data, 64, 99, 0, C.byref(res), C.byref(info))),
        ("host rank: index of 3 bytes", lambda j: _valid_host_rank(), lambda: L.rsx_sort_rank(hsrc.ctypes.data, haux.ctypes.data, 64, ol.U32, 3, 0,
                                                                                           C.byref(res), C.byref(info))),
        ("rank_inplace_async: index of 2 bytes", rank_async, lambda: L.rsx_sort_rank_inplace_async(p, o, n, ol.U32, 2, 0, _sptr(s))),
        ("unique: counts of 3 bytes", "unique", lambda: L.rsx_sort_unique_device(p, o, n, ol.U32, 0, o, 3, _sptr(s), C.byref(res), C.byref(sz),
                                                                                  C.byref(rsa.UniqueInfo()))),
        ("group: index of 3 bytes", "group", lambda: L.rsx_sort_group_device(p, n, ol.U32, 0, o, None, None, None, 3, _sptr(s), C.byref(sz),
                                                                             C.byref(rsa.GroupInfo()))),
        ("rankdata: index of 3 bytes", "rankdata", lambda: L.rsx_sort_rankdata_device(p, n, ol.U32, 0, o, None, None, 3, _sptr(s),
                                                                                      C.byref(rsa.RankdataInfo()))),
        ("topk: k > n", "topk", lambda: L.rsx_sort_topk_device(p, n, n + 1, ol.U32, 0, o, None, 4, _sptr(s), C.byref(rsa.TopkInfo()))),
        ("nth: rank >= n", "nth", lambda: L.rsx_sort_nth_device(p, n, rsa._u64p(r3), 3, ol.U32, 0, o, None, 4, rsa._u64p(less),
                                                                rsa._u64p(equal), _sptr(s), C.byref(rsa.NthInfo()))),
        ("lex: no columns", "lex", lambda: L.rsx_sort_lex_device(cols, 0, n, o, 4, _sptr(s), C.byref(rsa.LexInfo()))),
        ("records: key sticks out", "records", lambda: L.rsx_sort_records_tagged_device(p, o, n // 3, 12, 9, ol.U32, 0, _sptr(s), C.byref(res),
                                                                                        C.byref(info))),
    ]


def _valid(kind, j):
    lo, hi, _ = sq.SPEC[kind]
    return sq.make_step(kind, j, pos=500 + j, n=max(lo, 20011 + 17 * j))


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _valid_hint(s):
    """rsx_sort_inplace_async_hint on even keys, as the hint says"""
    a = ol.splitmix_fill(50021, ol.U32, 90)
    with torch.cuda.stream(s):
        buf = _dev32(a)
        rsa.radix_sort_inplace_async(buf, torch.zeros_like(buf), dtype=ol.U32, stream=s, hints=rsa.HINT_EVEN_TOP_DIGITS)
    s.synchronize()
    assert np.array_equal(sq._bits(buf, np.uint32), ol.oracle_sort(a, ol.U32)[0]), "rsx_sort_inplace_async_hint after its refusal"


def _digit_counts(a):
    k = ol.kdf_keys(a, ol.U32, ol.ASC)
    return np.concatenate([np.bincount(((k >> np.uint32(8 * j)) & np.uint32(0xFF)).astype(np.int64), minlength=256) for j in range(4)]).astype(np.uint64)


def _valid_histogram(s, a=None):
    """rsx_histogram_device: every column's digit counts (returned on the device) and the unsorted flag"""
    a = ol.splitmix_fill(40001, ol.U32, 91) if a is None else a
    with torch.cuda.stream(s):
        src = _dev32(a)
        hist = torch.full((1024,), -1, dtype=torch.int64, device="cuda")
        unsorted = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc = rsa.lib().rsx_histogram_device(src.data_ptr(), a.size, ol.U32, 0, hist.data_ptr(), unsorted.data_ptr(), _sptr(s))
    s.synchronize()
    assert rc == 0, rsa.lib().rsx_last_error()
    assert np.array_equal(sq._bits(hist, np.uint64), _digit_counts(a)) and int(unsorted.item()) != 0, "rsx_histogram_device after its refusal"
    return hist


def _valid_split(s, device_scheduled):
    """rsx_msd_split_device / rsx_msd_split_async by the top byte: a stable pass by that digit"""
    a = ol.splitmix_fill(40001, ol.U32, 92)
    dig = (a >> np.uint32(24)).astype(np.int64)
    hist = _valid_histogram(s, a) if device_scheduled else None
    with torch.cuda.stream(s):
        src = _dev32(a)
        out = torch.zeros_like(src)
        if device_scheduled:
            rc = rsa.lib().rsx_msd_split_async(src.data_ptr(), out.data_ptr(), a.size, ol.U32, 0, 3, hist.data_ptr(), _sptr(s))
        else:
            top = np.zeros(256, dtype=np.uint64)
            rc = rsa.lib().rsx_msd_split_device(src.data_ptr(), out.data_ptr(), a.size, ol.U32, 0, 3, top.ctypes.data, _sptr(s))
    s.synchronize()
    assert rc == 0, rsa.lib().rsx_last_error()
    if not device_scheduled:
        assert np.array_equal(top, np.bincount(dig, minlength=256).astype(np.uint64)), "rsx_msd_split_device: counts"
    assert np.array_equal(sq._bits(out, np.uint32), a[np.argsort(dig, kind="stable")]), "the split after its refusal"


def _valid_host_rank():
    a = ol.splitmix_fill(30011, ol.U32, 93)
    ib = np.full(2 * a.size, 0xA5A5A5A5, dtype=np.uint32)
    ranks, info = rsa.radix_sort_rank_host(a.copy(), ib, ol.U32)
    want, half, _, _ = ol.oracle_rank(a, ol.U32, 4)
    assert info.result_in_aux == half and np.array_equal(ranks, want), "rsx_sort_rank after its refusal"


def test_refused_then_valid():
    """Every refusal (RSX_EINVAL) writes nothing, and leaves the context as it was: the valid call of the same entry point that
    follows at once and a mid-size blocking sort after it are right."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    n = 30000
    a = ol.splitmix_fill(n, ol.U32, 77)
    B = sq.Bufs(n * 4)
    try:
        with torch.cuda.stream(s):
            src, out = B.new("src", n, 4, a), B.new("out", 2 * n, 4)
        last = run_steps([_valid("keys_mid", 0)], session)        # (the context exists and has state to disturb)
        host_untouched, refusals = _refusals(s, src, out, n)
        for j, (name, valid, call) in enumerate(refusals):
            with torch.cuda.stream(s):
                rc = call()
            s.synchronize()
            assert rc == EINVAL, (name, rc, rsa.lib().rsx_last_error())
            B.check_guards()
            assert np.array_equal(sq._bits(src, np.uint32), a) and bool((out.view(torch.uint8) == sq.FILL).all().item()), (name, "wrote")
            host_untouched()
            if isinstance(valid, str):
                last = run_steps([_valid(valid, j)], session, before=last)
            else:
                st = valid(j)          # (a step of a chosen form, or a call with a check of its own for what has no step kind)
                if isinstance(st, sq.Step):
                    last = run_steps([st], session, before=last)
            last = run_steps([_valid("keys_mid", j + 1)], session, before=last)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


@pytest.mark.parametrize("kind", ["unique", "group", "rankdata", "topk", "nth", "lex"])
def test_refused_on_a_capturing_stream_then_valid(kind):
    """The features wait for a count on the host, so a capturing stream is refused (RSX_EINVAL, nothing written, the capture
    stays intact); the same call right after the capture and a mid-size blocking sort are right."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    n = 30000
    a = ol.splitmix_fill(n, ol.U32, 78)
    B = sq.Bufs(n * 4)
    L = rsa.lib()
    try:
        with torch.cuda.stream(s):
            src, out = B.new("src", n, 4, a), B.new("out", 2 * n, 4)
        last = run_steps([_valid(kind, 0)], session)              # (the context of this stream exists before the capture)
        p, o = src.data_ptr(), out.data_ptr()
        res, sz = C.c_void_p(), C.c_size_t(0)
        r3, h = np.array([0, 5, 1], dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        cols = (rsa.LexCol * 1)()
        cols[0].data, cols[0].dtype, cols[0].order = p, ol.U32, 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cs = _sptr(torch.cuda.current_stream())
            rc = {
                "unique": lambda: L.rsx_sort_unique_device(p, o, n, ol.U32, 0, None, 0, cs, C.byref(res), C.byref(sz), C.byref(rsa.UniqueInfo())),
                "group": lambda: L.rsx_sort_group_device(p, n, ol.U32, 0, o, None, None, None, 4, cs, C.byref(sz), C.byref(rsa.GroupInfo())),
                "rankdata": lambda: L.rsx_sort_rankdata_device(p, n, ol.U32, 0, o, None, None, 4, cs, C.byref(rsa.RankdataInfo())),
                "topk": lambda: L.rsx_sort_topk_device(p, n, 100, ol.U32, 0, o, None, 4, cs, C.byref(rsa.TopkInfo())),
                "nth": lambda: L.rsx_sort_nth_device(p, n, rsa._u64p(r3), 3, ol.U32, 0, o, None, 4, rsa._u64p(h), rsa._u64p(h), cs,
                                                     C.byref(rsa.NthInfo())),
                "lex": lambda: L.rsx_sort_lex_device(cols, 1, n, o, 4, cs, C.byref(rsa.LexInfo())),
            }[kind]()
            err = L.rsx_last_error()
        assert rc == EINVAL and b"capturing" in err, (kind, rc, err)
        torch.cuda.synchronize()
        B.check_guards()
        assert np.array_equal(sq._bits(src, np.uint32), a) and bool((out.view(torch.uint8) == sq.FILL).all().item()), (kind, "wrote")
        run_steps([_valid(kind, 1), _valid("keys_mid", 2)], session, before=last)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


def test_too_small_workspace_then_valid():
    """rsx_sort_inplace_async_ws in a workspace that is too small: RSX_EINVAL, nothing enqueued; then the same call in a
    workspace of rsx_workspace_bytes, and a mid-size blocking sort on the stream's own context."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    n = 100003
    a = ol.splitmix_fill(n, ol.U32, 79)
    B = sq.Bufs(n * 4)
    try:
        with torch.cuda.stream(s):
            buf, scratch = B.new("buf", n, 4, a), B.new("scratch", n, 4)
            ws = torch.full((rsa.workspace_bytes(n, ol.U32) + 512,), sq.FILL, dtype=torch.uint8, device="cuda")
            off = (-ws.data_ptr()) % 256
            last = run_steps([_valid("keys_mid", 0)], session)
            rc = rsa.lib().rsx_sort_inplace_async_ws(buf.data_ptr(), scratch.data_ptr(), n, ol.U32, 0, ws[off:].data_ptr(), 1024, _sptr(s))
            s.synchronize()
            assert rc == EINVAL, (rc, rsa.lib().rsx_last_error())
            assert np.array_equal(sq._bits(buf, np.uint32), a) and bool((scratch.view(torch.uint8) == sq.FILL).all().item())
            assert bool((ws[off + 1024:] == sq.FILL).all().item()), "written behind the 1024 bytes the call was given"
            rsa.radix_sort_inplace_async_ws(buf, scratch, ws[off:off + rsa.workspace_bytes(n, ol.U32)], dtype=ol.U32, stream=s)
            s.synchronize()
        B.check_guards()
        assert np.array_equal(sq._bits(buf, np.uint32), ol.oracle_sort(a, ol.U32)[0])
        run_steps([_valid("keys_mid", 1)], session, before=last)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


@pytest.mark.parametrize("kind", ["keys_mid", "rank", "pairs", "unique", "group", "rankdata"])
def test_early_exits_then_unsorted(kind):
    """Calls that end early -- pre-sorted input, n = 0, 1, 2, an all-equal array -- each followed by an unsorted array of the same
    size and by a smaller one: what the early exit skipped (zeroing a set, resetting a table) is not missed by the next call."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    try:
        last, j = None, 0
        for n, style in ((70001, 6), (0, 0), (1, 0), (2, 0), (70001, 5), (20000, 6), (20000, 5)):
            for dt, order in ((ol.U32, ol.ASC), (ol.F64, ol.DESC)):
                j += 1
                early = step(kind, j, n=n, dt=dt, order=order, style=style)
                after = [step(kind, j + 100, n=max(n, 3), dt=dt, order=order, style=0),
                         step(kind, j + 200, n=max(n // 3, 2), dt=dt, order=order, style=1)]
                last = run_steps([early] + after, session, before=last)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


@pytest.mark.parametrize("kind,dt", [("keys_mid", ol.U32), ("keys_mid", ol.I64), ("pairs", ol.F32)], ids=["u32", "i64", "pairs-f32"])
def test_grow_shrink_grow(kind, dt):
    """One context: 300 001 keys, 2^22 + 7 keys (the slots of a sort without a histogram are allocated), 4097 keys, a feature
    (group, then lex), then 2^22 + 2^20 keys -- larger, so the buffers are freed and reallocated under everything that was cached."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    try:
        steps = [step(kind, 1, n=300001, dt=dt), step(kind, 2, n=(1 << 22) + 7, dt=dt, style=0), step(kind, 3, n=4097, dt=dt),
                 step("group", 4, n=150001, dt=dt), step("lex", 5, n=150001, dt=dt),
                 step(kind, 6, n=(1 << 22) + (1 << 20), dt=dt, style=0), step(kind, 7, n=300001, dt=dt)]
        run_steps(steps, session)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


def test_release_in_mid_sequence():
    """rsx_release_stream and rsx_release between the steps of the circuit's first piece (without the replays: a graph does not
    outlive its context): everything after them is still right, on contexts that start again from nothing."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)

    def release(i, before):
        torch.cuda.synchronize()
        if i % 3 == 1:
            rsa.release_stream(s)
        elif i % 3 == 2:
            rsa.lib().rsx_release()

    try:
        steps = [st for st in sq.piece_steps(WALK, sq.M, 0) + sq.piece_steps(WALK, sq.M, 9) if st.kind not in ("replay", "host")]
        run_steps(steps, session, release)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


def test_armed_histogram():
    """rsx_capture_histogram arms the thread's NEXT blocking sort that reaches its histogram (include/rsx.h): a sort of one key
    never writes and leaves the arm; the sort of 2^22 + 5 keys that follows would do without a histogram, but an armed sort
    counts -- ITS counts are delivered, equal to the oracle's rs_sort_main, and the arm is gone: the mid-size sort after it
    leaves the array alone."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    hist = np.full(256 * 4, 0xA5A5A5A5, dtype=np.uint64)
    try:
        with rsa.capturing_histogram(hist):
            one = step("keys_mid", 1, n=1, dt=ol.U32)
            big = step("keys_nohist", 0, n=(1 << 22) + 5, dt=ol.U32, order=ol.ASC, style=0)
            mid = step("keys_mid", 3, n=100001, dt=ol.U32, order=ol.ASC, style=0)
            last = run_steps([one], session)
            assert np.all(hist == 0xA5A5A5A5), "a sort of one key wrote the armed histogram"
            got, bufs = sq.run(big, session)
            bufs.check_guards()
            sq.check(big, got, before=last)
            assert got["route"] != 5, "an armed sort has to count"
            # what rs_sort_main leaves in the caller's Hist: the counts, summed up in the kept columns (radix_sort.hpp:72-80;
            # include/radix_sort.hpp, hist_post_state, makes it from the delivered counts the same way)
            a = sq.inputs(big)["keys"]
            _, _, whist = ol.oracle_sort_main_hist(a, ol.U32, ol.hvt_bytes_for(a.size))
            delivered = hist.copy()
            post = hist.copy()
            for j in sq.expect(big)["cols"]:
                post[256 * j:256 * j + 256] = np.cumsum(hist[256 * j:256 * j + 256])
            assert np.array_equal(post, whist), "the counts are not those of the first sort that ran a histogram"
            run_steps([mid], session, before=big)
            assert np.array_equal(hist, delivered), "the arm outlived the sort that delivered"
        free = step("keys_nohist", 1, n=(1 << 22) + 5, dt=ol.U32, order=ol.ASC, style=0)
        got, bufs = sq.run(free, session)
        sq.check(free, got, before=mid)
        assert got["route"] == 5, ("disarmed, uniform keys: the sort without a histogram", got["route"])
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


# ---- lost attempts and the back-off ---------------------------------------------------------------------------------------------
LOST_N = (1 << 22) + 99


def _lost_u32():
    """test_gpu_hybrid.py::test_blind_called_off_by_an_overflowing_slot: a top digit with 1.6 times its share, which the sample
    does not see and the digit's level-1 slot does not hold."""
    a = ol.splitmix_fill(LOST_N, ol.U32, 78, 0xFFFFFFFF).view(np.uint32).copy()
    extra = np.flatnonzero((a >> 24) == 0x11)[: int(0.6 * LOST_N / 256)]
    a[extra] = (a[extra] & np.uint32(0x00FFFFFF)) | np.uint32(0x77000000)
    return a


def _lost_log():
    """test_gpu_logroute.py::test_clustered_mantissas_lose_the_attempt_and_sort_anyway"""
    a = zipf_like(1 << 22, 11)
    blen = np.floor(np.log2(a.astype(np.float64))).astype(np.uint64) + np.uint64(1)
    sh = np.where(blen > 12, blen - np.uint64(12), np.uint64(0)).astype(np.uint64)
    return np.where(blen > 12, a & ~(np.uint64(0xFF) << sh), a).astype(np.uint64)


BIG_N = (16 << 20) + 3


def _lost_level2():
    """... its second input: a (digit, digit) pair with five times its share overflows its level-2 slot."""
    b = ol.splitmix_fill(LOST_N, ol.U32, 78, 0xFFFFFFFF).view(np.uint32).copy()
    b[5000:5000 + 300 * 11:11] = (b[5000:5000 + 300 * 11:11] & np.uint32(0x0000FFFF)) | np.uint32(0x43210000)
    return b


def _lost_after_writing(digit):
    """test_gpu_routes.py::test_level1_slot_overflows_after_the_second_buffer_was_written: 16 Mi + 3 keys, one top digit with 1.4
    times its share.  The attempt is called off AFTER its level-1 pass has written: digit 0x05's slot lies in the caller's
    second buffer, 0xF3's in the scratch array behind the last slot."""
    a = ol.splitmix_fill(BIG_N, ol.U32, 4160 + digit, 0xFFFFFFFF).view(np.uint32).copy()
    idx = np.arange(1000, 1000 + 26000 * 7, 7)
    a[idx] = (a[idx] & np.uint32(0x00FFFFFF)) | np.uint32(digit << 24)
    return a


_MAKE = {"lost u32": _lost_u32, "lost level 2": _lost_level2, "even u32": lambda: ol.splitmix_fill(LOST_N, ol.U32, 79, 0xFFFFFFFF),
         "lost 16Mi 0x05": lambda: _lost_after_writing(0x05), "lost 16Mi 0xF3": lambda: _lost_after_writing(0xF3),
         "even 16Mi": lambda: ol.splitmix_fill(BIG_N, ol.U32, 4159, 0xFFFFFFFF),
         "lost log": _lost_log, "even log": lambda: zipf_like(1 << 22, 12)}
_EVEN = {"lost u32": "even u32", "lost level 2": "even u32", "lost 16Mi 0x05": "even 16Mi", "lost 16Mi 0xF3": "even 16Mi",
         "lost log": "even log"}
_CASES, _RANKS = {}, {}


def _case(name):
    """(keys, sorted keys) of an input, made once for the module."""
    if name not in _CASES:
        a = _MAKE[name]()
        _CASES[name] = (a, ol.oracle_sort(a, ol.U32 if a.itemsize == 4 else ol.U64)[0])
    return _CASES[name]


def _ranks(name):
    if name not in _RANKS:
        _RANKS[name] = ol.oracle_rank_by_records(_case(name)[0], ol.U32)[0]
    return _RANKS[name]


LOST = [True, True, True, False, False, False, False, True, False, False]


def _lost_run(form, lost, lost_name):
    """The sorts of the sequence `lost` (True: the input that loses its attempt), then one more lost attempt, rsx_reload_env and
    an even input.  Every result is compared with the oracle's; returns (routes of the sequence, route after rsx_reload_env)."""
    s = torch.cuda.Stream()
    even_name = _EVEN[lost_name]
    dt = ol.U64 if form == "log" else ol.U32
    n = _case(lost_name)[0].size
    B = sq.Bufs(n * ol.DTYPE_SIZE[dt])
    routes = []
    try:
        with torch.cuda.stream(s):
            src = B.new("src", n, ol.DTYPE_SIZE[dt])
            out = B.new("second buffer", 2 * n if form == "rank" else n, 4 if form == "rank" else ol.DTYPE_SIZE[dt])

            def sort(name):
                a, want = _case(name)
                src.copy_(torch.from_numpy(a.view(np.int32 if dt == ol.U32 else np.int64).copy()).cuda())
                if form == "rank":
                    res, info = rsa.radix_sort_rank(src, out, dtype=dt, stream=s)
                    route, got, want = info.hybrid, sq._bits(res, np.uint32), _ranks(name)
                elif form == "async":
                    rsa.radix_sort_inplace_async(src, out, dtype=dt, stream=s)
                    route, got = rsa.async_route(s), sq._bits(src, ol.NP_BITS[dt])
                else:
                    res, info = rsa.radix_sort(src, out, dtype=dt, stream=s)
                    route, got = info.hybrid, sq._bits(res, ol.NP_BITS[dt])
                s.synchronize()
                B.check_guards()
                assert np.array_equal(got, want), (form, name, len(routes), "differs from the oracle after routes", routes)
                routes.append(route)
                return route

            rsa.reload_env()            # (what earlier tests taught this process is forgotten; the floors stay as the module set them)
            for l in lost:
                sort(lost_name if l else even_name)
            # the context sits sorts out again after another lost attempt; rsx_reload_env forgets that
            sort(lost_name)
            rsa.reload_env()
            return routes[:len(lost)], sort(even_name)
    finally:
        torch.cuda.synchronize()
        rsa.release_stream(s)


LOST_FORMS = [("keys", "lost u32"), ("keys", "lost level 2"), ("keys", "lost 16Mi 0x05"), ("keys", "lost 16Mi 0xF3"),
              ("rank", "lost u32"), ("log", "lost log"), ("async", "lost u32"), ("async", "lost 16Mi 0x05")]


@pytest.mark.parametrize("form,lost_name", LOST_FORMS, ids=["%s-%s" % (f, n[5:].replace(" ", "-")) for f, n in LOST_FORMS])
def test_lost_attempts_and_the_backoff(form, lost_name):
    """Inputs whose attempt without a histogram (or by (bit length, mantissa) digits) is lost alternate with even ones of the
    same size: a level-1 and a level-2 slot that overflow at 2^22 + 99 keys, and at 16 Mi + 3 keys a level-1 slot that overflows
    after the pass has written into the caller's second buffer (digit 0x05) or into the scratch slots (0xF3).  Every result is
    the oracle's, and the routes follow the rule of rsx_route_blind.hpp restated in seq_lib.backoff_routes: a lost attempt makes
    the context sit out the next 1, 3, 7 .. sorts of the kind (the device-scheduled form, read through rsx_async_route: 1, 2,
    4 ..), a won one resets it, and rsx_reload_env forgets it."""
    won = 6 if form == "log" else 5
    routes, after_reload = _lost_run(form, LOST, lost_name)
    attempts = sq.backoff_routes(LOST, device=form == "async")
    want_routes = [bool(t and not l) for t, l in zip(attempts, LOST)]
    assert [r == won for r in routes] == want_routes, (form, lost_name, routes, attempts)
    assert after_reload == won, (form, lost_name, "rsx_reload_env did not forget the back-off", after_reload)
