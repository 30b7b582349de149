"""Concurrent calls: sorts of several contexts in flight on the device together, host threads inside the library together.

INTEGRATION.md promises that calls on disjoint buffers are safe from several threads, that calls on one (device, stream) are
serialised by the context's lock, and that threads with streams of their own overlap.  Every other test file has one host
thread and at most one library kernel chain in flight; here

 A. four device-scheduled sorts on four streams are queued behind a gate (a spinning kernel on a fifth stream) and released in
    the same instant: look-back chains, ticket counters and slot cursors of four contexts run with the CUs shared;
 B. four host threads, each with a stream and a seq_lib.Session of its own, walk fixed lists of steps (concurrent_lib), one of
    them replaying a graph; and the features (locate / partition, reduce / join) the same way;
 C. four threads share ONE stream: the context's lock serialises them while its buffers grow;
 D. what belongs to the calling thread: the armed histogram, the last error, a context's creation, rsx_release_stream of a
    stream nobody else is on.

Everything is compared bit for bit with the references the suite already has (oracle_lib, seq_lib.expect, the *_lib helpers),
after the threads have joined, so that the threads spend their time in the library.  No test sets an RSX_* switch: the
environment must not change while a second thread exists (include/rsx.h, rsx_reload_env).  A worker that is still running after
concurrent_lib.LIMIT_S ends the pytest session: nothing more may be started on a device that holds a hung kernel."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import concurrent_lib as cl
import guard_lib as gl
import inner_lib as il
import join_lib as jl
import locate_lib as ll
import oracle_lib as ol
import pairs_lib as pl
import partition_lib as ptl
import radix_sorting_amd as rsa
import reduce_lib as rl
import seq_lib as sq

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GATE_US = 20000      # rsx_spin_device's unit; the sorts of case A are queued while it spins


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


def _threads(workers):
    """concurrent_lib.run_threads; a hung worker ends the session."""
    try:
        return cl.run_threads(workers, cl.LIMIT_S)
    except cl.Hung as e:
        pytest.exit("test_gpu_concurrent: %s -- nothing more is started on the GPU" % e, returncode=3)


def _release(*streams):
    torch.cuda.synchronize()
    for s in streams:
        rsa.release_stream(s)


# ---- A. device overlap behind a gate ----------------------------------------------------------------------------------------------
_KEYS, _WANT = {}, {}


def _keys(n, dt, style, seed):
    key = (n, dt, style, seed)
    if key not in _KEYS:
        a = il.wide_ties(n, dt, seed) if style == "ties" else il.wide(n, dt, seed)
        a = np.ascontiguousarray(a, dtype=ol.NP_BITS[dt])
        a.setflags(write=False)
        _KEYS[key] = a
    return _KEYS[key]


class _Call:
    """One device-scheduled sort on a stream of its own, in guarded buffers: form "keys" (rsx_sort_inplace_async), "pairs"
    (rsx_sort_pairs_inplace_async, 4-byte payloads), "rank" (rsx_sort_rank_inplace_async, 4-byte indices) or "ws"
    (rsx_sort_inplace_async_ws in a guarded workspace of rsx_workspace_bytes_fast)."""

    def __init__(self, form, n, dt, order, style, seed):
        self.form, self.n, self.dt, self.order, self.seed = form, n, dt, order, seed
        self.tag = "%s[%s %s n=%d]" % (form, ol.DTYPE_NAMES[dt], "desc" if order else "asc", n)
        self.a = _keys(n, dt, style, seed)
        self.vals = ol.splitmix_fill(n, ol.U32, seed + 1) if form == "pairs" else None
        self.stream = torch.cuda.Stream()
        kb = ol.DTYPE_SIZE[dt]
        self.B = B = sq.Bufs(n * kb)
        self.ws = None
        if form in ("keys", "ws"):
            self.data = {"buf": self.a}
            self.buf, self.scratch = B.new("buf", n, kb), B.new("scratch", n, kb)
            if form == "ws":
                self.ws = gl.Guarded(rsa.workspace_bytes_fast(n, dt), torch.uint8, 0, B.guard)
        elif form == "pairs":
            self.data = {"keys": self.a, "vals": self.vals}
            self.k, self.ks = B.new("keys", n, kb), B.new("keys scratch", n, kb)
            self.v, self.vs = B.new("vals", n, 4), B.new("vals scratch", n, 4)
        else:
            self.data = {"src": self.a}
            self.src, self.ib = B.new("src", n, kb), B.new("index buffer", 2 * n, 4)
        self.graph = None

    def load(self):
        """Every buffer FILL again, the inputs in place (on the current stream; the caller synchronises)."""
        for name, g, n in self.B.all:
            g.raw[g.start:g.end].fill_(sq.FILL)
            if name in self.data:
                d = np.ascontiguousarray(self.data[name]).reshape(-1).view(np.uint8)
                g.raw[g.start:g.start + d.size].copy_(torch.from_numpy(d.copy()))

    def enqueue(self, stream=None):
        s = self.stream if stream is None else stream
        if self.graph is not None:
            with torch.cuda.stream(s):
                self.graph.replay()
        elif self.form == "keys":
            rsa.radix_sort_inplace_async(self.buf, self.scratch, dtype=self.dt, order=self.order, stream=s)
        elif self.form == "ws":
            rsa.radix_sort_inplace_async_ws(self.buf, self.scratch, self.ws.t, dtype=self.dt, order=self.order, stream=s)
        elif self.form == "pairs":
            rsa.radix_sort_pairs_inplace_async(self.k, self.ks, self.v, self.vs, dtype=self.dt, order=self.order, stream=s)
        else:
            rsa.radix_sort_rank_inplace_async(self.src, self.ib, dtype=self.dt, order=self.order, stream=s)

    def capture(self):
        """The call as a graph (linear: one stream); the workspace is the caller's, so nothing the graph names can move."""
        assert self.form == "ws"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.stream):
            self.enqueue(torch.cuda.current_stream())
        torch.cuda.synchronize()
        self.graph = g

    def route(self):
        if self.form == "ws":
            return rsa.async_route_ws(self.ws.t, self.n, self.dt, self.stream)
        return rsa.async_route(self.stream)

    def want(self):
        key = (self.form if self.form != "ws" else "keys", self.n, self.dt, self.order, self.seed)
        if key not in _WANT:
            if self.form in ("keys", "ws"):
                _WANT[key] = (ol.oracle_sort(self.a, self.dt, self.order)[0],)
            elif self.form == "pairs":
                o = pl.Order(self.a, self.dt, self.order)
                _WANT[key] = (o.keys, o.vals(self.vals))
            elif ol.DTYPE_SIZE[self.dt] == 4:
                _WANT[key] = (ol.want_ranks(self.a, self.dt, self.order, big=pl.BIG)[0],)
            else:
                _WANT[key] = (ol.oracle_rank(self.a, self.dt, 4, self.order)[0].copy(),)
        return _WANT[key]

    def check(self, what):
        tag = "%s, %s" % (self.tag, what)
        ut = ol.NP_BITS[self.dt]
        self.B.check_guards()
        if self.ws is not None:
            self.ws.check(tag + ": workspace")
        assert np.all(self.B.tails() == sq.FILL), (tag, "written behind the n-th element")
        w = self.want()
        if self.form in ("keys", "ws"):          # the result always ends in the first buffer
            il.same(tag, "buf", sq._bits(self.buf, ut), w[0])
        elif self.form == "pairs":
            il.same(tag, "keys", sq._bits(self.k, ut), w[0])
            il.same(tag, "vals", sq._bits(self.v, np.uint32), w[1])
        else:                                     # the ranks always end in the first half, the keys are not written
            il.same(tag, "ranks", sq._bits(self.ib[:self.n], np.uint32), w[0])
            il.same(tag, "src", sq._bits(self.src, ut), self.a)

    def close(self):
        self.graph = None
        rsa.release_stream(self.stream)


U32, U64, I32, I64, F32, F64, ASC, DESC = ol.U32, ol.U64, ol.I32, ol.I64, ol.F32, ol.F64, ol.ASC, ol.DESC
N_ASYNC_NOHIST = (9 << 20) + 3
# (form, n, dtype, order, input): the smallest shapes of each route the suite names -- the one-launch sort (4096), quarter tiles
# with a look-back chain over nine tiles (70001 u32), one MSB pass and leaves chosen on the device (N_ONE_LEVEL), the sizes from
# which the blocking sorts go without a histogram (N22 pairs / ranks, N23 u32 keys, N64 8-byte keys; the device-scheduled forms
# still count at these sizes, in many more tiles).  The rank sorts get keys with ties, so that stability shows.
A_CASES = {
    "one-launch-and-nohist": [("keys", 4096, U32, DESC, "wide"), ("pairs", il.N_ONE_LEVEL, F32, ASC, "wide"),
                              ("rank", il.N22, U32, ASC, "ties"), ("ws", il.N23, U32, ASC, "wide")],
    "chain-and-leaves": [("keys", 70001, U32, ASC, "wide"), ("pairs", il.N22, U32, DESC, "wide"),
                         ("rank", il.N_ONE_LEVEL, I32, DESC, "ties"), ("ws", il.N_ONE_LEVEL, U32, DESC, "wide")],
    "8-byte": [("keys", il.N64, U64, ASC, "wide"), ("pairs", 70001, I64, DESC, "wide"), ("rank", 4096, U64, ASC, "ties"),
               ("ws", il.N64, F64, DESC, "wide")],
    # the first size at which the DEVICE-SCHEDULED keys-only sorts go without a histogram (async_blind_ok: 9 Mi 4-byte keys;
    # 36 MiB a buffer): two attempts -- one in the library's slots, one in a caller's workspace -- with their look-back chains,
    # ticket counters and slot cursors side by side, next to a key + payload and a rank sort
    "nohist-on-the-device": [("keys", N_ASYNC_NOHIST, U32, ASC, "wide"), ("pairs", il.N22, F32, ASC, "wide"),
                             ("rank", il.N22, I32, DESC, "ties"), ("ws", N_ASYNC_NOHIST, U32, DESC, "wide")],
}
A_ROUTES = {"nohist-on-the-device": {"keys": 5, "ws": 5}}     # what the case is for: asserted where the calls run alone


def _behind_the_gate(calls, gate_us=GATE_US):
    """Case A for calls that have run alone once: inputs, outputs and fill again; a spin on a fifth stream and an event behind
    it; every call's stream waits for the event and gets its call; one synchronisation.  Returns (seconds the enqueueing took,
    was the event still outstanding after the last enqueue)."""
    gate = torch.cuda.Stream()
    try:
        rsa.spin(1, gate)                      # (the gate stream's context exists before anything is timed)
        for c in calls:
            c.load()
        torch.cuda.synchronize()
        opened = torch.cuda.Event()
        rsa.spin(gate_us, gate)
        opened.record(gate)
        t0 = time.perf_counter()
        for c in calls:
            c.stream.wait_event(opened)
            c.enqueue()
        took = time.perf_counter() - t0
        closed = not opened.query()
        torch.cuda.synchronize()
        return took, closed
    finally:
        _release(gate)


def _case_a(specs, graph_first=False, want_routes=None):
    calls = [_Call(form, n, dt, order, style, 4200 + 10 * i) for i, (form, n, dt, order, style) in enumerate(specs)]
    try:
        # 1. every call alone: the contexts have their sizes (no hipFree later), and the routes are noted
        alone = []
        for c in calls:
            c.load()
            torch.cuda.synchronize()
            c.enqueue()
            alone.append(c.route())
            c.check("alone")
            if want_routes and c.form in want_routes:
                assert alone[-1] == want_routes[c.form], (c.tag, "alone: route", alone[-1], "the case wants", want_routes[c.form])
        if graph_first:
            calls[0].capture()
        took, closed = _behind_the_gate(calls)
        print("case A: enqueueing %d calls took %.3f ms behind a gate of %d us; gate still closed: %s; routes %s"
              % (len(calls), took * 1e3, GATE_US, closed, alone))
        assert closed, ("the host was too slow for the gate: enqueueing took %.3f ms and the %d us spin had ended, so the sorts "
                        "were not released together (no result was compared)" % (took * 1e3, GATE_US))
        for c, r in zip(calls, alone):
            c.check("released together")
            assert c.route() == r, (c.tag, "route", c.route(), "alone", r)
    finally:
        torch.cuda.synchronize()
        for c in calls:
            c.close()


@pytest.mark.parametrize("case", list(A_CASES))
def test_four_device_scheduled_sorts_released_together(case):
    """A. rsx_sort_inplace_async, rsx_sort_pairs_inplace_async, rsx_sort_rank_inplace_async and rsx_sort_inplace_async_ws on
    four side streams, each queued behind an event that a 20 ms spin on a fifth stream records: when the last call is enqueued
    the event must not have happened yet (else the TEST has failed to build its condition -- the host was too slow for the
    gate -- and says so), so the four sorts start in the same instant.  Then, per stream: the oracle's result, the result in
    the first buffer / the first half, tails and guard bands intact, and the route the call took when it ran alone.
    Observed on an MI355X: enqueueing the four calls takes 0.21 to 0.38 ms, a fiftieth of the 20 ms the gate stays closed
    (printed with -s).  The routes of the first three cases are 0 and 1: the device-scheduled entry points go without a histogram
    only from 9 Mi 4-byte keys, 8 Mi 8-byte keys and 16 Mi pairs on (include/rsx.h), above the sizes that send the BLOCKING sorts
    there; the last case has its two keys-only sorts at that floor (route 5 asserted), and the blocking form of the route runs
    beside other contexts in test_threads_walk_their_own_sequences (its keys_nohist step)."""
    _case_a(A_CASES[case], want_routes=A_ROUTES.get(case))


def test_graph_replay_released_with_eager_sorts():
    """A, second case: a graph captured from the _ws keys sort (linear, a workspace of its own) is replayed on stream 1 behind
    the gate while streams 2 to 4 hold eager device-scheduled sorts."""
    specs = [("ws", il.N23, U32, DESC, "wide"), ("keys", il.N_ONE_LEVEL, F32, ASC, "wide"), ("pairs", 70001, U32, ASC, "wide"),
             ("rank", il.N22, F32, DESC, "ties")]
    _case_a(specs, graph_first=True)


# ---- B. host threads with streams of their own ----------------------------------------------------------------------------------
def _assert_overlap(timeline, names):
    counts = cl.overlaps(timeline)
    print("case B: calls that overlapped another worker's, per worker: %s of %s"
          % (dict(counts), {w: len(v) for w, v in timeline.calls.items()}))
    assert all(counts.get(w, 0) >= 1 for w in names), ("a worker never was in the library together with another one", dict(counts))


def test_threads_walk_their_own_sequences():
    """B. Four threads, four streams, four sessions (built in the main thread; worker 0's owns a graph on its context, sized
    for its own steps).  Each worker enqueues a 20 ms spin on its stream and walks its list (concurrent_lib.sort_lists); results
    and buffers are kept and checked after the join: seq_lib.check, the tails, the guards.  Every worker's first call overlaps
    the others' by construction -- and overlaps() has to say so (observed on an MI355X: 8 to 10 of every worker's 10 calls
    overlap another worker's).  The keys_nohist step (inner_lib.N23 u32 keys, blocking) takes the route without a histogram
    while the other three contexts sort."""
    lists = cl.sort_lists()
    streams = [torch.cuda.Stream() for _ in lists]
    sessions = []
    timeline = cl.Timeline()
    try:
        for w, (s, steps) in enumerate(zip(streams, lists)):
            sessions.append(sq.Session(s, with_graph=w == 0, sized_for=steps if w == 0 else ()))
        torch.cuda.synchronize()

        def worker(w):
            def walk():
                rsa.spin(cl.SPIN_US, streams[w])
                return [timeline.call(sq.run, step, sessions[w], label=step.kind) for step in lists[w]]
            return walk

        names = ["worker %d" % w for w in range(len(lists))]
        results = _threads([(names[w], worker(w)) for w in range(len(lists))])
        torch.cuda.synchronize()
        for w, (steps, res) in enumerate(zip(lists, results)):
            before = None
            for step, (got, bufs) in zip(steps, res):
                try:
                    bufs.check_guards()
                except gl.GuardDamage as e:
                    raise AssertionError("%s, %s: %s" % (names[w], sq.describe(step), e))
                sq.check(step, got, before=before)
                if step.kind == "keys_nohist":
                    assert got["route"] == 5, (names[w], sq.describe(step), "route", got["route"])
                before = step
        _assert_overlap(timeline, names)
    finally:
        torch.cuda.synchronize()
        for sn in sessions:
            sn.graph = None
        _release(*streams)


def _dev(bits, dt):
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).cuda()


def _filled(size, it):
    return torch.full((size,), -7, dtype=it, device="cuda")


class _Feature:
    """One feature call of a worker: inputs made (and uploaded) in the main thread, `run(stream)` in the worker, `check()` in the
    main thread after the join -- against locate_lib / partition_lib / reduce_lib / join_lib."""

    def __init__(self, kind, dt, order, n, m, seed, ib):
        self.kind, self.dt, self.order, self.n, self.m, self.ib = kind, dt, order, n, m, ib
        self.tag = "%s[%s %s n=%d m=%d idx=%d]" % (kind, ol.DTYPE_NAMES[dt], "desc" if order else "asc", n, m, ib)
        it = torch.int32 if ib == 4 else torch.int64
        a = ol.splitmix_fill(n, dt, seed)
        if kind in ("locate", "partition"):
            # values / edges: half of them occur among the keys; locate's stay few (its search route), the partition's too
            self.a, self.vals = a, np.concatenate([a[:m // 2], ol.splitmix_fill(m - m // 2, dt, seed + 1)])
            self.src_t, self.vals_t = _dev(a, dt), _dev(self.vals, dt)
            if kind == "locate":
                self.outs = [_filled(m, it), _filled(m, it), _filled(n, it)]
            else:
                self.outs = [torch.full((n,), -7, dtype=self.src_t.dtype, device="cuda"), _filled(n, it), _filled(m + 2, it)]
        elif kind == "reduce":
            a = a.copy()
            a[::3] = a[0]                      # (groups of more than one row)
            self.a, self.vbits = a, rl.small_ints(n, ol.I64, seed + 2)
            self.src_t, self.vals_t = _dev(a, dt), _dev(self.vbits, ol.I64)
        else:
            mask = (1 << (8 * ol.DTYPE_SIZE[dt])) - 1
            base = ol.NP_BITS[dt](0x41 << (8 * ol.DTYPE_SIZE[dt] - 8))
            self.right = ol.splitmix_fill(m, dt, seed + 3, 0x0003FF00 & mask) | base      # about m / 1024 right rows per key
            self.left = ol.splitmix_fill(n, dt, seed + 4, 0x0007FF00 & mask) | base       # half of the left rows match nothing
            self.left_t, self.right_t = _dev(self.left, dt), _dev(self.right, dt)
            self.outs = [_filled(n, it), _filled(n, it), _filled(m, it)]
        self.rc = self.info = self.pairs = self.res = self.err = None

    def run(self, stream):
        with torch.cuda.stream(stream):
            if self.kind == "locate":
                self.rc, self.info = ll.call_device(self.src_t, self.n, self.vals_t, self.m, self.dt, self.order, self.ib, *self.outs,
                                                    flags=0, stream=stream)
            elif self.kind == "partition":
                self.rc, self.info = ptl.call_device(self.src_t, self.n, self.vals_t, self.m, self.dt, self.order, self.ib, *self.outs,
                                                     flags=rsa.PARTITION_BELOW, stream=stream)
            elif self.kind == "reduce":
                self.rc = 0
                self.res = rsa.radix_sort_reduce(self.src_t, self.vals_t, dtype=self.dt, val_dtype=ol.I64, order=self.order,
                                                 idx_dtype=torch.int32 if self.ib == 4 else torch.int64, sum=True, min=True, max=True,
                                                 counts=True, stream=stream)
            else:
                self.rc, self.pairs, self.info = jl.call_device(self.left_t, self.n, self.right_t, self.m, self.dt, self.order, self.ib,
                                                                *self.outs, flags=rsa.JOIN_LEFT, stream=stream)
            if self.rc != 0:
                self.err = rsa.lib().rsx_last_error()
        stream.synchronize()
        return self

    def check(self):
        assert self.rc == 0, (self.tag, self.rc, self.err)
        if self.kind == "locate":
            ll.check(self.tag, ll.Want(self.a, self.dt, self.order), self.vals, self.src_t, self.vals_t, *self.outs, False, self.info)
        elif self.kind == "partition":
            ptl.check(self.tag, ptl.Want(self.a, self.dt, self.order), self.vals, self.src_t, self.vals_t, *self.outs, True, self.info)
        elif self.kind == "reduce":
            keys, counts, sm, mn, mx, _ = self.res
            u = lambda t, ut: t.cpu().numpy().view(ut)
            iu = np.uint32 if self.ib == 4 else np.uint64
            got = (u(keys, ol.NP_BITS[self.dt]), u(counts, iu).astype(np.uint64), u(sm, np.uint64), u(mn, np.uint64), u(mx, np.uint64))
            il.compare_reduce(self.tag, got, rl.want_reduce(rl.groups(self.a, self.dt, self.order), self.vbits, ol.I64))
            assert np.array_equal(u(self.src_t, ol.NP_BITS[self.dt]), self.a) and np.array_equal(u(self.vals_t, np.uint64), self.vbits), \
                (self.tag, "an input was written")
        else:
            jl.check(self.tag, jl.Want(self.left, self.right, self.dt, self.order), *self.outs, self.pairs, self.info, True, None,
                     self.left_t, self.right_t)


# workers 0 and 1: locate / partition; workers 2 and 3: reduce / join.  (kind, n, m, idx bytes) -- m: values, edges or right rows
_FEATURE_LISTS = (
    (("locate", 90001, 200, 4), ("partition", 50003, 40, 8), ("locate", 300001, 300, 8), ("partition", 120001, 200, 4)),
    (("partition", 90001, 60, 4), ("locate", 50003, 100, 8), ("partition", 300001, 30, 8), ("locate", 70001, 250, 4)),
    (("reduce", 90001, 0, 4), ("join", 90001, 40003, 4), ("reduce", 300001, 0, 8), ("join", 50003, 70001, 8)),
    (("join", 70001, 30011, 8), ("reduce", 50003, 0, 8), ("join", 120001, 50021, 4), ("reduce", 200003, 0, 4)),
)


@pytest.mark.parametrize("dt,order", [(U32, ASC), (F64, DESC)], ids=["u32", "f64-desc"])
def test_threads_run_the_features(dt, order):
    """B, the features: workers 0 and 1 alternate rsx_sort_locate_device and rsx_sort_partition_device, workers 2 and 3
    rsx_sort_reduce_device and rsx_sort_join_device, each on a stream of its own behind a 20 ms spin; inputs are uploaded before
    the threads start and every answer is checked after they have joined."""
    streams = [torch.cuda.Stream() for _ in _FEATURE_LISTS]
    timeline = cl.Timeline()
    try:
        calls = [[_Feature(kind, dt, order, n, m, 9900 + 100 * w + 10 * i, ib) for i, (kind, n, m, ib) in enumerate(spec)]
                 for w, spec in enumerate(_FEATURE_LISTS)]
        torch.cuda.synchronize()

        def worker(w):
            def walk():
                rsa.spin(cl.SPIN_US, streams[w])
                for f in calls[w]:
                    timeline.call(f.run, streams[w], label=f.kind)
            return walk

        names = ["worker %d" % w for w in range(len(calls))]
        _threads([(names[w], worker(w)) for w in range(len(calls))])
        torch.cuda.synchronize()
        for w, fs in enumerate(calls):
            for f in fs:
                f.check()
        _assert_overlap(timeline, names)
    finally:
        _release(*streams)


# ---- C. one (device, stream) from four threads --------------------------------------------------------------------------------------
# (kind, j, n): radix_sort, radix_sort_pairs, radix_sort_rank, radix_sort_unique, radix_sort_inplace_async -- five calls per worker,
# each list with a small sort directly before a larger one, so that the shared workspace grows while the others wait for the lock
_SHARED = (
    (("keys_mid", 0, 5000), ("keys_mid", 1, 200003), ("pairs", 2, 30001), ("rank", 3, 50001), ("unique", 4, 40001)),
    (("pairs", 5, 7001), ("pairs", 6, il.N_ONE_LEVEL), ("keys_async", 7, 70001), ("unique", 8, 20011), ("keys_mid", 9, 60001)),
    (("rank", 0, 9001), ("rank", 1, 250007), ("unique", 2, 90001), ("keys_async", 3, 30011), ("pairs", 4, 40001)),
    (("keys_async", 5, 6001), ("keys_async", 6, il.N_ONE_LEVEL), ("keys_mid", 7, 100003), ("rank", 8, 20021), ("unique", 9, 150001)),
)


def test_four_threads_share_one_stream():
    """C. All four workers sort their own buffers on ONE side stream through the device entry points.  Such calls share a context
    and are serialised by its lock: every result is the oracle's, every tail and guard intact, while the
    context's buffers grow under the feet of the threads that wait."""
    s = torch.cuda.Stream()
    session = sq.Session(s, with_graph=False)
    lists = [[sq.make_step(kind, j, pos=9500 + 10 * w + i, n=n) for i, (kind, j, n) in enumerate(spec)] for w, spec in enumerate(_SHARED)]
    try:
        names = ["worker %d" % w for w in range(len(lists))]
        results = _threads([(names[w], (lambda w=w: [sq.run(step, session) for step in lists[w]])) for w in range(len(lists))])
        torch.cuda.synchronize()
        for w, (steps, res) in enumerate(zip(lists, results)):
            for step, (got, bufs) in zip(steps, res):
                try:
                    bufs.check_guards()
                except gl.GuardDamage as e:
                    raise AssertionError("%s, %s: %s" % (names[w], sq.describe(step), e))
                sq.check(step, got)
    finally:
        _release(s)


# ---- D. what belongs to the calling thread ------------------------------------------------------------------------------------------
HIST_FILL = 0xA5A5A5A5A5A5A5A5


def _digit_counts(a, dt, order):
    k = ol.kdf_keys(a, dt, order)
    kb = ol.DTYPE_SIZE[dt]
    return np.concatenate([np.bincount(((k >> k.dtype.type(8 * j)) & k.dtype.type(0xFF)).astype(np.int64), minlength=256)
                           for j in range(kb)]).astype(np.uint64)


def _sort_and_check(a, dt, order, stream, what):
    """A blocking rsx_sort_device of `a` on `stream`, against the oracle."""
    with torch.cuda.stream(stream):
        src = _dev(a, dt)
        aux = torch.zeros_like(src)
        res, info = rsa.radix_sort(src, aux, dtype=dt, order=order, stream=stream)
        stream.synchronize()
        got = sq._bits(res, ol.NP_BITS[dt])
    want, in_aux, _ = ol.oracle_sort(a, dt, order)
    assert info.result_in_aux == in_aux, (what, "returned buffer")
    il.same(what, "result", got, want)


@pytest.mark.parametrize("armed_sorts_first", [False, True], ids=["other-thread-sorts-first", "armed-thread-sorts-first"])
def test_armed_histogram_belongs_to_its_thread(armed_sorts_first):
    """D. rsx_capture_histogram arms the CALLING thread's next sort.  Thread 1 arms; thread 2 sorts on another stream and must
    neither consume the arm nor write the array (it is its fill pattern when thread 2's sort returns); thread 1's sort delivers
    the digit counts of ITS keys (np.bincount of oracle_lib.kdf_keys).  And the other way round: thread 1 arms and sorts first,
    thread 2's later sort captures nothing.  The order is fixed with events, not with sleeps."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a1, a2 = ol.splitmix_fill(90001, U32, 611), ol.splitmix_fill(70001, U32, 612, 0x00FFFFFF)
    hist = np.full(256 * 4, HIST_FILL, dtype=np.uint64)
    armed, other_done, mine_done = threading.Event(), threading.Event(), threading.Event()
    seen = {}

    def thread1():
        try:
            with rsa.capturing_histogram(hist):
                armed.set()
                if not armed_sorts_first:
                    assert other_done.wait(cl.LIMIT_S)
                    seen["before mine"] = hist.copy()
                _sort_and_check(a1, U32, ASC, s1, "the armed thread's sort")
                seen["after mine"] = hist.copy()
                mine_done.set()
                if armed_sorts_first:
                    assert other_done.wait(cl.LIMIT_S)
                    seen["after other"] = hist.copy()
        finally:
            armed.set()
            mine_done.set()

    def thread2():
        try:
            assert armed.wait(cl.LIMIT_S)
            if armed_sorts_first:
                assert mine_done.wait(cl.LIMIT_S)
            _sort_and_check(a2, U32, ASC, s2, "the other thread's sort")
        finally:
            other_done.set()

    try:
        _threads([("thread 1", thread1), ("thread 2", thread2)])
        want = _digit_counts(a1, U32, ASC)
        if not armed_sorts_first:
            assert np.all(seen["before mine"] == HIST_FILL), "another thread's sort consumed the arm or wrote the armed array"
        else:
            assert np.array_equal(seen["after other"], want), "another thread's later sort wrote the array"
        assert np.array_equal(seen["after mine"], want), "the armed thread did not receive the counts of its own keys"
        assert not np.array_equal(want, _digit_counts(a2, U32, ASC))
    finally:
        _release(s1, s2)


def test_last_error_belongs_to_its_thread():
    """D. Threads 1 and 2 make different refused calls (a bad dtype; an index of 3 bytes) while thread 3 sorts; each failing
    thread then reads its OWN message, and thread 3's is what it was when the worker began."""
    streams = [torch.cuda.Stream() for _ in range(3)]
    L = rsa.lib()
    n = 30000
    a = ol.splitmix_fill(n, U32, 621)
    src, out = _dev(a, U32), _filled(2 * n, torch.int32)
    torch.cuda.synchronize()
    res, info = C.c_void_p(), rsa.Info()
    refused = [threading.Event(), threading.Event()]
    sorted_once = threading.Event()

    def failing(i, call):
        def body():
            try:
                assert sorted_once.wait(cl.LIMIT_S)
                rc = call(C.c_void_p(streams[i].cuda_stream))
            finally:
                refused[i].set()
            assert refused[1 - i].wait(cl.LIMIT_S)          # (the other thread's message is written before this one is read)
            return rc, L.rsx_last_error()
        return body

    def sorting():
        before = L.rsx_last_error()
        _sort_and_check(ol.splitmix_fill(50001, F32, 622), F32, DESC, streams[2], "thread 3, first sort")
        sorted_once.set()
        assert refused[0].wait(cl.LIMIT_S) and refused[1].wait(cl.LIMIT_S)
        _sort_and_check(ol.splitmix_fill(70001, I64, 623), I64, ASC, streams[2], "thread 3, second sort")
        return before, L.rsx_last_error()

    try:
        r1, r2, r3 = _threads([
            ("thread 1", failing(0, lambda sp: L.rsx_sort_device(src.data_ptr(), out.data_ptr(), n, 99, 0, sp, C.byref(res), C.byref(info)))),
            ("thread 2", failing(1, lambda sp: L.rsx_sort_rank_device(src.data_ptr(), out.data_ptr(), n, U32, 3, 0, sp, C.byref(res),
                                                                     C.byref(rsa.Info())))),
            ("thread 3", sorting)])
        assert r1[0] == sq.EINVAL and r2[0] == sq.EINVAL, (r1, r2)
        assert b"rsx_sort_device" in r1[1] and b"rank" not in r1[1], ("thread 1 reads", r1[1])
        assert b"rank" in r2[1] and r2[1] != r1[1], ("thread 2 reads", r2[1])
        assert r3[0] == r3[1], ("thread 3's message changed while others failed", r3)
        assert np.array_equal(sq._bits(src, np.uint32), a) and bool((out == -7).all().item()), "a refused call wrote"
    finally:
        _release(*streams)


def test_two_threads_create_their_contexts_in_the_same_instant():
    """D. The process's first touch of two new streams, from two threads released by one barrier: both get working contexts."""
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    keys = [ol.splitmix_fill(5000, U32, 631 + i) for i in range(2)]
    try:
        _threads([("thread %d" % i, (lambda i=i: _sort_and_check(keys[i], U32, i, streams[i], "first touch, thread %d" % i)))
                  for i in range(2)])
        for i in range(2):
            _sort_and_check(keys[1 - i], U32, ASC, streams[i], "second sort on stream %d" % i)
    finally:
        _release(*streams)


def test_release_of_an_idle_stream_beside_sorting_threads():
    """D. Thread 1 releases its own stream five times -- nobody else is ever on it, the use include/rsx.h allows --, each release
    followed by a sort that creates the context again, while threads 2 to 4 keep sorting on theirs; afterwards every stream
    sorts."""
    streams = [torch.cuda.Stream() for _ in range(4)]
    sizes = (5000, 70001, 20011, 120001, 9001)
    keys = {(w, i): ol.splitmix_fill(n, (U32, F32, U64, I32)[w], 640 + 10 * w + i) for w in range(4) for i, n in enumerate(sizes)}
    dts = (U32, F32, U64, I32)

    def releasing():
        for i in range(5):
            streams[0].synchronize()
            rsa.release_stream(streams[0])
            _sort_and_check(keys[(0, i)], dts[0], i & 1, streams[0], "thread 1 after release %d" % i)

    def sorting(w):
        def body():
            for i in range(5):
                _sort_and_check(keys[(w, i)], dts[w], (w + i) & 1, streams[w], "thread %d, sort %d" % (w + 1, i))
        return body

    try:
        _threads([("thread 1", releasing)] + [("thread %d" % (w + 1), sorting(w)) for w in range(1, 4)])
        for w in range(4):
            _sort_and_check(keys[(w, 1)], dts[w], ASC, streams[w], "afterwards, stream %d" % w)
    finally:
        _release(*streams)
