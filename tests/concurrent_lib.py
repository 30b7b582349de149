"""Concurrent calls: host threads behind a barrier, a timeline of their library calls, and the fixed work lists of the
threaded tests (test_concurrent_lib_cpu.py, test_gpu_concurrent.py).  TEST INFRASTRUCTURE ONLY.

`run_threads(workers, limit_s)` starts one daemon thread per (name, callable) and releases them together.  What a worker
returns or raises is collected with its traceback; the first exception is raised again in the caller as WorkerFailed, naming the
worker.  A thread that is still alive at its limit is something else than a failure: Hung names it, and the caller must start
nothing more on the GPU (the thread is a daemon and is left behind).

`Timeline` stamps time.perf_counter_ns() around every library call a worker makes; `overlaps(timeline)` counts, per worker, the
calls that intersect in time a call of ANOTHER worker.  An interval is half-open: a call that begins at the instant another one
ends does not overlap it.

`sort_lists()` are the steps of the four workers that sort on streams of their own (seq_lib steps, fixed, different per worker);
every expectation is seq_lib.expect's, computed from the step's own input after the threads have joined."""
import collections
import threading
import time
import traceback

import inner_lib as il
import seq_lib as sq

Outcome = collections.namedtuple("Outcome", "name value error trace hung")


class WorkerFailed(AssertionError):
    """A worker raised; `outcomes` holds every worker's Outcome."""

    def __init__(self, message, outcomes):
        AssertionError.__init__(self, message)
        self.outcomes = outcomes


class Hung(AssertionError):
    """A worker was still running at its limit; `names` says which, `outcomes` holds every worker's Outcome."""

    def __init__(self, message, names, outcomes):
        AssertionError.__init__(self, message)
        self.names = names
        self.outcomes = outcomes


def run_threads(workers, limit_s):
    """workers: [(name, callable without arguments)].  Returns their return values in that order.  Raises Hung if a worker is
    still alive `limit_s` seconds after the release (whatever else went wrong), else WorkerFailed for the first exception."""
    names = [name for name, _ in workers]
    assert len(set(names)) == len(names), "worker names must differ"
    barrier = threading.Barrier(len(workers))
    slots = {}
    lock = threading.Lock()

    def body(name, fn):
        value = error = trace = None
        try:
            barrier.wait(timeout=limit_s)
            value = fn()
        except BaseException as e:      # noqa: B902  (everything a worker raises belongs to the caller)
            error, trace = e, traceback.format_exc()
        with lock:
            slots[name] = (value, error, trace)

    threads = [threading.Thread(target=body, args=(name, fn), name=name, daemon=True) for name, fn in workers]
    start = time.monotonic()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, start + limit_s - time.monotonic()))
    outcomes = []
    for t in threads:
        with lock:
            done = slots.get(t.name)
        if done is None:
            outcomes.append(Outcome(t.name, None, None, None, True))
        else:
            outcomes.append(Outcome(t.name, done[0], done[1], done[2], False))
    hung = [o.name for o in outcomes if o.hung]
    failed = [o for o in outcomes if o.error is not None]
    if hung:
        raise Hung("worker(s) %s still running after %.1f s (hung, not failed)%s" % (
            ", ".join(hung), limit_s, "".join("; worker %s failed: %r" % (o.name, o.error) for o in failed)), hung, outcomes)
    if failed:
        o = failed[0]
        raise WorkerFailed("worker %s raised %s: %s\n%s" % (o.name, type(o.error).__name__, o.error, o.trace), outcomes) from o.error
    return [o.value for o in outcomes]


class Timeline:
    """{worker: [(begin_ns, end_ns, label)]}.  `call` stamps around one call; the worker is the calling thread's name (the name
    run_threads gave it) unless it is given."""

    def __init__(self):
        self.calls = collections.OrderedDict()
        self._lock = threading.Lock()

    def add(self, worker, begin_ns, end_ns, label=""):
        assert end_ns >= begin_ns, (worker, begin_ns, end_ns)
        with self._lock:
            self.calls.setdefault(worker, []).append((int(begin_ns), int(end_ns), label))

    def call(self, fn, *args, worker=None, label="", **kwargs):
        worker = threading.current_thread().name if worker is None else worker
        t0 = time.perf_counter_ns()
        try:
            return fn(*args, **kwargs)
        finally:
            self.add(worker, t0, time.perf_counter_ns(), label)


def overlaps(timeline):
    """{worker: how many of its calls intersect in time a call of another worker}."""
    out = collections.OrderedDict()
    for w, mine in timeline.calls.items():
        others = [iv for v, ivs in timeline.calls.items() if v != w for iv in ivs]
        out[w] = sum(1 for a0, a1, _ in mine if any(a0 < b1 and b0 < a1 for b0, b1, _ in others))
    return out


# ---- the work lists of the four sorting workers -----------------------------------------------------------------------------------
SPIN_US = 20000          # what every worker enqueues first: its first call then sits in the library that long
LIMIT_S = 60.0           # a hang detector, not a speed bound

# (kind, j, n) per worker; j picks type and order (seq_lib.make_step).  Sizes are the small ends of each kind's routes: the
# one-launch sort (4096), a look-back chain over a few quarter tiles (70001), one MSB pass and leaves (300001 where a list has
# it), and one sort without a histogram at its default size (inner_lib.N23).  Every list holds one pair of neighbouring sorts of
# different sizes, the smaller first, so that a context's buffers grow while other threads are inside the library.
_LISTS = (
    # worker 0: owns a graph on its stream's context (Session(with_graph=True, sized_for=its steps))
    (("keys_mid", 0, 70001), ("replay", 0, None), ("pairs", 1, 50001), ("keys_async", 2, 70001), ("replay", 1, None),
     ("unique", 3, 40001), ("sub_async", 4, 60001), ("replay", 2, None), ("presorted", 5, 70001), ("refused", 0, 30001)),
    # worker 1
    (("keys_nohist", 0, il.N23), ("keys_small", 1, 4096), ("rank", 2, 60001), ("group", 3, 50001), ("topk", 4, 200003),
     ("keys_async", 5, il.N_ONE_LEVEL), ("lex", 6, 40001), ("records", 7, 30001), ("refused", 1, 30001), ("keys_mid", 8, 120001)),
    # worker 2
    (("topk", 0, 200003), ("nth", 1, 90001), ("rankdata", 2, 50001), ("sub_async", 3, 70001), ("pairs", 4, il.N_ONE_LEVEL),
     ("keys_small", 5, 4096), ("unique", 6, 70001), ("presorted", 7, 50001), ("records", 8, 40001), ("rank", 9, 70001)),
    # worker 3
    (("lex", 0, 50001), ("group", 1, 70001), ("keys_mid", 2, 5000), ("keys_mid", 3, il.N_ONE_LEVEL), ("nth", 4, 70001),
     ("rankdata", 5, 60001), ("sub_async", 6, 50001), ("keys_async", 7, 4096), ("refused", 2, 30001), ("pairs", 8, 70001)),
)


def sort_lists():
    """[[seq_lib.Step]] for workers 0 .. 3.  sub_async takes both its forms: the rank sort for workers 0 and 2 (even seed),
    key + payload for worker 3."""
    out = []
    for w, spec in enumerate(_LISTS):
        steps = []
        for pos, (kind, j, n) in enumerate(spec):
            st = sq.make_step(kind, j, pos=9000 + 100 * w + pos, n=n)
            if kind == "sub_async":
                st = st._replace(seed=(st.seed & ~1) | (1 if w == 3 else 0))
            steps.append(st)
        out.append(steps)
    return out
