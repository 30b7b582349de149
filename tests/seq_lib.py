"""Sequences of calls on one (device, stream) context: a vocabulary of steps, what each must deliver, and a walk through every
ordered pair of them (test_seq_lib_cpu.py, test_gpu_sequences.py).  TEST INFRASTRUCTURE ONLY.

A STEP is (kind, dtype, order, n, input style, index width, seed).  `expect(step)` is everything the call must deliver, computed
from the step's own input alone by the references the suite already has (the oracle's C restatements and the *_lib helpers) --
never from the code under test and never from what ran before it: the library keeps state from call to call (two alternating
sets of flags and histograms, tables "zeroed for the next call", back-off counters, shared scratch buffers), and the point of a
sequence is that none of it may show.  The route (rsx_info.hybrid) is NOT part of the expectation: it depends on the back-off,
which is history; `backoff_routes` restates that rule for the one test that follows it.

`run(step, session)` performs the call on the GPU (torch is only imported there), `check(step, got)` compares bit for bit.
Every buffer a call may write is allocated with PAD elements more than the call is told about, filled with FILL bytes, inside
guard bands (guard_lib): the bytes behind the n-th element (`tails`) and the guards must come back as they were.

`circuit(kinds)` is the closed walk that holds every ordered pair of kinds (A directly followed by B, A = B included) exactly
once: an Euler circuit of the complete digraph with loops, built by Hierholzer's algorithm in a fixed order.

The wrong_* generators turn a right answer into a plausible STALE one (something the previous call left behind); check() must
reject each (test_seq_lib_cpu.py)."""
import collections
import ctypes as C
import functools

import numpy as np

import group_lib as grl
import lex_lib as ll
import nth_lib as nl
import oracle_lib as ol
import pairs_lib as pl
import rankdata_lib as rdl
import topk_lib as tl
import unique_lib as ul

Step = collections.namedtuple("Step", "kind dt order n style idx_bytes seed")

FILL = 0x5A          # every byte of an output buffer before the call
PAD = 64             # elements behind the n the call is told about
EINVAL = -1          # RSX_EINVAL (include/rsx.h)
REC_BYTES, REC_KEY_AT = 12, 4
REPLAY_N, REPLAY_DT, REPLAY_ORDER = 50000, ol.U32, ol.ASC

ALL = tuple(range(10))
WIDE = (ol.U32, ol.U64, ol.I32, ol.I64, ol.F32, ol.F64)
NOHIST_N = 1 << 22

# kind -> (smallest n, largest n, key types)
SPEC = collections.OrderedDict([
    ("keys_small", (2, 4096, ALL)),                        # the one-launch sort
    ("keys_mid", (5000, 300001, ALL)),                     # blocking, histogram fused with the zeroing of the next sort's set
    ("keys_nohist", (NOHIST_N + 1, NOHIST_N + 9, WIDE)),   # a sort without a histogram (under the lowered floors, ENV)
    ("pairs", (2, 300001, ALL)),
    ("rank", (2, 300001, ALL)),
    ("keys_async", (2, 300001, ALL)),
    ("sub_async", (2, 300001, ALL)),                       # rank (even seed) or key + payload (odd seed), device-scheduled
    ("replay", (REPLAY_N, REPLAY_N, (REPLAY_DT,))),        # a graph captured when the sequence began, replayed on new keys
    ("unique", (2, 300001, ALL)),
    ("group", (2, 300001, ALL)),
    ("rankdata", (2, 300001, ALL)),
    ("topk", (200000, 300001, ALL)),
    ("nth", (1000, 300001, ALL)),
    ("lex", (2, 300001, ALL)),
    ("records", (2, 300001, ALL)),
    ("host", (2, 300001, ALL)),
    ("presorted", (2, 300001, ALL)),
    ("refused", (1000, 300001, WIDE)),
])
KINDS = tuple(SPEC)
# what the module-scoped fixture of test_gpu_sequences.py sets before its one rsx_reload_env
ENV = {"RSX_BLIND_MIN_LOG2": "22", "RSX_TWO_LEVEL_MIN_LOG2": "22", "RSX_LOG_MIN_LOG2": "20", "RSX_TOPK_FORCE": "1",
       "RSX_NTH_FORCE": "1"}

KEY_SORTS = ("keys_small", "keys_mid", "keys_nohist", "host", "presorted")   # out, aux, early_exit, result_in_aux, cols
FLAGGED = KEY_SORTS + ("pairs", "rank", "records")                            # kinds that report early_exit / result_in_aux
MAIN = {"pairs": "keys", "rank": "ranks", "unique": "keys", "group": "inverse", "rankdata": "place", "topk": "keys",
        "nth": "keys", "lex": "perm"}                                         # the main output where it is not "out"


# ---- the circuit ------------------------------------------------------------------------------------------------------------
def circuit(kinds):
    """The closed walk over `kinds` in which every ordered pair (a, b) -- b directly after a, a == b included -- occurs exactly
    once: len(kinds) ** 2 + 1 entries, first == last.  Hierholzer on the complete digraph with loops; the edges of a vertex are
    used in the order of `kinds`, so the same argument gives the same walk."""
    kinds = list(kinds)
    k = len(kinds)
    if k == 0:
        return []
    nxt = [0] * k                 # the next unused edge of each vertex: v -> nxt[v]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            walk.append(stack.pop())
    walk.reverse()
    return [kinds[v] for v in walk]


def pieces(walk, m):
    """The walk cut into pieces of about m steps; each piece begins with the last kind of the piece before it, so the pair across
    a cut is the first pair of the next piece."""
    if m < 2:
        raise ValueError("a piece holds at least one pair")
    out, i = [], 0
    while i < len(walk) - 1:
        out.append(walk[i:i + m])
        i += m - 1
    return out


M = 7    # steps per piece of the circuit: the references of a piece then take at most 1.5 s of CPU time (test_seq_lib_cpu.py)


def piece_steps(walk, m, i):
    """The steps of piece i of pieces(walk, m): those of the whole walk, so that a kind's types, orders and sizes rotate over the
    circuit and not over a piece."""
    return steps_of(walk)[i * (m - 1): i * (m - 1) + len(pieces(walk, m)[i])]


def steps_of(walk, salt=0):
    """A step for every entry of a walk of kinds.  The j-th occurrence of a kind takes the j-th of its key types and alternates
    the order so that a type meets both; its first occurrence has the smallest n of the kind, the second the largest, the
    others draw theirs; style, index width and seed follow from (salt, position)."""
    seen = collections.Counter()
    out = []
    for pos, kind in enumerate(walk):
        j = seen[kind]
        seen[kind] += 1
        out.append(make_step(kind, j, 1000 * salt + pos))
    return out


def make_step(kind, j, pos=0, n=None):
    lo, hi, dts = SPEC[kind]
    rng = np.random.default_rng([7, KINDS.index(kind), j, pos])
    dt = dts[j % len(dts)]
    order = (j // len(dts) + j) & 1
    if kind == "replay":
        order = REPLAY_ORDER
    if n is None:
        n = lo if j == 0 else hi if j == 1 else int(rng.integers(lo, hi + 1))
    style = int(rng.integers(0, 5))
    if kind == "keys_nohist":
        style = 0     # (even keys: anything else is turned away by the sample, and the kind would not be what its name says)
    idx_bytes = int(rng.choice([4, 8]))
    return Step(kind, dt, order, int(n), style, idx_bytes, int(rng.integers(1, 1 << 30)))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def keys_for(n, dt, style, seed):
    """test_gpu_fuzz._keys with the draws tied to the seed: 0 plain, 1 constant byte columns, 2 a random bit mask, 3 few distinct
    values, 4 nearly sorted bit patterns."""
    rng = np.random.default_rng([11, seed])
    size = ol.DTYPE_SIZE[dt]
    full = (1 << (8 * size)) - 1
    mask = full
    if style == 1:
        for b in range(size):
            if rng.random() < 0.4:
                mask &= ~(0xFF << (8 * b))
    elif style == 2:
        mask &= int(rng.integers(0, full, dtype=np.uint64, endpoint=True))
    a = ol.splitmix_fill(n, dt, seed, mask)
    if style == 3:
        pool = a[: max(1, int(rng.integers(1, 40)))]
        a = pool[rng.integers(0, len(pool), size=n)].copy()
    elif style == 4 and n:
        a = np.sort(a)
        for _ in range(int(rng.integers(0, 4))):
            i, j = rng.integers(0, n, size=2)
            a[i], a[j] = a[j], a[i]
    elif style == 5 and n:   # (the directed tests: every key the same; style 6, sorted by derived key, is made in inputs())
        a[:] = a[0]
    return a


def lex_second_dtype(dt):
    """a column type of another width than dt's"""
    return (ol.U16, ol.I32, ol.F64, ol.U8, ol.I16, ol.F32, ol.U64, ol.I8, ol.I64, ol.U32)[dt]


def refusal(step):
    return ("nth", "topk", "records")[step.seed % 3]


@functools.lru_cache(maxsize=4)
def inputs(step):
    """The step's inputs (numpy, bit patterns): `keys` always; by kind `vals`, `col1`, `k`, `ranks`, `records`."""
    a = keys_for(step.n, step.dt, step.style, step.seed)
    d = {"keys": a}
    rng = np.random.default_rng([13, step.seed])
    if step.kind == "presorted" or step.style == 6:
        a = d["keys"] = a[ol.stable_argsort_by_kdf(a, step.dt, step.order)]
    if step.kind in ("pairs", "sub_async"):
        d["vals"] = ol.splitmix_fill(step.n, ol.U32 if step.idx_bytes == 4 else ol.U64, step.seed + 1)
    elif step.kind == "lex":
        dt1 = lex_second_dtype(step.dt)
        d["col1"] = keys_for(step.n, dt1, (step.style + 1) % 4, step.seed + 2)
        if step.style != 3:      # (ties in the first column, so that the second one decides something)
            d["keys"] = a & ol.NP_BITS[step.dt](0x0F if ol.DTYPE_SIZE[step.dt] == 1 else 0xFF0F)
    elif step.kind == "topk":
        d["k"] = int(rng.integers(1, min(step.n, 5000) + 1))
    elif step.kind == "nth":
        d["ranks"] = np.array([0, step.n - 1, int(rng.integers(0, step.n))], dtype=np.uint64)
    elif step.kind == "records":
        rec = ol.splitmix_fill(step.n * REC_BYTES, ol.U8, step.seed + 3).reshape(step.n, REC_BYTES)
        kb = ol.DTYPE_SIZE[step.dt]
        rec[:, REC_KEY_AT:REC_KEY_AT + kb] = a.view(np.uint8).reshape(step.n, kb)
        d["records"] = rec
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- what a step must deliver ---------------------------------------------------------------------------------------------------
def _u64(x):
    return np.ascontiguousarray(x).astype(np.uint64)


def expect(step):
    """{name: value}: arrays as bit patterns (index arrays as uint64), flags as ints.  `tails`: "clean" -- every byte behind the
    n-th element of every buffer is still FILL."""
    inp = inputs(step)
    a, dt, order, n = inp["keys"], step.dt, step.order, step.n
    w = {"rc": 0, "tails": "clean"}
    kind = step.kind
    if kind in KEY_SORTS:
        out, in_aux, info = ol.oracle_sort(a, dt, order)
        w.update(out=out, result_in_aux=int(in_aux), early_exit=int(info.early_exit), cols=[int(c) for c in info.cols[:info.ncols]])
        if info.early_exit:
            w["aux"] = np.full(n * ol.DTYPE_SIZE[dt], FILL, dtype=np.uint8).view(ol.NP_BITS[dt])
    elif kind == "pairs":
        o = pl.Order(a, dt, order)
        w.update(keys=o.keys, vals=o.vals(inp["vals"]), result_in_aux=int(o.in_aux), early_exit=o.early_exit, cols=o.cols)
    elif kind == "rank":
        ranks, half, info, _ = ol.oracle_rank(a, dt, step.idx_bytes, order)
        w.update(ranks=_u64(ranks), result_in_aux=int(half), early_exit=int(info.early_exit))
    elif kind in ("keys_async", "replay"):
        w.update(out=ol.oracle_sort(a, dt, order)[0])
    elif kind == "sub_async":
        if step.seed % 2 == 0:
            w.update(ranks=_u64(ol.oracle_rank(a, dt, step.idx_bytes, order)[0]), src=a)
        else:
            o = pl.Order(a, dt, order)
            w.update(keys=o.keys, vals=o.vals(inp["vals"]))
    elif kind == "unique":
        keys, counts = ul.want_unique(a, dt, order)
        w.update(keys=keys, counts=_u64(counts), n_unique=int(keys.size))
    elif kind == "group":
        inverse, keys, counts, first = grl.want_group(a, dt, order)
        w.update(inverse=_u64(inverse), keys=keys, counts=_u64(counts), first=_u64(first), n_groups=int(keys.size), src=a)
    elif kind == "rankdata":
        place, less, equal = rdl.want_rankdata(a, dt, order)
        w.update(place=_u64(place), less=_u64(less), equal=_u64(equal), src=a)
    elif kind == "topk":
        keys, idx, kth, less, equal = tl.Want(a, dt, order).first(inp["k"])
        w.update(keys=keys, idx=_u64(idx), kth_key=int(kth), n_less=int(less), n_equal=int(equal), src=a)
    elif kind == "nth":
        keys, idx, less, equal = nl.Want(a, dt, order).at(inp["ranks"])
        w.update(keys=keys, idx=_u64(idx), n_less=_u64(less), n_equal=_u64(equal), src=a)
    elif kind == "lex":
        dts = [dt, lex_second_dtype(dt)]
        w.update(perm=_u64(ll.want_perm([a, inp["col1"]], dts, [order, order ^ 1])), src=a)
    elif kind == "records":
        s2 = np.array(inp["records"], copy=True)
        a2 = np.full_like(s2, FILL)
        info = ol.Info()
        r = ol.oracle().rso_sort_records(ol.ptr(s2), ol.ptr(a2), n, REC_BYTES, REC_KEY_AT, dt, order, C.byref(info))
        assert r in (0, 1)
        w.update(out=(a2 if r else s2).reshape(-1), result_in_aux=int(r), early_exit=int(info.early_exit))
    elif kind == "refused":
        w.update(rc=EINVAL, untouched=1)
    else:
        raise ValueError(kind)
    return w


def main_name(step):
    return MAIN.get(step.kind if step.kind != "sub_async" else ("rank" if step.seed % 2 == 0 else "pairs"), "out")


def _same(got, want):
    if isinstance(want, np.ndarray):
        g = np.ascontiguousarray(got)
        if g.dtype.itemsize != want.dtype.itemsize:
            return False
        g = g.view(want.dtype) if g.dtype != want.dtype else g
        return g.shape == want.shape and bool(np.array_equal(g, want))
    if isinstance(want, (list, tuple)):
        return list(got) == list(want)
    return int(got) == int(want)


def mismatches(step, got, want=None):
    """The names of what `got` gets wrong ([] = all right)."""
    want = expect(step) if want is None else want
    bad = []
    for name, w in want.items():
        if name not in got:
            bad.append(name + " (missing)")
        elif name == "tails":
            if not bool(np.all(np.asarray(got[name]) == FILL)):
                bad.append(name)
        elif not _same(got[name], w):
            bad.append(name)
    return bad


def check(step, got, want=None, before=None):
    """Bit for bit.  `before`: the step that ran directly before this one (named in the failure)."""
    bad = mismatches(step, got, want)
    assert not bad, "%s wrong after %s: %s" % (describe(step), "nothing" if before is None else describe(before), ", ".join(bad))


def describe(step):
    return "%s[%s %s n=%d style=%d idx=%d seed=%d]" % (step.kind, ol.DTYPE_NAMES[step.dt], "desc" if step.order else "asc", step.n,
                                                        step.style, step.idx_bytes, step.seed)


# ---- stale answers: each starts from the right one (want) and from what the step before delivered (prev_want) ---------------------
def _main_bytes(step, want):
    if step.kind == "refused":
        return np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(want[main_name(step)]).view(np.uint8).reshape(-1)


def wrong_stale_previous(step, want, prev, prev_want):
    """The previous step's output presented as this one's (cut or repeated to the length).  A refused call: as if it had run."""
    got = dict(want)
    if step.kind == "refused":
        got.update(rc=0, untouched=0)
        return got
    name = main_name(step)
    w = np.ascontiguousarray(want[name])
    old = _main_bytes(prev, prev_want)
    if old.size == 0 or w.size == 0:
        return None
    got[name] = np.resize(old, w.nbytes).view(w.dtype).reshape(w.shape)
    return got if not _same(got[name], w) else None


def wrong_stale_histogram(step, want, prev, prev_want):
    """A sorted array in which one value's count is one too high and another's one too low: the value comes from the previous
    step's input, as a histogram that was not zeroed would have it."""
    name = main_name(step)
    if name not in ("out", "keys") or step.kind in ("records", "topk", "nth", "refused", "group", "unique"):
        return None
    w = np.ascontiguousarray(want[name])
    pk = inputs(prev)["keys"]
    if w.size < 2 or pk.size == 0:
        return None
    v = np.resize(pk.view(np.uint8), w.dtype.itemsize).view(w.dtype)[0]
    mixed = np.concatenate([w[1:], np.array([v], dtype=w.dtype)])
    got = dict(want)
    got[name] = ol.oracle_sort(mixed, step.dt, step.order)[0]
    return got if not _same(got[name], w) else None


def wrong_stale_flag(step, want, prev, prev_want):
    """Right data with the previous step's early_exit / result_in_aux."""
    if step.kind not in FLAGGED or prev.kind not in FLAGGED:
        return None
    old = (prev_want["early_exit"], prev_want["result_in_aux"])
    if old == (want["early_exit"], want["result_in_aux"]):
        return None
    got = dict(want)
    got["early_exit"], got["result_in_aux"] = old
    return got


def wrong_stale_tail(step, want, prev, prev_want):
    """Everything the call was asked for is right, and behind it the entries of the previous, longer, result are still there."""
    old = _main_bytes(prev, prev_want)
    if step.kind == "refused" or old.size == 0:
        return None
    got = dict(want)
    mine = _main_bytes(step, want).size
    tail = np.resize(old[mine:] if old.size > mine else old, PAD * 8)
    if np.all(tail == FILL):
        return None
    got["tails"] = tail
    return got


WRONG = (wrong_stale_previous, wrong_stale_histogram, wrong_stale_flag, wrong_stale_tail)


def clean_answer(step, want):
    """The reference's own answer in the form run() reports: the tails as bytes."""
    got = dict(want)
    got["tails"] = np.full(PAD * 8, FILL, dtype=np.uint8)
    return got


# ---- the back-off of the attempts without a histogram (rsx_route_blind.hpp: blind_called_off, blind_wanted) ---------------------
def backoff_routes(lost, device=False):
    """lost[i]: would an attempt on input i be lost (a slot overflows after the sample let it through)?  Returns for every sort
    of the sequence whether it ATTEMPTS (True) or sits the attempt out.  The host's rule (blocking sorts): a lost attempt sets
    backoff = min(2 * backoff + 1, 31) and the context skips that many sorts of the kind; an attempt that is won resets backoff
    to 0.  device=True: the rule the device keeps for the device-scheduled sorts (rsx_hybrid.hpp, segctl_attempt_lost): 1, 2, 4
    .. 64 sorts are skipped."""
    backoff = skip = 0
    out = []
    for l in lost:
        if skip:
            skip -= 1
            out.append(False)
            continue
        out.append(True)
        if l and device:
            backoff = 1 if backoff == 0 else min(2 * backoff, 64)
            skip = backoff
        elif l:
            backoff = min(2 * backoff + 1, 31)
            skip = backoff
        else:
            backoff = 0
    return out


# ---- running a step on the GPU -----------------------------------------------------------------------------------------------
_CARRIER = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}


def _bits(t, ut):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(ut)


class Bufs:
    """The buffers of one step: each n + PAD elements of FILL bytes between guard bands of at least `guard` bytes."""

    def __init__(self, guard):
        self.guard = max(4096, (int(guard) + 255) & ~255)
        self.all = []

    def new(self, name, n, itemsize, data=None):
        import torch
        import guard_lib as gl
        g = gl.guarded(n + PAD, getattr(torch, _CARRIER[itemsize]), guard=self.guard)
        g.raw[g.start:g.end].fill_(FILL)
        if data is not None:
            d = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert d.size == n * itemsize, (name, d.size, n, itemsize)
            g.raw[g.start:g.start + d.size].copy_(torch.from_numpy(d.copy()))
        self.all.append((name, g, n))
        return g.t[:n]

    def ptr(self, name):
        return [g.t.data_ptr() for nm, g, _ in self.all if nm == name][0]

    def tails(self):
        import torch
        if not self.all:
            return np.zeros(0, dtype=np.uint8)
        return torch.cat([g.t[n:].contiguous().view(torch.uint8) for _, g, n in self.all]).cpu().numpy()

    def untouched(self):
        return int(all(bool((g.raw[g.start:g.end] == FILL).all().item()) for _, g, _ in self.all))

    def check_guards(self):
        import guard_lib as gl
        gl.check_all(*[(name, g) for name, g, _ in self.all])


class Session:
    """One sequence on one stream (None: the default stream, whose context the host-pointer entry points share).  At its start a
    keys-only rsx_sort_inplace_async of REPLAY_N keys is captured into a graph for the `replay` steps: on `stream` itself, i.e.
    on the context every other step of the sequence uses -- or, for the default stream, which cannot capture, on a stream of the
    session's own (the replays are then still ordered among the default stream's sorts, but use that other context).

    THE CONDITION of a graph on the library's own context ("Graphs and lifetimes"): nothing the graph names may
    move while it lives, i.e. no scratch buffer of the context may grow after the capture (a buffer that grows is freed and
    allocated anew).  A session whose graph shares its context with other steps is therefore given those steps (`sized_for`)
    and runs each of them once BEFORE the capture: every buffer of the context is then as large as any step of the sequence
    needs it -- a buffer only grows when more is asked of it than it holds (DevBuf::ensure), and the same step asks the same --
    so nothing is reallocated between the capture and the last replay.  (The context is then no longer fresh when the checked
    walk begins; the directed tests start from fresh contexts.)"""

    def __init__(self, stream=None, with_graph=True, sized_for=()):
        import torch
        import radix_sorting_amd as rsa
        self.stream = stream
        self.graph = None
        if not with_graph:
            return
        self.gstream = stream if stream is not None else torch.cuda.Stream()
        if stream is not None:
            for step in sized_for:
                if step.kind != "replay":
                    run(step, self)
            self.sync()
        self.gbufs = Bufs(REPLAY_N * 4)
        with torch.cuda.stream(self.gstream):
            self.gbuf = self.gbufs.new("graph buf", REPLAY_N, 4)
            self.gscratch = self.gbufs.new("graph scratch", REPLAY_N, 4)
            rsa.fill_splitmix(self.gbuf, seed=1, stream=self.gstream)
            rsa.radix_sort_inplace_async(self.gbuf, self.gscratch, dtype=REPLAY_DT, order=REPLAY_ORDER, stream=self.gstream)
        self.gstream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.gstream):
            rsa.radix_sort_inplace_async(self.gbuf, self.gscratch, dtype=REPLAY_DT, order=REPLAY_ORDER,
                                         stream=torch.cuda.current_stream())
        torch.cuda.synchronize()

    def sync(self):
        import torch
        if self.stream is None:
            torch.cuda.synchronize()
        else:
            self.stream.synchronize()


def run(step, session):
    """Perform the step on the session's stream; returns (got, bufs): `got` in the shape of expect(step), `bufs` for the guards."""
    import torch
    if session.stream is None:
        return _run(step, session)
    with torch.cuda.stream(session.stream):
        return _run(step, session)


def _run(step, session):
    import torch
    import radix_sorting_amd as rsa
    inp = inputs(step)
    a, dt, order, n, kind = inp["keys"], step.dt, step.order, step.n, step.kind
    kb, ib = ol.DTYPE_SIZE[dt], step.idx_bytes
    ut = ol.NP_BITS[dt]
    it = np.uint32 if ib == 4 else np.uint64
    idt = torch.int32 if ib == 4 else torch.int64
    s = session.stream
    sptr = C.c_void_p((s if s is not None else torch.cuda.current_stream()).cuda_stream)
    B = Bufs(n * kb)
    got = {"rc": 0}
    if kind in ("keys_small", "keys_mid", "keys_nohist", "presorted"):
        src, aux = B.new("src", n, kb, a), B.new("aux", n, kb)
        res, info = rsa.radix_sort(src, aux, dtype=dt, order=order, stream=s)
        session.sync()
        got.update(out=_bits(res, ut), aux=_bits(aux, ut), result_in_aux=info.result_in_aux, early_exit=info.early_exit,
                   cols=info.kept_columns(), route=info.hybrid)
    elif kind == "host":
        src = np.full(n + PAD, FILL * 0x0101010101010101 & ((1 << (8 * kb)) - 1), dtype=ut)
        aux = src.copy()
        src[:n] = a
        res, info = rsa.radix_sort_host(src[:n], aux[:n], dt, order)
        got.update(out=res.copy(), aux=aux[:n].copy(), result_in_aux=info.result_in_aux, early_exit=info.early_exit,
                   cols=info.kept_columns(), tails=np.concatenate([src[n:], aux[n:]]).view(np.uint8))
    elif kind == "pairs":
        k0, k1 = B.new("keys", n, kb, a), B.new("keys aux", n, kb)
        v0, v1 = B.new("vals", n, ib, inp["vals"]), B.new("vals aux", n, ib)
        kr, vr, info = rsa.radix_sort_pairs(k0, k1, v0, v1, dtype=dt, order=order, stream=s)
        session.sync()
        got.update(keys=_bits(kr, ut), vals=_bits(vr, it), result_in_aux=info.result_in_aux, early_exit=info.early_exit,
                   cols=info.kept_columns(), route=info.hybrid)
    elif kind == "rank":
        src = B.new("src", n, kb, a)
        ibuf = B.new("index buffer", 2 * n, ib)
        ranks, info = rsa.radix_sort_rank(src, ibuf, dtype=dt, order=order, stream=s)
        session.sync()
        got.update(ranks=_u64(_bits(ranks, it)), result_in_aux=info.result_in_aux, early_exit=info.early_exit, route=info.hybrid)
    elif kind == "keys_async":
        buf, scratch = B.new("buf", n, kb, a), B.new("scratch", n, kb)
        rsa.radix_sort_inplace_async(buf, scratch, dtype=dt, order=order, stream=s)
        session.sync()
        got.update(out=_bits(buf, ut))
    elif kind == "sub_async" and step.seed % 2 == 0:
        src = B.new("src", n, kb, a)
        ibuf = B.new("index buffer", 2 * n, ib)
        ranks = rsa.radix_sort_rank_inplace_async(src, ibuf, dtype=dt, order=order, stream=s)
        session.sync()
        got.update(ranks=_u64(_bits(ranks, it)), src=_bits(src, ut))
    elif kind == "sub_async":
        k0, k1 = B.new("keys", n, kb, a), B.new("keys scratch", n, kb)
        v0, v1 = B.new("vals", n, ib, inp["vals"]), B.new("vals scratch", n, ib)
        rsa.radix_sort_pairs_inplace_async(k0, k1, v0, v1, dtype=dt, order=order, stream=s)
        session.sync()
        got.update(keys=_bits(k0, ut), vals=_bits(v0, it))
    elif kind == "replay":
        B = session.gbufs
        session.gbuf.copy_(torch.from_numpy(a.view(np.int32).copy()).to(session.gbuf.device))
        session.graph.replay()
        session.sync()
        got.update(out=_bits(session.gbuf, ut))
    elif kind == "unique":
        src, aux, counts = B.new("src", n, kb, a), B.new("aux", n, kb), B.new("counts", n, ib)
        keys, cn, _ = rsa.radix_sort_unique(src, aux, dtype=dt, order=order, counts=counts, stream=s)
        session.sync()
        got.update(keys=_bits(keys, ut), counts=_u64(_bits(cn, it)), n_unique=int(keys.numel()))
    elif kind == "group":
        src = B.new("src", n, kb, a)
        outs = [B.new(name, n, size) for name, size in (("inverse", ib), ("keys", kb), ("counts", ib), ("first", ib))]
        inv, keys, cn, fi, _ = rsa.radix_sort_group(src, dtype=dt, order=order, idx_dtype=idt, inverse=outs[0], keys=outs[1],
                                                    counts=outs[2], first=outs[3], stream=s)
        session.sync()
        got.update(inverse=_u64(_bits(inv, it)), keys=_bits(keys, ut), counts=_u64(_bits(cn, it)), first=_u64(_bits(fi, it)),
                   n_groups=int(keys.numel()), src=_bits(src, ut))
    elif kind == "rankdata":
        src = B.new("src", n, kb, a)
        outs = [B.new(name, n, ib) for name in ("place", "less", "equal")]
        if n == 0:      # (torch gives an empty view a null pointer, and three null outputs are an error: the buffers' own addresses)
            rsa.check(rsa.lib().rsx_sort_rankdata_device(B.ptr("src"), 0, dt, order, B.ptr("place"), B.ptr("less"), B.ptr("equal"), ib,
                                                         sptr, C.byref(rsa.RankdataInfo())))
            pla, le, eq = outs
        else:
            pla, le, eq, _ = rsa.radix_sort_rankdata(src, dtype=dt, order=order, idx_dtype=idt, place=outs[0], less=outs[1],
                                                     equal=outs[2], stream=s)
        session.sync()
        got.update(place=_u64(_bits(pla, it)), less=_u64(_bits(le, it)), equal=_u64(_bits(eq, it)), src=_bits(src, ut))
    elif kind == "topk":
        k = inp["k"]
        src, keys, idx = B.new("src", n, kb, a), B.new("keys out", k, kb), B.new("idx out", k, ib)
        keys, idx, info = rsa.radix_sort_topk(src, k, dtype=dt, order=order, keys_out=keys, idx_out=idx, stream=s)
        session.sync()
        got.update(keys=_bits(keys, ut), idx=_u64(_bits(idx, it)), kth_key=info.kth_key, n_less=info.n_less, n_equal=info.n_equal,
                   src=_bits(src, ut), route=info.route)
    elif kind == "nth":
        r = inp["ranks"]
        src, keys, idx = B.new("src", n, kb, a), B.new("keys out", r.size, kb), B.new("idx out", r.size, ib)
        keys, idx, less, equal, info = rsa.radix_sort_nth(src, r, dtype=dt, order=order, keys_out=keys, idx_out=idx, stream=s)
        session.sync()
        got.update(keys=_bits(keys, ut), idx=_u64(_bits(idx, it)), n_less=less, n_equal=equal, src=_bits(src, ut), route=info.route)
    elif kind == "lex":
        dt1 = lex_second_dtype(dt)
        c0, c1 = B.new("column 0", n, kb, a), B.new("column 1", n, ol.DTYPE_SIZE[dt1], inp["col1"])
        out = B.new("idx out", n, ib)
        perm, _ = rsa.radix_sort_lex([c0, c1], orders=[order, order ^ 1], dtypes=[dt, dt1], idx_out=out, stream=s)
        session.sync()
        got.update(perm=_u64(_bits(perm, it)), src=_bits(c0, ut))
    elif kind == "records":
        src, aux = B.new("records", n * REC_BYTES, 1, inp["records"]), B.new("records aux", n * REC_BYTES, 1)
        res, info = rsa.radix_sort_records_tagged(src.view(torch.uint8), aux.view(torch.uint8), REC_BYTES, REC_KEY_AT, dt, order, stream=s)
        session.sync()
        got.update(out=_bits(res, np.uint8), result_in_aux=info.result_in_aux, early_exit=info.early_exit)
    elif kind == "refused":
        got.update(_refused(step, B, a, sptr))
        session.sync()
    else:
        raise ValueError(kind)
    if "tails" not in got:
        got["tails"] = B.tails()
    return got, B


def _refused(step, B, a, sptr):
    """A call the library must turn away with RSX_EINVAL before it writes anything: the C ABI itself (the Python wrappers would
    refuse first)."""
    import radix_sorting_amd as rsa
    n, dt, order, kb = step.n, step.dt, step.order, ol.DTYPE_SIZE[step.dt]
    lib = rsa.lib()
    what = refusal(step)
    if what == "records":
        rec = ol.splitmix_fill(n * REC_BYTES, ol.U8, step.seed + 3)
        src = B.new("records", n * REC_BYTES, 1, rec)
        outs = Bufs(n * kb)
        aux = outs.new("records aux", n * REC_BYTES, 1)
        res, info = C.c_void_p(), rsa.Info()
        rc = lib.rsx_sort_records_tagged_device(src.data_ptr(), aux.data_ptr(), n, REC_BYTES, REC_BYTES - kb + 1, dt, order, sptr,
                                                C.byref(res), C.byref(info))
        same = bool(np.array_equal(_bits(src, np.uint8), rec))
    else:
        src = B.new("src", n, kb, a)
        outs = Bufs(n * kb)
        keys, idx = outs.new("keys out", 8, kb), outs.new("idx out", 8, 4)
        if what == "topk":
            info = rsa.TopkInfo()
            rc = lib.rsx_sort_topk_device(src.data_ptr(), n, n + 1, dt, order, keys.data_ptr(), idx.data_ptr(), 4, sptr, C.byref(info))
        else:
            info = rsa.NthInfo()
            ranks = np.array([0, n, 1], dtype=np.uint64)
            less, equal = np.full(3, 0xA5, dtype=np.uint64), np.full(3, 0xA5, dtype=np.uint64)
            rc = lib.rsx_sort_nth_device(src.data_ptr(), n, rsa._u64p(ranks), 3, dt, order, keys.data_ptr(), idx.data_ptr(), 4,
                                         rsa._u64p(less), rsa._u64p(equal), sptr, C.byref(info))
            if not (np.all(less == 0xA5) and np.all(equal == 0xA5)):
                rc = 1000 + rc      # (written although refused)
        same = bool(np.array_equal(_bits(src, ol.NP_BITS[dt]), a))
    B.all += outs.all
    return {"rc": int(rc), "untouched": int(same and outs.untouched())}
