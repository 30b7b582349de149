"""The blocking entry points on host arrays: rsx_sort_group, _rankdata, _topk, _nth, _locate, _reduce, _join, rsx_join_pairs and
rsx_sort_partition, which stage through one helper (staged_call, radix_sorting_amd/csrc/rsx_api.hpp) into the slots of one buffer of
the context, and rsx_sort_lex, which lays its columns out in the same buffer itself.  One table (CASES) drives four checks:

  host form = device form   the same call on host arrays and on device arrays, both through the host entry: bit-identical, and what
                            the feature's own tests/*_lib.py expects; u8 and u64 keys, 4- and 8-byte indices, n in {2, 33, 257, 4099}
                            (2: past every host shortcut; the others put n x 1, 4 and 8 bytes on both sides of a multiple of 256,
                            where a slot of the wrong width or padding would overlap its neighbour), second lengths {1, 3, 65}
  every subset of outputs   a slot's place depends on which arrays are there; n = 257
  mixed pointers            every array in turn of the other kind: -1, the one message, nothing written
  one buffer, many callers  a sequence on one context in which the staging buffer grows, serves smaller callers and grows again

Every host array lies between two 64-byte bands of 0xA5 and starts out as 0xA5 itself: what a call brings back is exactly what it
reports (n_groups, k, pairs), the rest of the array and the bands stay as they were."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import group_lib as gl
import join_lib as jl
import lex_lib as xl
import locate_lib as ll
import nth_lib as nl
import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa
import rankdata_lib as rkl
import reduce_lib as rdl
import topk_lib as tl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BAND, FILL = 64, 0xA5
MIXED = b"host and device pointers in one call"
UINT = {1: np.uint8, 4: np.uint32, 8: np.uint64}
# few enough distinct keys that groups have several members and joins have matches
MASK = {ol.U8: 0xFF, ol.U32: 0x00000FFF, ol.U64: 0x8000000000000F07}
P64 = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.synchronize()


def keys(dt, n, seed):
    return ol.splitmix_fill(n, dt, seed, MASK[dt])


class Buf:
    """`nbytes` bytes of the host's or the device's between two bands, all 0xA5 but for `data`."""

    def __init__(self, nbytes, device, data=None):
        a = np.full(nbytes + 2 * BAND, FILL, dtype=np.uint8)
        if data is not None:
            a[BAND:BAND + nbytes] = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.nbytes, self.device = nbytes, device
        self.store = torch.from_numpy(a).cuda() if device else a
        self.ptr = (self.store.data_ptr() if device else a.ctypes.data) + BAND

    def read(self):
        a = self.store.cpu().numpy() if self.device else self.store
        assert (a[:BAND] == FILL).all() and (a[BAND + self.nbytes:] == FILL).all(), "a band was written"
        return a[BAND:BAND + self.nbytes]


class Case:
    """One call: `ins` name -> array, `outs` name -> (elements of room, bytes each), in the order of the C signature;
    call(p) -> (rc, ret) on the pointers p[name] (None: absent); returned(ret) -> name -> elements brought back;
    want() -> name -> expected array, or (array, mask of the entries that are defined)."""

    def __init__(self, ins, outs, call, returned, want, needs=lambda present: True):
        self.ins, self.outs, self.call, self.returned, self.needs = ins, outs, call, returned, needs
        self.want = functools.lru_cache(maxsize=1)(want)


def case_group(dt, n, m, ib):
    kb, bits = ol.DTYPE_SIZE[dt], keys(dt, n, 11)

    def call(p):
        ng, info = C.c_size_t(0xDEAD), rsa.GroupInfo()
        rc = rsa.lib().rsx_sort_group(p["src"], n, dt, ol.ASC, p["inverse"], p["keys"], p["counts"], p["first"], ib, C.byref(ng), C.byref(info))
        return rc, ng.value

    def want():
        inv, k, cn, fi = gl.want_group(bits, dt)
        return {"inverse": inv, "keys": k, "counts": cn, "first": fi}

    return Case({"src": bits}, {"inverse": (n, ib), "keys": (n, kb), "counts": (n, ib), "first": (n, ib)}, call,
                lambda g: {"inverse": n, "keys": g, "counts": g, "first": g}, want)


def case_rankdata(dt, n, m, ib):
    bits = keys(dt, n, 21)

    def call(p):
        info = rsa.RankdataInfo()
        return rsa.lib().rsx_sort_rankdata(p["src"], n, dt, ol.ASC, p["place"], p["less"], p["equal"], ib, C.byref(info)), None

    return Case({"src": bits}, {"place": (n, ib), "less": (n, ib), "equal": (n, ib)}, call, lambda _: {"place": n, "less": n, "equal": n},
                lambda: dict(zip(("place", "less", "equal"), rkl.want_rankdata(bits, dt))))


def case_topk(dt, n, m, ib):
    kb, bits, k = ol.DTYPE_SIZE[dt], keys(dt, n, 31), min(m, n)

    def call(p):
        info = rsa.TopkInfo()
        return rsa.lib().rsx_sort_topk(p["src"], n, k, dt, ol.ASC, p["keys"], p["idx"], ib, C.byref(info)), None

    return Case({"src": bits}, {"keys": (k, kb), "idx": (k, ib)}, call, lambda _: {"keys": k, "idx": k},
                lambda: dict(zip(("keys", "idx"), tl.Want(bits, dt).first(k)[:2])))


def case_nth(dt, n, m, ib):
    kb, bits = ol.DTYPE_SIZE[dt], keys(dt, n, 41)
    ranks = np.array([(j * 7919 + 1) % n for j in range(m)], dtype=np.uint64)

    def call(p):
        n_less, n_equal, info = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64), rsa.NthInfo()
        rc = rsa.lib().rsx_sort_nth(p["src"], n, ranks.ctypes.data_as(P64), m, dt, ol.ASC, p["keys"], p["idx"], ib, n_less.ctypes.data_as(P64),
                                    n_equal.ctypes.data_as(P64), C.byref(info))
        return rc, None

    return Case({"src": bits}, {"keys": (m, kb), "idx": (m, ib)}, call, lambda _: {"keys": m, "idx": m},
                lambda: dict(zip(("keys", "idx"), nl.Want(bits, dt).at(ranks)[:2])))


def case_locate(dt, n, m, ib):
    bits, vals = keys(dt, n, 51), keys(dt, m, 52)

    def call(p):
        info = rsa.LocateInfo()
        return rsa.lib().rsx_sort_locate(p["src"], n, p["vals"], m, dt, ol.ASC, p["less"], p["equal"], p["bin"], ib, 0, C.byref(info)), None

    def want():
        w = ll.Want(bits, dt)
        less, equal = w.at(vals)
        return {"less": less, "equal": equal, "bin": w.bins(vals, False)}

    return Case({"src": bits, "vals": vals}, {"less": (m, ib), "equal": (m, ib), "bin": (n, ib)}, call, lambda _: {"less": m, "equal": m, "bin": n},
                want)


def case_reduce(dt, n, m, ib):
    # (values as wide as the indices are narrow: no two kinds of slot of the call have the same width)
    kb, vdt = ol.DTYPE_SIZE[dt], ol.U64 if ib == 4 else ol.U32
    vb, kbits, vbits = ol.DTYPE_SIZE[vdt], keys(dt, n, 61), ol.splitmix_fill(n, vdt, 62)

    def call(p):
        ng, info = C.c_size_t(0xDEAD), rsa.ReduceInfo()
        ops = (rdl.SUM if p["sum"] else 0) | (rdl.MIN if p["min"] else 0) | (rdl.MAX if p["max"] else 0)
        rc = rsa.lib().rsx_sort_reduce(p["keys"], p["vals"], n, dt, ol.ASC, vdt, ops, p["out_keys"], p["counts"], ib, p["sum"], p["min"], p["max"],
                                       C.byref(ng), C.byref(info))
        return rc, ng.value

    return Case({"keys": kbits, "vals": vbits}, {"out_keys": (n, kb), "counts": (n, ib), "sum": (n, 8), "min": (n, vb), "max": (n, vb)}, call,
                lambda g: dict.fromkeys(("out_keys", "counts", "sum", "min", "max"), g),
                lambda: dict(zip(("out_keys", "counts", "sum", "min", "max"), rdl.want_reduce(rdl.groups(kbits, dt), vbits, vdt))))


def case_join(dt, n, m, ib):
    left, right = keys(dt, n, 71), keys(dt, m, 72)

    def call(p):
        pairs, info = C.c_uint64(0xDEAD), rsa.JoinInfo()
        rc = rsa.lib().rsx_sort_join(p["left"], n, p["right"], m, dt, ol.ASC, p["start"], p["count"], p["right_perm"], ib, 0, C.byref(pairs),
                                     C.byref(info))
        assert rc != 0 or pairs.value == jl.Want(left, right, dt).n_pairs()
        return rc, None

    def want():
        w = jl.Want(left, right, dt)
        return {"start": (w.start, w.count > 0), "count": w.count, "right_perm": w.perm}   # (a start is defined where something matches)

    return Case({"left": left, "right": right}, {"start": (n, ib), "count": (n, ib), "right_perm": (m, ib)}, call,
                lambda _: {"start": n, "count": n, "right_perm": m}, want)


def case_join_pairs(dt, n, m, ib):
    w = jl.Want(keys(dt, n, 71), keys(dt, m, 72), dt)
    li, ri = w.pairs(left_join=True)
    cap = li.size + 5   # (room beyond the pairs there are: the tail stays as it was)

    def call(p):
        pairs = C.c_uint64(0xDEAD)
        rc = rsa.lib().rsx_join_pairs(p["start"], p["count"], p["right_perm"], n, m, ib, rsa.JOIN_LEFT, p["out_left"], p["out_right"], cap,
                                      C.byref(pairs))
        assert rc != 0 or pairs.value == li.size
        return rc, li.size

    return Case({"start": w.start.astype(UINT[ib]), "count": w.count.astype(UINT[ib]), "right_perm": w.perm.astype(UINT[ib])},
                {"out_left": (cap, ib), "out_right": (cap, ib)}, call, lambda pairs: {"out_left": pairs, "out_right": pairs},
                lambda: {"out_left": li, "out_right": ri})   # (no match: -1, all ones in either width)


def case_partition(dt, n, m, ib):
    kb, bits, edges = ol.DTYPE_SIZE[dt], keys(dt, n, 81), keys(dt, m, 82)

    def call(p):
        info = rsa.PartitionInfo()
        rc = rsa.lib().rsx_sort_partition(p["src"], n, p["edges"], m, dt, ol.ASC, p["keys"], p["idx"], p["offsets"], ib, 0, C.byref(info))
        return rc, None

    def want():
        idx, k, offsets = pl.Want(bits, dt).split(edges, False)
        return {"keys": k, "idx": idx, "offsets": offsets}

    return Case({"src": bits, "edges": edges}, {"keys": (n, kb), "idx": (n, ib), "offsets": (m + 2, ib)}, call,
                lambda _: {"keys": n, "idx": n, "offsets": m + 2}, want, needs=lambda present: "keys" in present or "idx" in present)


def case_lex(dt, n, m, ib):
    # three columns, the first and the last the same array: it is staged once
    a, b = keys(dt, n, 91), keys(dt, n, 92)

    def call(p):
        info = rsa.LexInfo()
        return rsa.lib().rsx_sort_lex(xl.lex_cols([p["a"], p["b"], p["a"]], [dt] * 3), 3, n, p["idx"], ib, C.byref(info)), None

    return Case({"a": a, "b": b}, {"idx": (n, ib)}, call, lambda _: {"idx": n}, lambda: {"idx": xl.want_perm([a, b, a], [dt] * 3)})


# name -> (the case's builder, whether the call has a second length)
CASES = {"group": (case_group, False), "rankdata": (case_rankdata, False), "topk": (case_topk, True), "nth": (case_nth, True),
         "locate": (case_locate, True), "reduce": (case_reduce, False), "join": (case_join, True), "join_pairs": (case_join_pairs, True),
         "partition": (case_partition, True), "lex": (case_lex, False)}


def run_form(c, device, present=None, other=None):
    """The call with every array the device's or the host's, but `other`, which is of the other kind; the outputs `present`
    (None: all).  Returns (rc, ret, message, the arrays)."""
    present = list(c.outs) if present is None else present
    bufs = {name: Buf(a.nbytes, device != (name == other), a) for name, a in c.ins.items()}
    for name in present:
        bufs[name] = Buf(c.outs[name][0] * c.outs[name][1], device != (name == other))
    torch.cuda.synchronize()
    rc, ret = c.call({name: bufs[name].ptr if name in bufs else None for name in itertools.chain(c.ins, c.outs)})
    err = rsa.lib().rsx_last_error()
    torch.cuda.synchronize()
    return rc, ret, err, bufs


def results(c, tag, device, present=None):
    """... a call that succeeds: name -> what was brought back.  The inputs, the bands and the arrays' tails are as they were."""
    rc, ret, err, bufs = run_form(c, device, present)
    assert rc == 0, (tag, rc, err)
    for name, a in c.ins.items():
        assert np.array_equal(bufs[name].read(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), (tag, name, "an input was written")
    back, got = c.returned(ret), {}
    for name in (c.outs if present is None else present):
        raw, k = bufs[name].read(), back[name] * c.outs[name][1]
        assert (raw[k:] == FILL).all(), (tag, name, "written beyond the %d elements brought back" % back[name])
        got[name] = raw[:k].copy().view(UINT[c.outs[name][1]])
    return got


def compare(tag, got, want):
    for name, g in got.items():
        w, defined = want[name] if isinstance(want[name], tuple) else (want[name], None)
        w = np.asarray(w).astype(g.dtype)
        assert g.size == w.size, (tag, name, g.size, w.size)
        if defined is not None:
            g, w = g[defined], w[defined]
        assert np.array_equal(g, w), (tag, name, np.flatnonzero(g != w)[:8], g[:8], w[:8])


@pytest.mark.parametrize("name", list(CASES))
def test_host_form_is_device_form(name):
    build, second = CASES[name]
    for dt, ib, n, m in itertools.product((ol.U8, ol.U64), (4, 8), (2, 33, 257, 4099), (1, 3, 65) if second else (0,)):
        tag = (name, ol.DTYPE_NAMES[dt], ib, n, m)
        c = build(dt, n, m, ib)
        host, device = results(c, tag + ("host",), False), results(c, tag + ("device",), True)
        compare(tag + ("host",), host, c.want())
        compare(tag + ("device",), device, c.want())
        for out in host:
            assert host[out].tobytes() == device[out].tobytes(), (tag, out, "the host form and the device form differ")


@pytest.mark.parametrize("name", list(CASES))
def test_every_subset_of_the_outputs(name):
    build, second = CASES[name]
    for dt, ib in itertools.product((ol.U8, ol.U64), (4, 8)):
        c = build(dt, 257, 3, ib)
        outs = list(c.outs)
        for r in range(1, len(outs) + 1):
            for present in itertools.combinations(outs, r):
                if c.needs(present):
                    tag = (name, ol.DTYPE_NAMES[dt], ib, present)
                    compare(tag, results(c, tag, False, list(present)), c.want())


@pytest.mark.parametrize("name", list(CASES))
def test_mixed_pointers(name):
    build, second = CASES[name]
    for dt, ib in ((ol.U8, 4), (ol.U64, 8)):
        c = build(dt, 33, 3, ib)
        for device, other in itertools.product((False, True), itertools.chain(c.ins, c.outs)):
            tag = (name, ol.DTYPE_NAMES[dt], ib, "device arrays" if device else "host arrays", other)
            rc, _, err, bufs = run_form(c, device, other=other)
            assert rc == -1 and MIXED in err, (tag, rc, err)
            for out in c.outs:
                assert (bufs[out].read() == FILL).all(), (tag, out, "an output was written")


def test_one_buffer_many_callers():
    """On one context: a reduce of 70000 u8 keys that asks for keys, counts and sums (13 bytes of slots per key), a top-10 of 300, a
    join and its pairs of 4099 rows a side, a partition of 70000 u64 keys with 8-byte indices (16 bytes of slots per key: the
    buffer grows again), and the reduce once more."""
    def host(tag, c, present=None):
        got = results(c, tag, False, present)
        compare(tag, got, c.want())
        return got

    reduce = case_reduce(ol.U8, 70000, 0, 4)
    first = host("reduce", reduce, ["out_keys", "counts", "sum"])
    host("topk", case_topk(ol.U32, 300, 10, 4))
    host("join", case_join(ol.U32, 4099, 4099, 4))
    host("join_pairs", case_join_pairs(ol.U32, 4099, 4099, 4))
    host("partition", case_partition(ol.U64, 70000, 3, 8))
    again = host("reduce again", reduce, ["out_keys", "counts", "sum"])
    for out in first:
        assert first[out].tobytes() == again[out].tobytes(), (out, "the second reduce differs from the first")
