"""rsx_sort_partition_device on the GPU: the stable multi-way split of the keys by given edges, against NumPy on the oracle's
derived keys (partition_lib.Want.split: locate_lib's bins, np.argsort(kind="stable"), the keys read through it, the counts of
the bins scanned).

Every case runs on its natural route with the route and the ranking form asserted, and again on the forced sort route
(RSX_PARTITION_FORCE=2); keys, idx and offsets are compared with NumPy both times and src and edges must be bit-identical
afterwards.  The index width (4 / 8 bytes), the six subsets of the outputs (each of keys / idx / offsets missing in turn) and the
BELOW flag rotate over the cases instead of multiplying them; both orders run.  The derived keys are computed once per (keys,
dtype, order) and shared by every list of edges.  T is the tile of the count and of the placement, S the smallest number of keys
a workgroup owns (partition_lib.TILE, partition_lib.SHARE), B the seam between the two ranking forms in parts.  The cut-off between
the routes is pinned to 255 distinct edges (RSX_PARTITION_MAX_EDGES) wherever a test does not say otherwise: the library's default
is the lower, measured one (test_the_default_cut_off).  The route never depends on n, so every size meets the same route."""
import itertools

import numpy as np
import pytest

import locate_lib as ll
import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_IT = {4: torch.int32, 8: torch.int64}
_KT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SWITCHES = ("RSX_PARTITION_FORCE", "RSX_PARTITION_MAX_EDGES", "RSX_PARTITION_BALLOT_PARTS")
SUBSETS = [(True, True, True), (True, False, True), (False, True, True), (True, True, False), (True, False, False), (False, True, False)]
VARIANTS = [(ib, s, below) for (s, ib), below in zip(itertools.product(SUBSETS, (4, 8)), itertools.cycle((False, True, True, False, True)))]
T, S = pl.TILE, pl.SHARE


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    switch(monkeypatch)
    yield
    torch.cuda.synchronize()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()


def switch(monkeypatch, **values):
    """Set the switches named (FORCE, MAX_EDGES, BALLOT_PARTS), take every other one away -- but the cut-off, which is pinned to the
    most the scatter route takes (the library's default is lower: DESIGN.md 4q) unless MAX_EDGES="default" asks for the default."""
    values.setdefault("MAX_EDGES", rsa.PARTITION_MAX_EDGES)
    for name in SWITCHES:
        v = values.get(name[len("RSX_PARTITION_"):])
        if v is None or v == "default":
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    rsa.reload_env()


def to_dev(a, offset=0):
    """The bits on the device; offset: so many elements behind a 256-byte boundary."""
    a = np.ascontiguousarray(a)
    st = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]
    if not offset:
        return torch.from_numpy(a.view(st).copy()).cuda()
    room = torch.empty(a.size + 256, dtype=_KT[a.itemsize], device="cuda")
    skip = ((-room.data_ptr()) % 256) // a.itemsize + offset
    t = room[skip:skip + a.size]
    assert t.data_ptr() % 256 == offset * a.itemsize
    t.copy_(torch.from_numpy(a.view(st).copy()))
    return t


def run_case(tag, src_t, want, edges, idx_bytes=4, subset=(True, True, True), below=False, route=None, edges_t=None, seam=pl.BALLOT_PARTS):
    """One call, checked against NumPy; returns its info."""
    edges = np.ascontiguousarray(edges, dtype=ol.NP_BITS[want.dt])
    n, m = want.bits.size, edges.size
    if edges_t is None:
        edges_t = to_dev(edges)
    keys_t = torch.full((n,), 0x5A, dtype=_KT[ol.DTYPE_SIZE[want.dt]], device="cuda") if subset[0] else None
    idx_t = torch.full((n,), 0x5A, dtype=_IT[idx_bytes], device="cuda") if subset[1] else None
    off_t = torch.full((m + 2,), 0x5A, dtype=_IT[idx_bytes], device="cuda") if subset[2] else None
    rc, info = pl.call_device(src_t, n, edges_t, m, want.dt, want.order, idx_bytes, keys_t, idx_t, off_t, rsa.PARTITION_BELOW if below else 0)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    pl.check(tag, want, edges, src_t, edges_t, keys_t, idx_t, off_t, below, info, route, seam)
    return info


def both_routes(monkeypatch, tag, bits, dt, edge_lists, orders=(ol.ASC, ol.DESC), offset=0, rot=None, both_flags=False, seam=None):
    """Every list of edges in both orders, on the natural route and on the forced sort route; returns the natural route's infos."""
    bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    src_t = to_dev(bits, offset)
    wants = {o: pl.Want(bits, dt, o) for o in orders}
    rot = rot or itertools.cycle(VARIANTS)
    cases = []
    for o in orders:
        for i, edges in enumerate(edge_lists):
            edges = np.ascontiguousarray(edges(wants[o]) if callable(edges) else edges, dtype=ol.NP_BITS[dt])
            ib, subset, below = next(rot)
            for b in ((False, True) if both_flags else (below,)):
                cases.append((o, i, edges, to_dev(edges), (ib, subset, b)))
    infos = {}
    for force in (None, 2):
        switch(monkeypatch, FORCE=force, BALLOT_PARTS=seam)
        for o, i, edges, edges_t, (ib, subset, below) in cases:
            t = "%s n=%d list=%d m=%d order=%d ib=%d outs=%s below=%d force=%s" % (tag, bits.size, i, edges.size, o, ib, subset, below, force)
            route = rsa.PARTITION_SORT if force else pl.natural_route(edges, dt, o)
            info = run_case(t, src_t, wants[o], edges, ib, subset, below, route, edges_t, pl.BALLOT_PARTS if seam is None else seam)
            if not force:
                infos[(o, i, below)] = info
    return infos


# ---- lists of edges -------------------------------------------------------------------------------------------------------

def _splitters(k):
    """k quantile splitters taken from the keys themselves (so that keys sit ON the edges)"""
    def make(want):
        n = want.bits.size
        by = want.bits[np.argsort(want.kd, kind="stable")]
        return by[[(i + 1) * n // (k + 1) for i in range(k)]]
    return make


def _absent(k, seed):
    """k edges none of which occurs among the keys"""
    def make(want):
        cand = ol.splitmix_fill(4 * k + 64, want.dt, seed)
        cand = cand[~np.isin(ol.kdf_keys(cand, want.dt, want.order), want.sorted)]
        assert cand.size >= k
        return cand[:k]
    return make


def _in_k(*ks):
    """the edges whose derived keys are ks (negative: counted down from all-ones)"""
    def make(want):
        top = (1 << (8 * ol.DTYPE_SIZE[want.dt])) - 1
        return ll.from_kdf(np.array([k if k >= 0 else top + 1 + k for k in ks], dtype=np.uint64).astype(ol.NP_BITS[want.dt]), want.dt, want.order)
    return make


def _distinct(k, seed, repeat_to=0, descending=False):
    """k distinct edges in a shuffled order (repeat_to: repeated up to so many edges; descending: in descending order of the keys)"""
    def make(want):
        kb = ol.DTYPE_SIZE[want.dt]
        if kb == 1:
            v = np.arange(256, dtype=np.uint8).view(ol.NP_BITS[want.dt])
        else:
            v = np.unique(ol.splitmix_fill(k + k // 8 + 64, want.dt, seed))
        assert v.size >= k
        rng = np.random.default_rng(seed)
        v = rng.permutation(v)[:k]
        if repeat_to > k:
            v = rng.permutation(np.concatenate([v, v[rng.integers(0, k, size=repeat_to - k)]]))
        if descending:
            v = v[np.argsort(ol.kdf_keys(v, want.dt, want.order), kind="stable")[::-1]]
        return v
    return make


def small_lists(n):
    lists = [lambda w: w.bits[[n // 2]], _splitters(min(n, 3)), _in_k(0, -1)]
    lists.append(_splitters(255) if n >= 256 else _distinct(40, 7))
    return lists


SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, S - 1, S + 1, 2 * S + 3, 300001]


@pytest.mark.parametrize("dt", [ol.U32, ol.F32, ol.U64])
def test_sizes(dt, monkeypatch):
    rot = itertools.cycle(VARIANTS)
    for n in SIZES:
        infos = both_routes(monkeypatch, ol.DTYPE_NAMES[dt], ol.splitmix_fill(n, dt, 7100 + dt), dt, small_lists(n), rot=rot)
        assert all(i.route == rsa.PARTITION_SCATTER and i.shares == pl.shares(n, 0, ol.DTYPE_SIZE[dt]) for i in infos.values())


@pytest.mark.parametrize("dt", [ol.U32, ol.F32, ol.U64])
def test_src_one_element_behind_a_boundary(dt, monkeypatch):
    kb = ol.DTYPE_SIZE[dt]
    for n in (T + 2, 2 * S + 3, S + T + 16 // kb - 1):     # (the last: one share with the head, two without it)
        infos = both_routes(monkeypatch, "offset", ol.splitmix_fill(n, dt, 7200 + dt), dt, small_lists(n), offset=1)
        assert all(i.shares == pl.shares(n, kb, kb) for i in infos.values())


@pytest.mark.parametrize("dt", list(range(10)))
def test_all_dtypes(dt, monkeypatch):
    n = 65537
    lists = [lambda w: w.bits[[5]], _splitters(7), _distinct(255, 21), _distinct(200, 22, repeat_to=300)]
    infos = both_routes(monkeypatch, ol.DTYPE_NAMES[dt], ol.splitmix_fill(n, dt, 7300 + dt), dt, lists)
    for o in (ol.ASC, ol.DESC):
        got = [[i for (oo, li, _), i in infos.items() if oo == o and li == k][0] for k in range(4)]
        assert [i.route for i in got] == [rsa.PARTITION_SCATTER] * 4
        assert [i.distinct_edges for i in got][2:] == [255, 200]
        assert [i.rank_form for i in got] == [1, 2, 2, 2]


@pytest.mark.parametrize("dt", [ol.U32, ol.F32, ol.U64])
def test_the_shapes_of_the_edges(dt, monkeypatch):
    """1 edge (two parts), 255 distinct, 300 of which 200 are distinct (empty parts), descending edges, all edges below every key
    and all above, edges drawn from the keys (ties) -- each under both flags"""
    n = 2 * S + 3
    bits = ol.splitmix_fill(n, dt, 7400 + dt)
    kd = ol.kdf_keys(bits, dt, ol.ASC)
    bits = bits[(kd > kd.min()) & (kd < kd.max())]     # (room below and above every key in either order)
    top = (1 << (8 * ol.DTYPE_SIZE[dt])) - 1
    by_kdf = lambda w, ks: ll.from_kdf(np.array(ks, dtype=np.uint64).astype(ol.NP_BITS[dt]), dt, w.order)
    below_all = lambda w: by_kdf(w, [int(w.sorted[0]) - 1, 0, int(w.sorted[0]) - 1])
    above_all = lambda w: by_kdf(w, [int(w.sorted[-1]) + 1, top])
    lists = [lambda w: w.bits[[9]], _distinct(255, 31), _distinct(200, 32, repeat_to=300), _distinct(100, 33, descending=True), below_all, above_all,
             lambda w: w.bits[:97], _splitters(63)]
    infos = both_routes(monkeypatch, "shapes", bits, dt, lists, both_flags=True)
    for (o, li, below), i in infos.items():
        assert i.route == rsa.PARTITION_SCATTER
        if li == 0:
            assert (i.distinct_edges, i.rank_form) == (1, 1)
        if li == 2:
            assert i.distinct_edges == 200


def test_the_ballot_seam(monkeypatch):
    """B - 1, B and B + 1 parts with the seam pinned, and with the default; every part count on either form"""
    dt, n = ol.U32, S + T + 77
    bits = ol.splitmix_fill(n, dt, 7500)
    for seam in (6, None):
        b = pl.BALLOT_PARTS if seam is None else seam
        lists = [_splitters(b - 2), _splitters(b - 1), _splitters(b)]
        infos = both_routes(monkeypatch, "seam %s" % seam, bits, dt, lists, orders=(ol.ASC,), seam=seam)
        assert [infos[(ol.ASC, k, bl)].rank_form for (_, k, bl) in sorted(infos)] == [1, 1, 2]
    for seam, form in ((0, 2), (256, 1)):
        lists = [_splitters(1), _splitters(16), _distinct(255, 41)]
        infos = both_routes(monkeypatch, "seam %d" % seam, bits, dt, lists, orders=(ol.DESC,), seam=seam)
        assert all(i.rank_form == form for i in infos.values())


@pytest.mark.parametrize("dt", [ol.U32, ol.F64])
def test_all_keys_equal(dt, monkeypatch):
    """one bin holds whole tiles, on either ranking form"""
    n = 2 * S + 9
    bits = np.full(n, 0x40490FDB, dtype=ol.NP_BITS[dt])
    lists = [lambda w: w.bits[[0]], _in_k(0, -1), lambda w: np.concatenate([w.bits[[0]], _absent(254, 51)(w)])]
    for seam in (None, 0, 256):
        both_routes(monkeypatch, "equal keys seam=%s" % seam, bits, dt, lists, both_flags=True, seam=seam)


@pytest.mark.parametrize("dt", [ol.U32, ol.I64])
def test_keys_already_in_order(dt, monkeypatch):
    n = 2 * S + 3
    bits = ol.splitmix_fill(n, dt, 7600 + dt)
    bits = bits[np.argsort(ol.kdf_keys(bits, dt, ol.ASC), kind="stable")]
    infos = both_routes(monkeypatch, "in order", bits, dt, [_splitters(1), _splitters(15), _splitters(255)], both_flags=True)
    # the keys are in order (ascending) or in reverse order (descending): in order the split moves nothing
    want = pl.Want(bits, dt, ol.ASC)
    assert np.array_equal(want.split(_splitters(15)(want), False)[0], np.arange(n, dtype=np.uint64)) and len(infos) == 12


@pytest.mark.parametrize("dt", [ol.F32, ol.F64])
def test_floats_with_nans_and_zeros(dt, monkeypatch):
    n = S + 1003
    kb = ol.DTYPE_SIZE[dt]
    bits = ol.splitmix_fill(n, dt, 7700 + dt)
    sign, expo = 1 << (8 * kb - 1), (0x7F800000 if kb == 4 else 0x7FF0000000000000)
    special = np.array([0, sign, expo, expo | sign, expo | 1, expo | sign | 1, expo | (expo >> 1), expo | sign | (expo >> 1)], dtype=ol.NP_BITS[dt])
    bits[5:5 + 8 * 20] = np.tile(special, 20)
    lists = [special, special[:2], special[::-1][:3], lambda w: np.concatenate([special, _absent(100, 53)(w)]), _splitters(255)]
    both_routes(monkeypatch, "floats", bits, dt, lists, both_flags=True)


@pytest.mark.parametrize("dt", [ol.U32, ol.U64, ol.U16])
def test_edges_that_take_the_sort_route(dt, monkeypatch):
    n = 2 * S + 3
    bits = ol.splitmix_fill(n, dt, 7800 + dt)
    lists = [_distinct(256, 61), _distinct(4097, 62), _distinct(255, 63)]
    infos = both_routes(monkeypatch, "many edges", bits, dt, lists, both_flags=True)
    for (o, li, below), i in infos.items():
        assert i.route == (rsa.PARTITION_SORT, rsa.PARTITION_SORT, rsa.PARTITION_SCATTER)[li]
        assert li == 2 or i.distinct_edges > 255


def test_a_lowered_cut_off(monkeypatch):
    """RSX_PARTITION_MAX_EDGES=k: k distinct edges scatter, k + 1 sort -- whatever n is"""
    dt = ol.U32
    for n in (5, S + 77):
        bits = ol.splitmix_fill(n, dt, 7900)
        want = pl.Want(bits, dt)
        src_t = to_dev(bits)
        switch(monkeypatch, MAX_EDGES=33)
        assert run_case("k", src_t, want, _distinct(33, 44)(want), route=rsa.PARTITION_SCATTER).distinct_edges == 33
        assert run_case("k + 1", src_t, want, _distinct(34, 45)(want), route=rsa.PARTITION_SORT).distinct_edges == 34
        switch(monkeypatch, MAX_EDGES=1)
        run_case("1", src_t, want, bits[[3, 3, 3]], route=rsa.PARTITION_SCATTER)
        run_case("2", src_t, want, np.array([7, 9], dtype=np.uint32), route=rsa.PARTITION_SORT)


def test_the_default_cut_off(monkeypatch):
    """no switch set: RSX_PARTITION_DEFAULT_MAX_EDGES distinct edges scatter, one more sort -- whatever n is"""
    dt, k = ol.U32, rsa.PARTITION_DEFAULT_MAX_EDGES
    switch(monkeypatch, MAX_EDGES="default")
    for n in (9, S + T + 5):
        bits = ol.splitmix_fill(n, dt, 7950)
        want = pl.Want(bits, dt)
        src_t = to_dev(bits)
        assert run_case("k", src_t, want, _distinct(k, 46, repeat_to=k + 9)(want), route=rsa.PARTITION_SCATTER).distinct_edges == k
        assert run_case("k + 1", src_t, want, _distinct(k + 1, 47)(want), route=rsa.PARTITION_SORT).distinct_edges == k + 1
    info, _, _, off, _ = rsa.partition_even(src_t, k + 1, dtype=rsa.U32)
    assert info.route == rsa.PARTITION_SCATTER and [int(x) for x in off.cpu()][-1] == bits.size
    info, _, _, off, _ = rsa.partition_even(src_t, k + 2, dtype=rsa.U32)
    assert info.route == rsa.PARTITION_SORT and [int(x) for x in off.cpu()][-1] == bits.size


def test_no_edges_and_no_keys():
    """m == 0: one part -- the keys copied, idx = 0 .. n-1, offsets = {0, n}; n == 0: the offsets all zero, nothing else written"""
    bits = ol.splitmix_fill(70001, ol.U64, 8000)
    src_t = to_dev(bits)
    want = pl.Want(bits, ol.U64, ol.DESC)
    for ib, subset in ((4, (True, True, True)), (8, (False, True, True)), (8, (True, False, False))):
        info = run_case("m == 0", src_t, want, bits[:0], ib, subset, route=rsa.PARTITION_TRIVIAL, edges_t=src_t[:0])
        assert (info.input_reads, info.distinct_edges, info.rank_form, info.shares) == (0, 0, 0, 0)
    edges_t = to_dev(bits[:3])
    keys_t, idx_t, off_t = (torch.full((c,), 0x5A, dtype=torch.int64, device="cuda") for c in (4, 4, 5))
    rc, info = pl.call_device(src_t, 0, edges_t, 3, ol.U64, ol.ASC, 8, keys_t, idx_t, off_t)
    assert rc == 0 and info.route == rsa.PARTITION_TRIVIAL
    torch.cuda.synchronize()
    assert not off_t.any() and (keys_t == 0x5A).all() and (idx_t == 0x5A).all()


@pytest.mark.parametrize("parts", [2, 7, 64, 65])
def test_partition_even(parts):
    """on a permutation the parts are exactly even; with heavy ties the offsets are nth's n_less"""
    n = 100003
    perm = np.random.default_rng(parts).permutation(n).astype(np.uint32)
    info, keys, idx, off, spl = rsa.partition_even(to_dev(perm), parts, dtype=rsa.U32, idx=True)
    torch.cuda.synchronize()
    assert info.route == rsa.PARTITION_SCATTER
    assert [int(x) for x in off.cpu()] == [i * n // parts for i in range(parts + 1)]
    want = pl.Want(perm, ol.U32)
    pl.check("even", want, spl.cpu().numpy().view(np.uint32), None, None, keys, idx, off, False, info, rsa.PARTITION_SCATTER)
    ties = (ol.splitmix_fill(n, ol.I32, 8100 + parts).view(np.int32) % 11).astype(np.int32)
    src_t = to_dev(ties)
    ranks = [i * n // parts for i in range(1, parts)]
    _, _, n_less, _, _ = rsa.radix_sort_nth(src_t, ranks, dtype=rsa.I32, want_idx=False)
    info, keys, _, off, spl = rsa.partition_even(src_t, parts, dtype=rsa.I32)
    torch.cuda.synchronize()
    assert [int(x) for x in off.cpu()] == [0] + [int(x) for x in n_less] + [n]
    pl.check("even ties", pl.Want(ties.view(np.uint32), ol.I32), spl.cpu().numpy().view(np.uint32), None, None, keys, None, off, False, info)


def test_the_python_wrappers():
    a = ol.splitmix_fill(50001, ol.I32, 8200)
    src = to_dev(a)
    e = np.concatenate([a[:20], ol.splitmix_fill(30, ol.I32, 8201)])
    want = pl.Want(a, ol.I32)
    for below in (False, True):
        info, keys, idx, off = rsa.radix_sort_partition(src, to_dev(e), idx=True, below=below)
        torch.cuda.synchronize()
        pl.check("wrapper", want, e, src, None, keys, idx, off, below, info, rsa.PARTITION_SCATTER)
        bins = torch.bucketize(torch.from_numpy(a.view(np.int32).copy()), torch.from_numpy(np.sort(e.view(np.int32))), right=not below)
        assert torch.equal(idx.cpu().to(torch.int64), torch.sort(bins, stable=True).indices)
        info, keys, idx, off = rsa.radix_sort_partition_host(a, e, rsa.I32, idx=True, below=below, idx_dtype=np.uint64)
        pl.check("host", want, e, None, None, keys, idx, off, below, info, rsa.PARTITION_SCATTER)
    info, keys, idx, off = rsa.radix_sort_partition_host(a, e[:0], rsa.I32, idx=True)
    assert info.route == rsa.PARTITION_TRIVIAL and np.array_equal(keys, a) and np.array_equal(idx, np.arange(a.size)) and list(off) == [0, a.size]
    with pytest.raises(rsa.RsxError, match="out_keys is src"):
        rsa.radix_sort_partition(src, to_dev(e), keys=src)


def test_a_capturing_stream_is_refused():
    bits = ol.splitmix_fill(4095, ol.U32, 8300)
    want = pl.Want(bits, ol.U32)
    edges = ol.splitmix_fill(10, ol.U32, 8301)
    a, v = to_dev(bits), to_dev(edges)
    keys_t = torch.zeros(4095, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc, info = pl.call_device(a, 4095, v, 10, ol.U32, ol.ASC, 4, keys_t, None, None, 0, s)     # (the context of this stream exists before the capture)
        assert rc == 0, rsa.lib().rsx_last_error()
    s.synchronize()
    pl.check("before the capture", want, edges, a, v, keys_t, None, None, False, info, rsa.PARTITION_SCATTER)
    keys_t.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, _ = pl.call_device(a, 4095, v, 10, ol.U32, ol.ASC, 4, keys_t, None, None, 0, torch.cuda.current_stream())
        err = rsa.lib().rsx_last_error()
    assert rc == -1 and b"capturing" in err
    torch.cuda.synchronize()
    assert not keys_t.any()
    rsa.lib().rsx_release_stream(s.cuda_stream)
