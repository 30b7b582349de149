"""rsx_sort_locate_device on the GPU: where given values fall in the sorted order of the keys, against NumPy on the oracle's
derived keys (locate_lib.Want: np.sort, np.searchsorted left / right).

Every case runs on its natural route with the route asserted and on the forced sort route (RSX_LOCATE_FORCE=2); less, equal and
the bins are compared with NumPy and src and vals must be bit-identical afterwards.  The index width (4 / 8 bytes), the seven
subsets of the outputs and the BELOW flag rotate over the cases instead of multiplying them; both orders run.  The sorted
derived keys are computed once per (keys, dtype, order) and shared by every list of values.  T is the search kernel's tile, a
share the smallest number of keys a workgroup owns (locate_lib.TILE, locate_lib.SHARE)."""
import itertools

import numpy as np
import pytest

import locate_lib as ll
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_IT = {4: torch.int32, 8: torch.int64}
SWITCHES = ("RSX_LOCATE_FORCE", "RSX_LOCATE_MAX_VALUES", "RSX_LOCATE_COUNTER_SETS")
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if any(s)]      # (less, equal, bins): seven of them
VARIANTS = [(ib, s, below) for (s, ib), below in zip(itertools.product(SUBSETS, (4, 8)), itertools.cycle((False, True, True, False, True)))]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()


def switch(monkeypatch, **values):
    """Set the switches named (FORCE, MAX_VALUES, COUNTER_SETS), take every other one away."""
    for name in SWITCHES:
        v = values.get(name[len("RSX_LOCATE_"):])
        if v is None:
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
    room = torch.empty(a.size + 256, dtype=torch.from_numpy(np.zeros(0, dtype=st)).dtype, device="cuda")
    skip = ((-room.data_ptr()) % 256) // a.itemsize + offset
    t = room[skip:skip + a.size]
    assert t.data_ptr() % 256 == offset * a.itemsize
    t.copy_(torch.from_numpy(a.view(st).copy()))
    return t


def run_case(tag, src_t, want, vals, idx_bytes=4, subset=(True, True, True), below=False, route=None, vals_t=None):
    """One call, checked against NumPy; returns its info."""
    vals = np.ascontiguousarray(vals, dtype=ol.NP_BITS[want.dt])
    n, m = want.bits.size, vals.size
    if vals_t is None:
        vals_t = to_dev(vals)
    new = lambda count: torch.full((count,), 0x5A, dtype=_IT[idx_bytes], device="cuda")
    less_t = new(m) if subset[0] else None
    equal_t = new(m) if subset[1] else None
    bin_t = new(n) if subset[2] else None
    rc, info = ll.call_device(src_t, n, vals_t, m, want.dt, want.order, idx_bytes, less_t, equal_t, bin_t,
                              rsa.LOCATE_BINS_BELOW if below else 0)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    ll.check(tag, want, vals, src_t, vals_t, less_t, equal_t, bin_t, below, info, route)
    return info


def natural_route(dt, vals, order):
    if ol.DTYPE_SIZE[dt] <= 2:
        return rsa.LOCATE_TABLE
    return rsa.LOCATE_SEARCH if ll.search_shape(vals, dt, order)[0] <= rsa.LOCATE_MAX_SEARCH_VALUES else rsa.LOCATE_SORT


def both_routes(monkeypatch, tag, bits, dt, value_lists, orders=(ol.ASC, ol.DESC), offset=0, rot=None):
    """Every list of values in both orders, on the natural route and on the forced sort route; returns the natural route's infos."""
    bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    src_t = to_dev(bits, offset)
    wants = {o: ll.Want(bits, dt, o) for o in orders}
    rot = rot or itertools.cycle(VARIANTS)
    cases = []
    for o in orders:
        for i, vals in enumerate(value_lists):
            vals = np.ascontiguousarray(vals(wants[o]) if callable(vals) else vals, dtype=ol.NP_BITS[dt])
            cases.append((o, i, vals, to_dev(vals), next(rot)))
    infos = {}
    for force in (None, 2):
        switch(monkeypatch, FORCE=force)
        for o, i, vals, vals_t, (ib, subset, below) in cases:
            t = "%s n=%d list=%d m=%d order=%d ib=%d outs=%s below=%d force=%s" % (tag, bits.size, i, vals.size, o, ib, subset, below, force)
            route = rsa.LOCATE_SORT if force else natural_route(dt, vals, o)
            info = run_case(t, src_t, wants[o], vals, ib, subset, below, route, vals_t)
            if not force:
                infos[(o, i)] = info
    return infos


# ---- lists of values ------------------------------------------------------------------------------------------------------

def ones(dt):
    return (1 << (8 * ol.DTYPE_SIZE[dt])) - 1


def splitters(k):
    """k quantile splitters taken from the keys themselves (so that keys sit ON the edges)"""
    def make(want):
        n = want.bits.size
        by = want.bits[np.argsort(want.kd, kind="stable")]
        return by[[(i + 1) * n // (k + 1) for i in range(k)]]
    return make


def absent(k, seed):
    """k values none of which occurs among the keys"""
    def make(want):
        cand = ol.splitmix_fill(4 * k + 64, want.dt, seed)
        cand = cand[~np.isin(ol.kdf_keys(cand, want.dt, want.order), want.sorted)]
        assert cand.size >= k
        return cand[:k]
    return make


def in_k(*ks):
    """the values whose derived keys are ks (negative: counted down from all-ones)"""
    def make(want):
        top = ones(want.dt)
        return ll.from_kdf(np.array([k if k >= 0 else top + 1 + k for k in ks], dtype=np.uint64).astype(ol.NP_BITS[want.dt]), want.dt, want.order)
    return make


def one_digit(count):
    """`count` edges inside one digit of the start table and one far above them: the longest search for that many edges"""
    def make(want):
        top = ones(want.dt)
        ks = np.concatenate([np.arange(count, dtype=np.uint64) * np.uint64(3) + np.uint64(1000), np.array([top - 5], dtype=np.uint64)])
        return ll.from_kdf(ks.astype(ol.NP_BITS[want.dt]), want.dt, want.order)
    return make


def distinct(k, seed, repeat_to=0):
    """k distinct values in a shuffled order (repeat_to: repeated up to so many values)"""
    def make(want):
        v = np.unique(ol.splitmix_fill(k + k // 8 + 64, want.dt, seed))
        assert v.size >= k
        rng = np.random.default_rng(seed)
        v = rng.permutation(v)[:k]
        if repeat_to > k:
            v = rng.permutation(np.concatenate([v, v[rng.integers(0, k, size=repeat_to - k)]]))
        return v
    return make


def small_lists(n):
    lists = [lambda w: w.bits[[n // 2]], lambda w: w.bits[[0, 0]], in_k(0, 1, 2), in_k(-1, -2), in_k(0, -1), absent(256, 31), one_digit(100)]
    if n >= 256:
        lists.append(splitters(255))
    else:
        lists.append(splitters(min(n, 7)))
    return lists


SIZES = [1, 2, ll.TILE - 1, ll.TILE, ll.TILE + 1, ll.SHARE - 1, ll.SHARE, ll.SHARE + 1, 3 * ll.SHARE + 5, 1001, 1002, 1003]


@pytest.mark.parametrize("dt", [ol.U32, ol.U64])
def test_sizes(dt, monkeypatch):
    rot = itertools.cycle(VARIANTS)
    for n in SIZES:
        both_routes(monkeypatch, ol.DTYPE_NAMES[dt], ol.splitmix_fill(n, dt, 8100 + dt), dt, small_lists(n), rot=rot)


@pytest.mark.parametrize("dt", [ol.U32, ol.U64])
def test_src_one_element_behind_a_boundary(dt, monkeypatch):
    for n in (ll.TILE + 2, 3 * ll.SHARE + 5):
        both_routes(monkeypatch, "offset", ol.splitmix_fill(n, dt, 8200 + dt), dt, small_lists(n), offset=1)


@pytest.mark.parametrize("dt", [ol.U32, ol.U64])
def test_the_cut_off(dt, monkeypatch):
    """4096 distinct values search, 4097 sort, 5000 values of which 4096 are distinct search; and all edges in one digit"""
    n = 3 * ll.SHARE + 5
    lists = [distinct(4096, 41), distinct(4097, 42), distinct(4096, 43, repeat_to=5000), one_digit(4095), one_digit(1000)]
    infos = both_routes(monkeypatch, "cut-off", ol.splitmix_fill(n, dt, 8300 + dt), dt, lists)
    for o in (ol.ASC, ol.DESC):
        assert [infos[(o, i)].route for i in range(5)] == [rsa.LOCATE_SEARCH, rsa.LOCATE_SORT, rsa.LOCATE_SEARCH, rsa.LOCATE_SEARCH, rsa.LOCATE_SEARCH]
        assert infos[(o, 0)].distinct_values == 4096 and infos[(o, 2)].distinct_values == 4096 and infos[(o, 1)].distinct_values > 4096
        assert infos[(o, 3)].search_steps == 12 and infos[(o, 4)].search_steps == 10     # (ll.check compared them with the header's rule)


def test_a_lowered_cut_off(monkeypatch):
    """RSX_LOCATE_MAX_VALUES=k: k distinct values search, k + 1 sort"""
    dt, n = ol.U32, ll.SHARE + 77
    bits = ol.splitmix_fill(n, dt, 8400)
    want = ll.Want(bits, dt)
    src_t = to_dev(bits)
    switch(monkeypatch, MAX_VALUES=33)
    assert run_case("k", src_t, want, distinct(33, 44)(want), route=rsa.LOCATE_SEARCH).distinct_values == 33
    assert run_case("k + 1", src_t, want, distinct(34, 45)(want), route=rsa.LOCATE_SORT).distinct_values == 34
    switch(monkeypatch, MAX_VALUES=1)
    run_case("1", src_t, want, bits[[5, 5, 5]], route=rsa.LOCATE_SEARCH)
    run_case("2", src_t, want, bits[[5, 6]], route=rsa.LOCATE_SORT)


@pytest.mark.parametrize("dt", [ol.U32, ol.F64])
def test_all_keys_equal_with_one_counter_set_and_the_default(dt, monkeypatch):
    n = 2 * ll.SHARE + 9
    bits = np.full(n, 0x40490FDB, dtype=ol.NP_BITS[dt])
    want = ll.Want(bits, dt)
    src_t = to_dev(bits)
    lists = [bits[[0]], in_k(0, -1)(want), np.concatenate([bits[[0]], absent(40, 51)(want)])]
    for sets in (1, None):
        switch(monkeypatch, COUNTER_SETS=sets)
        for i, vals in enumerate(lists):
            info = run_case("equal keys sets=%s list=%d" % (sets, i), src_t, want, vals, 4 + 4 * (i & 1), route=rsa.LOCATE_SEARCH)
            assert info.counter_sets == (1 if sets else 32)


@pytest.mark.parametrize("dt", [ol.U32, ol.U64])
def test_a_thirty_second_of_the_keys_one_value(dt, monkeypatch):
    n = 3 * ll.SHARE + 5
    bits = ol.splitmix_fill(n, dt, 8500 + dt)
    bits[::32] = bits[7]
    both_routes(monkeypatch, "thirty-second", bits, dt, [lambda w: w.bits[[7]], splitters(255), lambda w: np.concatenate([w.bits[[7, 7]], absent(30, 52)(w)])])


@pytest.mark.parametrize("dt", [ol.F32, ol.F64])
def test_floats_with_nans_and_zeros(dt, monkeypatch):
    n = ll.SHARE + 1003
    kb = ol.DTYPE_SIZE[dt]
    bits = ol.splitmix_fill(n, dt, 8600 + dt)
    sign, expo = 1 << (8 * kb - 1), (0x7F800000 if kb == 4 else 0x7FF0000000000000)
    special = np.array([0, sign, expo, expo | sign, expo | 1, expo | sign | 1, expo | (expo >> 1), expo | sign | (expo >> 1)], dtype=ol.NP_BITS[dt])
    bits[5:5 + 8 * 20] = np.tile(special, 20)
    both_routes(monkeypatch, "floats", bits, dt, [special, special[::-1][:3], splitters(255), lambda w: np.concatenate([special, absent(100, 53)(w)]),
                                                   in_k(0, -1)])


@pytest.mark.parametrize("dt", [ol.I32, ol.I64])
def test_signed_keys_across_zero(dt, monkeypatch):
    n = ll.SHARE + 1001
    t = ol.NP_BITS[dt]
    bits = (ol.splitmix_fill(n, dt, 8700 + dt).astype(np.int64) % 2001 - 1000).astype(np.int64).astype({4: np.int32, 8: np.int64}[ol.DTYPE_SIZE[dt]]).view(t)
    around = np.array([-3, -2, -1, 0, 1, 2, 3, -1000, 1000, -1001, 1001], dtype={4: np.int32, 8: np.int64}[ol.DTYPE_SIZE[dt]]).view(t)
    both_routes(monkeypatch, "signed", bits, dt, [around, around[3:4], splitters(63), in_k(0, -1)])


@pytest.mark.parametrize("dt", [ol.U8, ol.I8, ol.U16, ol.I16])
def test_table_route(dt, monkeypatch):
    """1- and 2-byte keys: m = 1, 300, 70000 (more values than table entries; 4-byte indices among them), every value equal"""
    rot = itertools.cycle(VARIANTS)
    for n in (1, 2, 4097, 3 * ll.SHARE + 5):
        bits = ol.splitmix_fill(n, dt, 8800 + dt)
        lists = [ol.splitmix_fill(1, dt, 61), ol.splitmix_fill(300, dt, 62), np.full(300, bits[0], dtype=bits.dtype), in_k(0, -1)]
        if n > 4000:
            lists.append(ol.splitmix_fill(70000, dt, 63))
        infos = both_routes(monkeypatch, ol.DTYPE_NAMES[dt], bits, dt, lists, rot=rot)
        assert all(i.route == rsa.LOCATE_TABLE for i in infos.values())
    # more values than table entries, 4-byte indices, every output
    switch(monkeypatch)
    bits = ol.splitmix_fill(70001, dt, 8900 + dt)
    vals = ol.splitmix_fill(70000, dt, 64)
    run_case("m >= 65536, idx 4", to_dev(bits), ll.Want(bits, dt), vals, 4, (True, True, True), False, rsa.LOCATE_TABLE)
    run_case("m >= 65536, idx 4, below", to_dev(bits), ll.Want(bits, dt, ol.DESC), vals, 4, (True, True, True), True, rsa.LOCATE_TABLE)


def test_four_mi_keys_and_the_splitters_of_nth():
    """No switch set: 4 Mi + 5 u32 keys, the 255 splitters radix_sort_nth finds, all three outputs: one read of the keys, and the
    sizes of the parts (the bins counted) are the differences of `less`."""
    dt, n = ol.U32, (4 << 20) + 5
    bits = ol.splitmix_fill(n, dt, 9001)
    src_t = to_dev(bits)
    keys_t, _, _, _, _ = rsa.radix_sort_nth(src_t, [(i + 1) * n // 256 for i in range(255)], dtype=rsa.U32, want_idx=False)
    torch.cuda.synchronize()
    vals = keys_t.cpu().numpy().view(np.uint32)
    want = ll.Want(bits, dt)
    less_t, equal_t, bin_t = (torch.full((c,), 0x5A, dtype=torch.int32, device="cuda") for c in (255, 255, n))
    rc, info = ll.call_device(src_t, n, keys_t, 255, dt, ol.ASC, 4, less_t, equal_t, bin_t, 0)
    assert rc == 0, rsa.lib().rsx_last_error()
    ll.check("4 Mi", want, vals, src_t, keys_t, less_t, equal_t, bin_t, False, info, rsa.LOCATE_SEARCH)
    assert info.input_reads == 1
    less = np.sort(less_t.cpu().numpy().view(np.uint32).astype(np.int64))
    parts = np.bincount(bin_t.cpu().numpy().view(np.uint32), minlength=256)
    assert np.array_equal(parts, np.diff(np.concatenate([[0], less, [n]])))
    assert abs(parts - n / 256).max() <= 1 + int(equal_t.cpu().numpy().max())     # the split is balanced, as nth promises


def test_u64_keys_below_two_to_the_forty():
    dt, n = ol.U64, (1 << 20) + 3
    bits = ol.splitmix_fill(n, dt, 9002, (1 << 40) - 1)
    want = ll.Want(bits, dt, ol.DESC)
    vals = np.concatenate([bits[:500], ol.splitmix_fill(500, dt, 9003, (1 << 40) - 1)])
    run_case("u64 < 2^40", to_dev(bits), want, vals, 8, (True, True, True), False, rsa.LOCATE_SEARCH)


def test_a_sequence_on_one_context():
    """sort -> locate -> rank sort -> locate with other sizes on one stream: the context's buffers are shared with the sorts"""
    dt = ol.U32
    a = ol.splitmix_fill(300001, dt, 9100)
    src = to_dev(a)
    res, _ = rsa.radix_sort(src.clone(), torch.zeros_like(src), dtype=rsa.U32)
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy().view(np.uint32), np.sort(a))
    want = ll.Want(a, dt)
    run_case("after a sort", src, want, splitters(255)(want), 4, (True, True, True), False, rsa.LOCATE_SEARCH)
    run_case("after a sort, many values", src, want, distinct(5000, 71)(want), 8, (True, True, True), True, rsa.LOCATE_SORT)
    b = ol.splitmix_fill(100003, ol.F32, 9101)
    ib = torch.zeros(2 * b.size, dtype=torch.int32, device="cuda")
    ranks, _ = rsa.radix_sort_rank(to_dev(b), ib, dtype=rsa.F32)
    torch.cuda.synchronize()
    assert np.array_equal(ranks.cpu().numpy().view(np.uint32), ol.oracle_rank(b, ol.F32, 4)[0])
    c = ol.splitmix_fill(ll.SHARE + 3, ol.U64, 9102)
    wc = ll.Want(c, ol.U64, ol.DESC)
    run_case("after a rank sort", to_dev(c), wc, splitters(63)(wc), 8, (True, False, True), False, rsa.LOCATE_SEARCH)
    run_case("and the first keys again", src, want, splitters(7)(want), 4, (False, True, True), True, rsa.LOCATE_SEARCH)
    res, _ = rsa.radix_sort(src.clone(), torch.zeros_like(src), dtype=rsa.U32)
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy().view(np.uint32), np.sort(a))


def test_the_python_conveniences():
    a = ol.splitmix_fill(50001, ol.I32, 9200)
    src = to_dev(a)
    v = np.concatenate([a[:40], ol.splitmix_fill(60, ol.I32, 9201)])
    vt = to_dev(v)
    s = np.sort(a.view(np.int32))
    for side in ("left", "right"):
        got, info = rsa.searchsorted(src, vt, side=side)
        assert np.array_equal(got.cpu().numpy(), np.searchsorted(s, v.view(np.int32), side=side))
    edges = np.sort(v.view(np.int32))
    for right in (False, True):
        got, info = rsa.bucketize(src, vt, right=right)
        assert np.array_equal(got.cpu().numpy(), np.searchsorted(edges, a.view(np.int32), side="right" if right else "left"))
        assert np.array_equal(got.cpu(), torch.bucketize(torch.from_numpy(a.view(np.int32).copy()), torch.from_numpy(edges.copy()), right=right))
    info, le, eq, bi = rsa.radix_sort_locate_host(a, v, rsa.I32, equal=True, bins=True, below=True)
    want = ll.Want(a, ol.I32)
    ll.check("host", want, v, None, None, le, eq, bi, True, info, rsa.LOCATE_SEARCH)
    info, le, eq, bi = rsa.radix_sort_locate_host(a, v[:0], rsa.I32, less=False, bins=True)
    assert info.route == rsa.LOCATE_TRIVIAL and not bi.any() and bi.size == a.size
    info, le, eq, bi = rsa.radix_sort_locate_host(a[:0], v, rsa.I32, equal=True)
    assert info.route == rsa.LOCATE_TRIVIAL and not le.any() and not eq.any() and le.size == v.size


def test_a_capturing_stream_is_refused():
    bits = ol.splitmix_fill(4095, ol.U32, 9300)
    want = ll.Want(bits, ol.U32)
    vals = ol.splitmix_fill(10, ol.U32, 9301)
    a, v = to_dev(bits), to_dev(vals)
    less_t = torch.zeros(10, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc, info = ll.call_device(a, 4095, v, 10, ol.U32, ol.ASC, 4, less_t, None, None, 0, s)     # (the context of this stream exists before the capture)
        assert rc == 0, rsa.lib().rsx_last_error()
    s.synchronize()
    ll.check("before the capture", want, vals, a, v, less_t, None, None, False, info, rsa.LOCATE_SEARCH)
    less_t.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, _ = ll.call_device(a, 4095, v, 10, ol.U32, ol.ASC, 4, less_t, None, None, 0, torch.cuda.current_stream())
        err = rsa.lib().rsx_last_error()
    assert rc == -1 and b"capturing" in err
    torch.cuda.synchronize()
    assert not less_t.any()
    rsa.lib().rsx_release_stream(s.cuda_stream)
