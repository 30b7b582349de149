"""rsx_sort_nth_device on the GPU: the entries at given ranks of the stable sorted order, against the oracle's ranks.

Every case runs the select route (RSX_NTH_FORCE=1) and the sort route (RSX_NTH_FORCE=2), asserts the route, compares keys,
indices, n_less and n_equal with the oracle (nth_lib.Want) and checks that the source is unchanged.  What a forced select
reports (digit_passes, active_buckets, from_prefix, candidates, or that it had to give up) is compared with the course
nth_lib counts from the oracle's sorted keys.  The oracle's ranks are computed once per (keys, dtype, order) and shared by
every rank list.  The index width (4 / 8 bytes), which outputs are asked for (both / keys only / indices only) and which of
the two host arrays are passed rotate over the cases instead of multiplying them."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import nth_lib as nl
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_IT = {4: torch.int32, 8: torch.int64}
ROUTES = (("1", rsa.NTH_SELECT), ("2", rsa.NTH_SORT))
VARIANTS = list(itertools.product((4, 8), ("both", "keys", "idx")))
HOST_ARRAYS = [(True, True), (True, False), (False, True), (True, True), (False, False)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    monkeypatch.delenv("RSX_NTH_FORCE", raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_NTH_FORCE", raising=False)
    rsa.reload_env()


def force(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("RSX_NTH_FORCE", raising=False)
    else:
        monkeypatch.setenv("RSX_NTH_FORCE", value)
    rsa.reload_env()


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).cuda()


def run_case(tag, src_t, want, ranks, idx_bytes=4, outputs="both", route=None, stream=None, host_arrays=(True, True)):
    """One call, checked against the oracle; returns its info."""
    kb = ol.DTYPE_SIZE[want.dt]
    n, m = want.bits.size, len(ranks)
    keys_t = torch.full((m,), 0x5A, dtype=_T[kb], device="cuda") if outputs in ("both", "keys") else None
    idx_t = torch.full((m,), 0x5A, dtype=_IT[idx_bytes], device="cuda") if outputs in ("both", "idx") else None
    rc, info, n_less, n_equal = nl.call_device(src_t, n, ranks, want.dt, want.order, idx_bytes, keys_t, idx_t, stream, host_arrays)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    if stream is not None:
        stream.synchronize()
    nl.check(tag, want, ranks, keys_t, idx_t, n_less, n_equal, info, route, host_arrays)
    return info


def both_routes(monkeypatch, tag, bits, dt, rank_lists, orders=(ol.ASC, ol.DESC), variants=None, src_t=None):
    """Every rank list in both orders on both routes; returns {(order, list number): (the forced select's info, its course)}."""
    bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    if src_t is None:
        src_t = to_dev(bits)
    wants = {o: nl.Want(bits, dt, o) for o in orders}
    rot, hrot = itertools.cycle(variants or VARIANTS), itertools.cycle(HOST_ARRAYS)
    out = {}
    cases = [(o, i, ranks(wants[o]) if callable(ranks) else ranks, next(rot), next(hrot)) for o in orders for i, ranks in enumerate(rank_lists)]
    for value, route in ROUTES:
        force(monkeypatch, value)
        for o, i, ranks, (ib, outs), ha in cases:
            if not len(ranks):
                continue
            t = "%s n=%d list=%d m=%d order=%d ib=%d %s force=%s" % (tag, bits.size, i, len(ranks), o, ib, outs, value)
            if route == rsa.NTH_SORT:
                run_case(t, src_t, wants[o], ranks, ib, outs, route, host_arrays=ha)
            elif len(set(ranks)) > rsa.NTH_MAX_SELECT_RANKS:
                run_case(t, src_t, wants[o], ranks, ib, outs, rsa.NTH_SORT, host_arrays=ha)     # too many distinct ranks to select
            else:
                info = run_case(t, src_t, wants[o], ranks, ib, outs, None, host_arrays=ha)
                out[(o, i)] = (info, nl.check_course(t, wants[o], ranks, outs != "keys", info))
    assert np.array_equal(src_t.cpu().numpy().view(ol.NP_BITS[dt]), bits), (tag, "src was written")
    return out


# ---- rank lists ---------------------------------------------------------------------------------------------------------

def straddle(want):
    """Two neighbouring ranks whose keys differ in their top digit (the middle such place), or nothing."""
    kb = ol.DTYPE_SIZE[want.dt]
    top = (want.kd.astype(np.uint64) >> np.uint64(8 * (kb - 1)))
    edges = np.flatnonzero(top[1:] != top[:-1])
    if not edges.size:
        return []
    r = int(edges[edges.size // 2])
    return [r, r + 1]


def rank_lists(n):
    spaced = lambda k: [(i * n) // k for i in range(k)]
    lists = [[0], [n - 1], [0, n - 1], [n // 4, n // 2, (3 * n) // 4], spaced(64),
             [n - 1, n // 2, n // 2, 0, n - 1, n // 2],          # repeats, descending
             straddle]
    if n >= 65:
        lists.append(spaced(65))                                   # 65 distinct ranks: the sort route
    return lists


# ---- the sweep ----------------------------------------------------------------------------------------------------------

def sizes_for(kb):
    t = nl.tile(kb)
    return [2, 3, t - 1, t, t + 1, 2 * t + 17, 3 * (1 << 16) + 5, (1 << 20) + 3]


@pytest.mark.parametrize("dt", list(range(10)))
def test_sweep(dt, monkeypatch):
    for n in sizes_for(ol.DTYPE_SIZE[dt]):
        bits = ol.splitmix_fill(n, dt, 7100 + dt)
        both_routes(monkeypatch, ol.DTYPE_NAMES[dt], bits, dt, rank_lists(n))


def test_sixty_five_distinct_ranks_take_the_sort_route(monkeypatch):
    """No switch set, n large enough to select: 64 distinct ranks select, 65 sort."""
    force(monkeypatch, None)
    n = 1 << 18
    bits = ol.splitmix_fill(n, ol.U32, 7201)
    want = nl.Want(bits, ol.U32, ol.ASC)
    src_t = to_dev(bits)
    run_case("64 ranks", src_t, want, [(i * n) // 64 for i in range(64)], route=rsa.NTH_SELECT)
    run_case("65 ranks", src_t, want, [(i * n) // 65 for i in range(65)], route=rsa.NTH_SORT)
    run_case("64 distinct among 200", src_t, want, [((i % 64) * n) // 64 for i in range(200)], route=rsa.NTH_SELECT)


@pytest.mark.parametrize("n,route", [(1 << 18, rsa.NTH_SELECT), ((1 << 18) - 1, rsa.NTH_SORT)])
def test_default_route(n, route, monkeypatch):
    force(monkeypatch, None)
    for dt in (ol.U32, ol.F64):
        bits = ol.splitmix_fill(n, dt, 7301)
        want = nl.Want(bits, dt, ol.ASC)
        src_t = to_dev(bits)
        for ranks in ([n // 2], [n // 4, n // 2, (3 * n) // 4], [(i * n) // 64 for i in range(64)]):
            run_case("default n=%d" % n, src_t, want, ranks, route=route)
        assert np.array_equal(src_t.cpu().numpy().view(ol.NP_BITS[dt]), bits)


# ---- the distributions whose courses the design was worked out on -------------------------------------------------------

def _spaced(n, k):
    return [(i * n) // k for i in range(k)]


def _distributions():
    n = (1 << 20) + 3
    rng = np.random.default_rng(7401)
    five = [0, n // 4, n // 2, (3 * n) // 4, n - 1]
    quart = [n // 4, n // 2, (3 * n) // 4]
    u32 = ol.splitmix_fill(n, ol.U32, 7402)
    f01 = rng.random(n, dtype=np.float32).view(np.uint32)
    return [
        ("uniform u32, 5 ranks", u32, ol.U32, [five]),
        ("uniform u32, 64 ranks", u32, ol.U32, [_spaced(n, 64)]),
        ("u32 & 0xFFFF", u32 & np.uint32(0xFFFF), ol.U32, [five, _spaced(n, 9)]),
        ("f32 in [0, 1)", f01, ol.F32, [quart, [(i * n) // 64 for i in range(1, 64)]]),
        ("normal f32", rng.standard_normal(n, dtype=np.float32).view(np.uint32), ol.F32, [quart, _spaced(n, 9)]),
        ("normal f64", rng.standard_normal(n).view(np.uint64), ol.F64, [quart, _spaced(n, 9)]),
        ("u64 below 2^40", ol.splitmix_fill(n, ol.U64, 7403, (1 << 40) - 1), ol.U64, [five, _spaced(n, 64)]),
    ]


@pytest.mark.parametrize("case", range(7))
def test_distributions_take_the_counted_course(case, monkeypatch):
    tag, bits, dt, lists = _distributions()[case]
    got = both_routes(monkeypatch, tag, bits, dt, lists, orders=(ol.ASC,), variants=[(4, "both"), (8, "keys"), (8, "idx")])
    assert len(got) == len(lists)
    for info, course in got.values():
        assert not course.falls_to_sort and info.route == rsa.NTH_SELECT and info.from_prefix == 0
        assert info.input_reads == info.digit_passes + 2 <= ol.DTYPE_SIZE[dt] + 2


def test_capacity_boundary(monkeypatch):
    """Rank 0 with exactly cap elements of top digit 0 and every other top digit above: they fit after one histogram; with one
    element more they do not, and the second digit leaves a few hundred."""
    n = 1 << 18
    cap = nl.capacity(n)
    for extra, passes in ((0, 1), (1, 2)):
        a = ol.splitmix_fill(n, ol.U32, 7501 + extra)
        low = a & np.uint32(0x00FFFFFF)
        a = low | np.uint32(0x01000000) | (a & np.uint32(0x7E000000))       # top digits 1 .. 127
        a[::7][:cap + extra] = low[::7][:cap + extra]                        # ... and cap (+ 1) keys of top digit 0
        assert int((a >> np.uint32(24) == 0).sum()) == cap + extra
        got = both_routes(monkeypatch, "cap + %d" % extra, a, ol.U32, [[0], [0]], orders=(ol.ASC,), variants=[(4, "both"), (4, "keys")])
        for info, course in got.values():
            assert info.route == rsa.NTH_SELECT and info.digit_passes == passes and info.active_buckets == 1
            if extra == 0:
                assert info.candidates == cap
            else:
                assert 0 < info.candidates < 1000


# ---- inputs built to break the select route -----------------------------------------------------------------------------

def test_all_equal_and_eight_values(monkeypatch):
    """A wanted key that occurs more often than the candidate buffer holds: keys alone are answered from the digits, a call that
    wants indices takes the sort route and says so -- and still gives the oracle's indices."""
    n = 65537
    quart = [n // 4, n // 2, (3 * n) // 4]
    cases = [("all equal u32", np.full(n, 0x42, dtype=np.uint32), ol.U32), ("all equal f64", np.full(n, 0xC045000000000000, dtype=np.uint64), ol.F64),
             ("eight values", ol.splitmix_fill(n, ol.U32, 7601, 0x7), ol.U32), ("eight values i64", ol.splitmix_fill(n, ol.U64, 7602, 0x7), ol.I64)]
    for tag, bits, dt in cases:
        got = both_routes(monkeypatch, tag, bits, dt, [quart, quart, [0, n - 1], [n - 1, 0]], variants=[(4, "keys"), (8, "both")])
        for (o, i), (info, course) in got.items():
            if i in (0, 2):      # keys only
                assert info.route == rsa.NTH_SELECT and info.from_prefix == 1 and info.candidates == 0
                assert info.digit_passes == ol.DTYPE_SIZE[dt] == info.input_reads
            else:
                assert course.falls_to_sort and info.route == rsa.NTH_SORT


def test_sorted_and_reversed_keys(monkeypatch):
    n = 65537
    a = np.sort(ol.splitmix_fill(n, ol.U32, 7701))
    both_routes(monkeypatch, "ascending", a, ol.U32, rank_lists(n)[:6])
    both_routes(monkeypatch, "descending", a[::-1].copy(), ol.U32, rank_lists(n)[:6])


def test_float_specials(monkeypatch):
    f32 = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x3F800000, 0xBF800000], dtype=np.uint32)
    a = np.concatenate([f32, ol.splitmix_fill(300, ol.U32, 7801), f32, f32])
    every = list(range(a.size))
    both_routes(monkeypatch, "f32 specials", a, ol.F32, [every[:64], every[-64:], every[::-1], [0, a.size - 1], every[100:164:3]])
    f64 = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0xFFF8000000ABCDEF, 0x0, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x1, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000],
                   dtype=np.uint64)
    b = np.concatenate([f64, ol.splitmix_fill(300, ol.U64, 7802), f64, f64])
    every = list(range(b.size))
    both_routes(monkeypatch, "f64 specials", b, ol.F64, [every[:64], every[-64:], every[::-1], [0, b.size - 1]])


def test_signed_extremes(monkeypatch):
    small = ol.splitmix_fill(1000, ol.U32, 7901, 0x7).astype(np.int32) - 3
    a = np.concatenate([[np.iinfo(np.int32).min, np.iinfo(np.int32).max], small, [np.iinfo(np.int32).max, np.iinfo(np.int32).min]])
    n = a.size
    both_routes(monkeypatch, "i32 extremes", a.astype(np.int32).view(np.uint32), ol.I32, [[0, 1, 2, n - 3, n - 2, n - 1], [n // 2], [1, n - 2]])
    small = ol.splitmix_fill(1000, ol.U64, 7902, 0x7).astype(np.int64) - 3
    b = np.concatenate([[np.iinfo(np.int64).min, np.iinfo(np.int64).max], small, [np.iinfo(np.int64).max, np.iinfo(np.int64).min]])
    both_routes(monkeypatch, "i64 extremes", b.astype(np.int64).view(np.uint64), ol.I64, [[0, 1, 2, n - 3, n - 2, n - 1], [n // 2], [1, n - 2]])


def test_misaligned_source(monkeypatch):
    """d_src one element past a 16-byte boundary: the vector loads must not be taken."""
    for dt in (ol.U8, ol.U16, ol.U32, ol.F64):
        kb = ol.DTYPE_SIZE[dt]
        n = 2 * nl.tile(kb) + 17
        bits = ol.splitmix_fill(n, dt, 8001)
        whole = torch.zeros(n + 1, dtype=_T[kb], device="cuda")
        whole[1:].copy_(to_dev(bits))
        assert whole.data_ptr() % 16 == 0
        both_routes(monkeypatch, "misaligned", bits, dt, rank_lists(n)[:6], orders=(ol.ASC,), src_t=whole[1:])


# ---- streams ------------------------------------------------------------------------------------------------------------

def test_non_default_stream_and_growth(monkeypatch):
    """A stream of its own, and calls of different n back to back on it: the context's buffers grow between them."""
    s = torch.cuda.Stream()
    for value, route in ROUTES:
        force(monkeypatch, value)
        for n in (4095, 300001, 65537):
            bits = ol.splitmix_fill(n, ol.U32, 8101 + n)
            want = nl.Want(bits, ol.U32, ol.ASC)
            src_t = to_dev(bits)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                run_case("stream n=%d" % n, src_t, want, [n // 4, n // 2, (3 * n) // 4], 4, "both", route, stream=s)
                run_case("stream n=%d" % n, src_t, want, [(i * n) // 64 for i in range(64)], 8, "both", route, stream=s)
    rsa.lib().rsx_release_stream(s.cuda_stream)


def test_capturing_stream_is_refused(monkeypatch):
    n = 4095
    bits = ol.splitmix_fill(n, ol.U32, 8201)
    want = nl.Want(bits, ol.U32, ol.ASC)
    src_t = to_dev(bits)
    keys_t = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run_case("before the capture", src_t, want, [7, n // 2], stream=s)     # (the context of this stream exists before the capture)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, _, n_less, _ = nl.call_device(src_t, n, [7, n // 2], ol.U32, ol.ASC, 4, keys_t, None, torch.cuda.current_stream())
        err = rsa.lib().rsx_last_error()
    assert rc == -1 and b"capturing" in err
    torch.cuda.synchronize()
    assert not keys_t.any() and (n_less == 0xA5A5A5A5A5A5A5A5).all()
    rsa.lib().rsx_release_stream(s.cuda_stream)


# ---- the upper layers ---------------------------------------------------------------------------------------------------

def test_host_entry_point(monkeypatch):
    """rsx_sort_nth on host arrays, and on device pointers through the host entry."""
    n = 65537
    bits = ol.splitmix_fill(n, ol.F32, 8301, 0xFFF000FF)
    ranks = [n - 1, 5, n // 2, 5, n // 3]
    p64 = C.POINTER(C.c_uint64)
    for value, route in ROUTES:
        force(monkeypatch, value)
        for order in (ol.ASC, ol.DESC):
            want = nl.Want(bits, ol.F32, order)
            hk, hi, n_less, n_equal, info = rsa.radix_sort_nth_host(bits, ranks, rsa.F32, order)
            nl.check("host arrays", want, ranks, hk, hi, n_less, n_equal, info, route)
            hk, hi, n_less, n_equal, info = rsa.radix_sort_nth_host(bits, ranks, rsa.F32, order, idx_dtype=np.uint64)
            assert hi.dtype == np.uint64
            nl.check("host arrays, 8-byte indices", want, ranks, hk, hi, n_less, n_equal, info, route)
            hk, hi, n_less, n_equal, info = rsa.radix_sort_nth_host(bits, ranks, rsa.F32, order, want_idx=False)
            assert hi is None
            nl.check("host arrays, keys only", want, ranks, hk, None, n_less, n_equal, info, route)
            # device pointers through rsx_sort_nth
            src_t = to_dev(bits)
            keys_t = torch.full((len(ranks),), 0x5A, dtype=torch.int32, device="cuda")
            idx_t = torch.full((len(ranks),), 0x5A, dtype=torch.int64, device="cuda")
            r = np.array(ranks, dtype=np.uint64)
            n_less, n_equal, info = np.zeros(r.size, dtype=np.uint64), np.zeros(r.size, dtype=np.uint64), rsa.NthInfo()
            torch.cuda.synchronize()
            rc = rsa.lib().rsx_sort_nth(src_t.data_ptr(), n, r.ctypes.data_as(p64), r.size, rsa.F32, order, keys_t.data_ptr(), idx_t.data_ptr(),
                                        8, n_less.ctypes.data_as(p64), n_equal.ctypes.data_as(p64), C.byref(info))
            assert rc == 0, rsa.lib().rsx_last_error()
            nl.check("device pointers, host entry", want, ranks, keys_t, idx_t, n_less, n_equal, info, route)
    rc = rsa.lib().rsx_sort_nth(src_t.data_ptr(), n, r.ctypes.data_as(p64), r.size, rsa.F32, 0, hk.ctypes.data, None, 4, None, None, None)
    assert rc == -1 and b"host and device pointers in one call" in rsa.lib().rsx_last_error()


def test_one_key_on_the_device():
    src_t = to_dev(np.array([0xBF800000], dtype=np.uint32))
    keys_t = torch.full((3,), 0x5A, dtype=torch.int32, device="cuda")
    idx_t = torch.full((3,), 0x5A, dtype=torch.int64, device="cuda")
    rc, info, n_less, n_equal = nl.call_device(src_t, 1, [0, 0, 0], ol.F32, ol.DESC, 8, keys_t, idx_t)
    assert rc == 0 and info.route == rsa.NTH_TRIVIAL
    torch.cuda.synchronize()
    assert keys_t.cpu().numpy().view(np.uint32).tolist() == [0xBF800000] * 3 and idx_t.cpu().tolist() == [0, 0, 0]
    assert n_less.tolist() == [0, 0, 0] and n_equal.tolist() == [1, 1, 1]


def test_python_wrappers(monkeypatch):
    n = 65537
    bits = ol.splitmix_fill(n, ol.F32, 8401, 0xFFF000FF)
    ranks = [n // 2, 0, n - 1, n // 2]
    for value, route in ROUTES:
        force(monkeypatch, value)
        for order in (ol.ASC, ol.DESC):
            want = nl.Want(bits, ol.F32, order)
            keys, idx, n_less, n_equal, info = rsa.radix_sort_nth(to_dev(bits), ranks, dtype=rsa.F32, order=order)
            assert idx.dtype == torch.int32
            nl.check("torch wrapper", want, ranks, keys, idx, n_less, n_equal, info, route)
            keys, idx, n_less, n_equal, info = rsa.radix_sort_nth(to_dev(bits), np.array(ranks), dtype=rsa.F32, order=order, want_idx=False)
            assert idx is None
            nl.check("torch wrapper, keys only", want, ranks, keys, None, n_less, n_equal, info, route)
    with pytest.raises(rsa.RsxError, match="rank exceeds n"):
        rsa.radix_sort_nth(to_dev(bits), [n], dtype=rsa.F32)


def test_cpp_template():
    exe = os.path.join(ROOT, "tests", "cpp", "nth_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "nth_check: ok" in out.stdout, out.stdout + out.stderr
