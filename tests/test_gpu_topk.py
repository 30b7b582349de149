"""rsx_sort_topk_device on the GPU: the first k of the stable sorted order, against the oracle's ranks.

Every case runs the select route (RSX_TOPK_FORCE=1) and the sort route (RSX_TOPK_FORCE=2), asserts the route, compares keys,
indices and the info fields with the oracle (topk_lib.Want) and checks that the source is unchanged.  The oracle's ranks are
computed once per (keys, dtype, order) and shared by every k.  The sweep crosses n x k x dtype x order completely; the index
width (4 / 8 bytes) and which outputs are asked for (both / keys only / indices only) rotate over the cases instead of
multiplying them -- every (width, outputs) pair meets every n and every dtype many times -- which keeps the file at a few
seconds."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa
import topk_lib as tl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_IT = {4: torch.int32, 8: torch.int64}
ROUTES = (("1", rsa.TOPK_SELECT), ("2", rsa.TOPK_SORT))
VARIANTS = list(itertools.product((4, 8), ("both", "keys", "idx")))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    monkeypatch.delenv("RSX_TOPK_FORCE", raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_TOPK_FORCE", raising=False)
    rsa.reload_env()


def force(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("RSX_TOPK_FORCE", raising=False)
    else:
        monkeypatch.setenv("RSX_TOPK_FORCE", value)
    rsa.reload_env()


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).cuda()


def run_case(tag, src_t, want, k, idx_bytes=4, outputs="both", route=None, stream=None):
    """One call; returns (info, keys bytes, indices) for comparisons between routes."""
    kb = ol.DTYPE_SIZE[want.dt]
    n = want.bits.size
    keys_t = torch.full((k,), 0x5A, dtype=_T[kb], device="cuda") if outputs in ("both", "keys") else None
    idx_t = torch.full((k,), 0x5A, dtype=_IT[idx_bytes], device="cuda") if outputs in ("both", "idx") else None
    rc, info = tl.call_device(src_t, n, k, want.dt, want.order, idx_bytes, keys_t, idx_t, stream)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    if stream is not None:
        stream.synchronize()
    tl.check(tag, want, k, keys_t, idx_t, info, route)
    return info


def both_routes(monkeypatch, tag, bits, dt, ks, orders=(ol.ASC, ol.DESC), variants=None):
    """Every k in both orders on both routes; returns {(order, k): the select route's info}."""
    bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    src_t = to_dev(bits)
    wants = {o: tl.Want(bits, dt, o) for o in orders}
    rot = itertools.cycle(variants or VARIANTS)
    infos = {}
    cases = [(o, k, next(rot)) for o in orders for k in ks]
    for value, route in ROUTES:
        force(monkeypatch, value)
        for o, k, (ib, outs) in cases:
            info = run_case("%s n=%d k=%d order=%d ib=%d %s force=%s" % (tag, bits.size, k, o, ib, outs, value), src_t, wants[o], k, ib,
                            outs, route)
            if route == rsa.TOPK_SELECT:
                infos[(o, k)] = info
    # (both routes were compared with the same oracle values: their outputs are identical)
    assert np.array_equal(src_t.cpu().numpy().view(ol.NP_BITS[dt]), bits), (tag, "src was written")
    return infos


# ---- the sweep ----------------------------------------------------------------------------------------------------------

SIZES = [2, 3, 255, 256, 257, 4095, 65537, 300001, (1 << 20) + 3]
EVERYWHERE = (ol.U32, ol.F32, ol.I64, ol.F64)


def ks_for(n):
    return sorted({min(max(k, 1), n) for k in (1, 2, 255, 256, 257, n // 16, n // 2, n - 1, n)})


@pytest.mark.parametrize("dt", list(range(10)))
def test_sweep(dt, monkeypatch):
    sizes = SIZES if dt in EVERYWHERE else SIZES[:3] + SIZES[-2:]
    for n in sizes:
        bits = ol.splitmix_fill(n, dt, 4100 + dt)
        both_routes(monkeypatch, ol.DTYPE_NAMES[dt], bits, dt, ks_for(n))


def test_uniform_keys_take_two_reads(monkeypatch):
    n = (1 << 20) + 3
    for dt in (ol.U32, ol.F32, ol.U64):
        infos = both_routes(monkeypatch, "uniform", ol.splitmix_fill(n, dt, 4201), dt, (1, 4096, n // 16), orders=(ol.ASC,))
        for key, info in infos.items():
            assert info.input_reads <= 2, (dt, key, info.input_reads)


def test_defaults_are_correct(monkeypatch):
    """The switch unset: whatever route the thresholds pick, the result is the oracle's."""
    force(monkeypatch, None)
    for n, dt in ((257, ol.U32), (65537, ol.F32), (300001, ol.I64), ((1 << 20) + 3, ol.U32), ((1 << 20) + 3, ol.F64)):
        bits = ol.splitmix_fill(n, dt, 4301, 0xFFFFFFFFFFF000FF)
        src_t = to_dev(bits)
        want = tl.Want(bits, dt, ol.ASC)
        for k in (1, 64, n // 16, n // 2, n):
            run_case("defaults n=%d k=%d" % (n, k), src_t, want, k)
        assert np.array_equal(src_t.cpu().numpy().view(ol.NP_BITS[dt]), bits)


# ---- inputs built to break the select route -----------------------------------------------------------------------------

def test_ties_across_the_k_boundary(monkeypatch):
    n = 65537
    bits = ol.splitmix_fill(n, ol.U32, 4401, 0x3)
    counts = np.bincount(bits, minlength=4)
    for order in (ol.ASC, ol.DESC):
        cum = np.cumsum(counts if order == ol.ASC else counts[::-1])
        ks = [7, int(cum[0]) + 5, int(cum[1]) - 1, int(cum[2]) + int(cum[3] - cum[2]) // 2]
        infos = both_routes(monkeypatch, "four values", bits, ol.U32, ks, orders=(order,), variants=[(4, "both"), (8, "idx")])
        for (o, k), info in infos.items():
            assert info.n_less < k < info.n_less + info.n_equal, (o, k, info.n_less, info.n_equal)
    # the kept indices of the k-th key's ties are exactly the lowest ones (ascending order, k five elements into the 1s)
    k = int(counts[0]) + 5
    force(monkeypatch, "1")
    idx_t = torch.empty(k, dtype=torch.int32, device="cuda")
    rc, info = tl.call_device(to_dev(bits), n, k, ol.U32, ol.ASC, 4, None, idx_t)
    assert rc == 0
    got = idx_t.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[int(counts[0]):], np.flatnonzero(bits == 1)[:5])


def test_all_keys_equal(monkeypatch):
    for dt, n in ((ol.U32, 65537), (ol.F64, 4095), (ol.U8, 300001)):
        bits = np.full(n, 0x42, dtype=ol.NP_BITS[dt])
        infos = both_routes(monkeypatch, "all equal", bits, dt, (1, 2, n // 2, n), variants=[(4, "both"), (8, "both")])
        for info in infos.values():
            assert info.n_less == 0 and info.n_equal == n
    force(monkeypatch, "1")
    idx_t = torch.empty(1000, dtype=torch.int64, device="cuda")
    rc, _ = tl.call_device(to_dev(np.full(65537, 7, dtype=np.uint32)), 65537, 1000, ol.U32, ol.DESC, 8, None, idx_t)
    assert rc == 0 and np.array_equal(idx_t.cpu().numpy(), np.arange(1000))


@pytest.mark.parametrize("dt", [ol.U32, ol.I64, ol.U16])
def test_oversized_bucket_stays_in_the_input(dt, monkeypatch):
    """Keys whose top bytes are constant: the selected bucket (all n keys) exceeds the candidate capacity, so every digit is
    found by a histogram over the input, and nothing overflows."""
    kb = ol.DTYPE_SIZE[dt]
    n = 65537
    assert n > tl.capacity(n)
    bits = ol.splitmix_fill(n, dt, 4501, 0xFF) | ol.NP_BITS[dt](0x1200 if kb == 2 else 0x12345600)
    infos = both_routes(monkeypatch, "constant top bytes", bits, dt, (1, 300, n // 2, n - 1))
    for key, info in infos.items():
        assert 2 < info.input_reads <= kb + 1, (key, info.input_reads)


def test_sorted_keys(monkeypatch):
    n = 65537
    a = np.sort(ol.splitmix_fill(n, ol.U32, 4601))
    both_routes(monkeypatch, "ascending", a, ol.U32, (1, 257, n // 2, n))
    both_routes(monkeypatch, "descending", a[::-1].copy(), ol.U32, (1, 257, n // 2, n))


def test_one_light_one_heavy_top_digit(monkeypatch):
    n = 65537
    a = ol.splitmix_fill(n, ol.U32, 4701, 0x00FFFFFF) | np.uint32(0x7F000000)
    a[n // 3] = 0x01000005      # the only key of its top digit
    infos = both_routes(monkeypatch, "light + heavy", a, ol.U32, (1, 2, n - 1))
    assert infos[(ol.ASC, 1)].input_reads == 2 and infos[(ol.ASC, 2)].input_reads > 2


def test_float_specials(monkeypatch):
    f32 = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x3F800000, 0xBF800000], dtype=np.uint32)
    a = np.concatenate([f32, ol.splitmix_fill(300, ol.U32, 4801), f32, f32])
    both_routes(monkeypatch, "f32 specials", a, ol.F32, (1, 3, 15, 45, a.size // 2, a.size - 1, a.size))
    f64 = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0xFFF8000000ABCDEF, 0x0, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x1, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000],
                   dtype=np.uint64)
    b = np.concatenate([f64, ol.splitmix_fill(300, ol.U64, 4802), f64, f64])
    both_routes(monkeypatch, "f64 specials", b, ol.F64, (1, 3, 12, 36, b.size // 2, b.size - 1, b.size))


def test_signed_extremes(monkeypatch):
    small = ol.splitmix_fill(1000, ol.U32, 4901, 0x7).astype(np.int32) - 3
    a = np.concatenate([[np.iinfo(np.int32).min, np.iinfo(np.int32).max], small, [np.iinfo(np.int32).max, np.iinfo(np.int32).min]])
    both_routes(monkeypatch, "i32 extremes", a.astype(np.int32).view(np.uint32), ol.I32, (1, 2, 3, 500, a.size - 2, a.size))
    small = ol.splitmix_fill(1000, ol.U64, 4902, 0x7).astype(np.int64) - 3
    b = np.concatenate([[np.iinfo(np.int64).min, np.iinfo(np.int64).max], small, [np.iinfo(np.int64).max, np.iinfo(np.int64).min]])
    both_routes(monkeypatch, "i64 extremes", b.astype(np.int64).view(np.uint64), ol.I64, (1, 2, 3, 500, b.size - 2, b.size))


@pytest.mark.parametrize("dt", [ol.U8, ol.U32, ol.U64])
def test_tile_edges(dt, monkeypatch):
    t = tl.tile(ol.DTYPE_SIZE[dt])
    for n in (t - 1, t, t + 1):
        both_routes(monkeypatch, "tile edge", ol.splitmix_fill(n, dt, 5001, 0xFFFFFFFF000FF0FF), dt, (1, 257, n // 2, n),
                    orders=(ol.ASC,))


# ---- streams ------------------------------------------------------------------------------------------------------------

def test_non_default_stream_and_growth(monkeypatch):
    """A stream of its own, and two calls of different n back to back on it: the context's buffers grow between them."""
    s = torch.cuda.Stream()
    for value, route in ROUTES:
        force(monkeypatch, value)
        for n in (4095, 300001, 65537):
            bits = ol.splitmix_fill(n, ol.U32, 5101 + n)
            want = tl.Want(bits, ol.U32, ol.ASC)
            src_t = to_dev(bits)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                run_case("stream n=%d" % n, src_t, want, n // 16, 4, "both", route, stream=s)
                run_case("stream n=%d" % n, src_t, want, n // 2, 8, "both", route, stream=s)
    rsa.lib().rsx_release_stream(s.cuda_stream)


def test_capturing_stream_is_refused(monkeypatch):
    n, k = 4095, 16
    bits = ol.splitmix_fill(n, ol.U32, 5201)
    want = tl.Want(bits, ol.U32, ol.ASC)
    src_t = to_dev(bits)
    keys_t = torch.zeros(k, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run_case("before the capture", src_t, want, k, stream=s)     # (the context of this stream exists before the capture)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, _ = tl.call_device(src_t, n, k, ol.U32, ol.ASC, 4, keys_t, None, torch.cuda.current_stream())
        err = rsa.lib().rsx_last_error()
    assert rc == -1 and b"capturing" in err
    torch.cuda.synchronize()
    assert not keys_t.any()
    rsa.lib().rsx_release_stream(s.cuda_stream)


# ---- the upper layers ---------------------------------------------------------------------------------------------------

def test_python_wrappers(monkeypatch):
    n, k = 65537, 300
    bits = ol.splitmix_fill(n, ol.F32, 5301, 0xFFF000FF)
    for value, route in ROUTES:
        force(monkeypatch, value)
        for order in (ol.ASC, ol.DESC):
            want = tl.Want(bits, ol.F32, order)
            keys, idx, info = rsa.radix_sort_topk(to_dev(bits), k, dtype=rsa.F32, order=order)
            assert idx.dtype == torch.int32
            tl.check("torch wrapper", want, k, keys, idx, info, route)
            keys, idx, info = rsa.radix_sort_topk(to_dev(bits), k, dtype=rsa.F32, order=order, want_idx=False)
            assert idx is None
            tl.check("torch wrapper, keys only", want, k, keys, None, info, route)
            hk, hi, info = rsa.radix_sort_topk_host(bits, k, rsa.F32, order)
            wkeys, widx = want.first(k)[:2]
            assert info.route == route and np.array_equal(hk, wkeys) and np.array_equal(hi.astype(np.uint64), widx)
            hk, hi, info = rsa.radix_sort_topk_host(bits, k, rsa.F32, order, idx_dtype=np.uint64)
            assert np.array_equal(hk, wkeys) and hi.dtype == np.uint64 and np.array_equal(hi, widx)


def test_cpp_template():
    exe = os.path.join(ROOT, "tests", "cpp", "topk_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "topk_check: ok" in out.stdout, out.stdout + out.stderr
