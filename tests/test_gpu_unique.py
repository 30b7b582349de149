"""rsx_sort_unique_device on the GPU: the distinct keys in KDF order and their counts against the oracle, every route asserted
where a case was written for it (so that none passes by falling back), RSX_UNIQUE_MAX_BITS=0 against the bitmap results, edge
inputs, and full-size cases against torch.unique on the device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_CT = {4: torch.int32, 8: torch.int64}
ROUTE = {0: "TRIVIAL", 1: "BITMAP_LDS", 2: "BITMAP_GLOBAL", 3: "TABLE", 4: "SORT"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "bitmap_sort_16.json")) as f:
        return json.load(f)


def run(bits, dt, order=ol.ASC, count_bytes=0, stream=None):
    """radix_sort_unique on a device copy of `bits`: (keys, counts or None, info) back on the host as bit patterns."""
    kb = ol.DTYPE_SIZE[dt]
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    src = torch.from_numpy(a.view(ul.SIGNED[kb]).copy()).cuda()
    aux = torch.full_like(src, 0x5A)
    counts = torch.full((a.size,), -1, dtype=_CT[count_bytes], device="cuda") if count_bytes else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out, cnt, info = rsa.radix_sort_unique(src, aux, dtype=dt, order=order, counts=counts)
        stream.synchronize()
    else:
        out, cnt, info = rsa.radix_sort_unique(src, aux, dtype=dt, order=order, counts=counts)
    torch.cuda.synchronize()
    assert out.data_ptr() in (src.data_ptr(), aux.data_ptr())
    assert info.sort.result_in_aux == (out.data_ptr() == aux.data_ptr() and a.size > 0)
    keys = out.cpu().numpy().view(ol.NP_BITS[dt])
    cn = None if cnt is None else cnt.cpu().numpy().view(np.uint32 if count_bytes == 4 else np.uint64).astype(np.uint64)
    return keys, cn, info


def check(bits, dt, order=ol.ASC, count_bytes=0, route=None, what="", stream=None):
    want, wcnt = ul.want_unique(bits, dt, order)
    keys, cn, info = run(bits, dt, order, count_bytes, stream)
    tag = "%s dt=%d order=%d n=%d counts=%d route=%s" % (what, dt, order, np.asarray(bits).size, count_bytes, ROUTE.get(info.route))
    assert keys.size == want.size, tag + ": n_unique %d, oracle %d" % (keys.size, want.size)
    assert np.array_equal(keys, want), tag + ": keys differ from the oracle"
    if count_bytes:
        assert np.array_equal(cn, wcnt), tag + ": counts differ from the oracle"
        assert int(cn.sum()) == np.asarray(bits).size
    if route is not None:
        assert info.route == route, tag + ": expected route " + ROUTE[route]
    return keys, cn, info


# ---- Listing 7 --------------------------------------------------------------------------------------------------------

def test_listing7_c_abi_host_buffers():
    g = golden()
    src = np.array(g["input"], dtype=np.uint16)
    aux = np.full_like(src, 0xA5A5)
    counts = np.zeros(src.size, dtype=np.uint32)
    res, nu, info = C.c_void_p(), C.c_size_t(0), rsa.UniqueInfo()
    rsa.check(rsa.lib().rsx_sort_unique(src.ctypes.data, aux.ctypes.data, src.size, rsa.U16, rsa.ASCENDING, counts.ctypes.data, 4,
                                        C.byref(res), C.byref(nu), C.byref(info)))
    assert res.value in (src.ctypes.data, aux.ctypes.data)
    out = src if res.value == src.ctypes.data else aux
    assert list(out[:nu.value]) == g["output"]
    assert " ".join(str(int(v)) for v in out[:nu.value]) == g["printed"]
    assert list(counts[:nu.value]) == [1, 1, 1, 1, 3, 2, 1]


def test_listing7_python_wrapper():
    g = golden()
    a = np.array(g["input"], dtype=np.uint16)
    keys, cn, info = check(a, ol.U16, what="listing 7")
    assert list(keys) == g["output"] and info.route == rsa.UNIQUE_BITMAP_LDS and info.table_bytes == 8192
    keys, cn, info = check(a, ol.U16, count_bytes=8, what="listing 7 + counts")
    assert list(keys) == g["output"] and list(cn) == [1, 1, 1, 1, 3, 2, 1]
    keys, _, _ = check(a, ol.U16, order=ol.DESC, what="listing 7 descending")
    assert list(keys) == g["output"][::-1]


def test_listing7_cpp_template():
    exe = os.path.join(ROOT, "tests", "cpp", "unique_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "unique_check: ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.splitlines()[0].strip() == golden()["printed"]


# ---- the sweep ----------------------------------------------------------------------------------------------------------

SIZES = [2, 3, 255, 256, 257, 4095, 65537, 300001, (1 << 20) + 3]
MASKS = {1: 0xFF, 2: 0x3FFF, 4: 0x800FF0FF, 8: 0x80000000000FFFFF}


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt", list(range(10)))
def test_sweep(dt, order):
    kb = ol.DTYPE_SIZE[dt]
    for n in SIZES:
        a = ol.splitmix_fill(n, dt, 7100 + 13 * dt + n % 97, MASKS[kb])
        want, wcnt = ul.want_unique(a, dt, order)
        for cb in (0, 4, 8):
            keys, cn, info = run(a, dt, order, cb)
            tag = "dt=%d order=%d n=%d counts=%d route=%s" % (dt, order, n, cb, ROUTE.get(info.route))
            assert np.array_equal(keys, want), tag
            assert info.route in ROUTE and info.sort.key_bytes == kb, tag
            if cb:
                assert np.array_equal(cn, wcnt), tag
                assert info.route in (rsa.UNIQUE_TRIVIAL, rsa.UNIQUE_TABLE, rsa.UNIQUE_SORT), tag


# ---- routes by construction ---------------------------------------------------------------------------------------------

N22 = 1 << 22
BITMAP_CASES = [
    # (name, dtype, mask, route, varying bits, table bytes)
    ("u32-3runs-v16", ol.U32, 0x00F0FF0F, rsa.UNIQUE_BITMAP_LDS, 16, 8192),
    ("u64-v20", ol.U64, 0xFFFFF, rsa.UNIQUE_BITMAP_LDS, 20, 131072),
    ("f32-v19", ol.F32, 0x7FF000FF, rsa.UNIQUE_BITMAP_LDS, 19, 65536),
    ("u32-v22", ol.U32, 0x003FFFFF, rsa.UNIQUE_BITMAP_GLOBAL, 22, 1 << 19),
    ("u32-v24", ol.U32, 0x00FFFFFF, rsa.UNIQUE_BITMAP_GLOBAL, 24, 1 << 21),
]


@pytest.mark.parametrize("case", BITMAP_CASES, ids=[c[0] for c in BITMAP_CASES])
def test_bitmap_routes_and_forced_sort(case, monkeypatch):
    """The bitmap form the input was built for, then RSX_UNIQUE_MAX_BITS=0: the sort route, the identical keys."""
    name, dt, mask, route, vbits, tbytes = case
    a = ol.splitmix_fill(N22, dt, 8101, mask)
    keys, _, info = check(a, dt, route=route, what=name)
    assert info.varying_bits == vbits and info.table_bytes == tbytes, (info.varying_bits, info.table_bytes)
    keys_d, _, info_d = check(a, dt, order=ol.DESC, route=route, what=name + " desc")
    monkeypatch.setenv("RSX_UNIQUE_MAX_BITS", "0")
    keys0, _, info0 = check(a, dt, route=rsa.UNIQUE_SORT, what=name + " MAX_BITS=0")
    assert info0.table_bytes == 0
    assert np.array_equal(keys0, keys)
    # a cut-off below the input's varying bits: the sort route as well
    monkeypatch.setenv("RSX_UNIQUE_MAX_BITS", str(vbits - 1))
    keys1, _, _ = check(a, dt, route=rsa.UNIQUE_SORT, what=name + " MAX_BITS=V-1")
    assert np.array_equal(keys1, keys)


def test_table_routes(monkeypatch):
    a = ol.splitmix_fill(N22, ol.U32, 8102, 0x00FF0000)
    for cb in (0, 4, 8):
        _, _, info = check(a, ol.U32, count_bytes=cb, route=rsa.UNIQUE_TABLE, what="one column")
        assert info.table_bytes == 2048 and info.sort.kept_columns() == [2]
    b = ol.splitmix_fill(N22 + 5, ol.U8, 8103)
    for dt in (ol.U8, ol.I8):
        for order in (ol.ASC, ol.DESC):
            check(b, dt, order, 4, rsa.UNIQUE_TABLE, "1-byte keys")
            check(b, dt, order, 0, rsa.UNIQUE_TABLE, "1-byte keys")
    c = ol.splitmix_fill(N22 + 3, ol.I16, 8104)
    for order in (ol.ASC, ol.DESC):
        _, _, info = check(c, ol.I16, order, 4, rsa.UNIQUE_TABLE, "i16 + counts")
        assert info.table_bytes == 65536 * 4
        check(c, ol.I16, order, 8, rsa.UNIQUE_TABLE, "i16 + counts")
    small = ol.splitmix_fill(1000, ol.I16, 8105)
    check(small, ol.I16, ol.ASC, 4, rsa.UNIQUE_TABLE, "i16 + counts, small")
    monkeypatch.setenv("RSX_UNIQUE_MAX_BITS", "0")
    check(a, ol.U32, count_bytes=4, route=rsa.UNIQUE_SORT, what="one column, MAX_BITS=0")
    check(c, ol.I16, count_bytes=4, route=rsa.UNIQUE_SORT, what="i16, MAX_BITS=0")
    check(b, ol.U8, count_bytes=8, route=rsa.UNIQUE_SORT, what="u8, MAX_BITS=0")


def test_sort_routes():
    a = ol.splitmix_fill(N22, ol.F32, 8106, 0xFFF000FF)      # mixed signs: every KDF bit varies
    _, _, info = check(a, ol.F32, route=rsa.UNIQUE_SORT, what="f32 mixed signs")
    assert info.varying_bits == 32
    check(a, ol.F32, ol.DESC, 4, rsa.UNIQUE_SORT, "f32 mixed signs + counts")
    b = ol.splitmix_fill(N22, ol.U32, 8107, 0x00F0FF0F)      # bitmap-eligible, but counts are wanted
    check(b, ol.U32, count_bytes=8, route=rsa.UNIQUE_SORT, what="wide keys + counts")
    c = ol.splitmix_fill(N22, ol.U32, 8108, 0x55555555)      # sixteen runs: more than the key compaction holds
    keys, _, info = check(c, ol.U32, what="sixteen runs")
    assert info.route in ROUTE


def test_uniform_u32_inherits_the_fast_route():
    """Evenly spread keys at 2^24: the sample sends them to the sort before any histogram, and the sort takes its route 5."""
    a = ol.splitmix_fill(1 << 24, ol.U32, 8109)
    _, _, info = check(a, ol.U32, route=rsa.UNIQUE_SORT, what="uniform u32")
    assert info.sort.hybrid == 5 and info.varying_bits == 0
    _, _, info = check(a, ol.U32, count_bytes=4, route=rsa.UNIQUE_SORT, what="uniform u32 + counts")
    assert info.sort.hybrid == 5


# ---- edge inputs -------------------------------------------------------------------------------------------------------

def test_all_keys_equal():
    a = np.full(100003, 0xDEADBEEF, dtype=np.uint32)
    for cb in (0, 4, 8):
        keys, cn, info = check(a, ol.U32, count_bytes=cb, route=rsa.UNIQUE_TRIVIAL, what="all equal")
        assert keys.size == 1 and info.sort.result_in_aux == 0
        if cb:
            assert int(cn[0]) == a.size


def test_sorted_inputs():
    asc = np.arange(100003, dtype=np.uint32) * np.uint32(3)
    keys, _, info = check(asc, ol.U32, what="strictly ascending")
    assert keys.size == asc.size and info.sort.early_exit == 2
    keys, cn, info = check(asc, ol.U32, count_bytes=4, route=rsa.UNIQUE_SORT, what="strictly ascending + counts")
    assert keys.size == asc.size and info.sort.early_exit == 2 and np.all(cn == 1)
    dup = np.sort(ol.splitmix_fill(300001, ol.U32, 8110, 0x0003FFFF))
    check(dup, ol.U32, what="sorted with duplicates")
    check(dup, ol.U32, count_bytes=8, route=rsa.UNIQUE_SORT, what="sorted with duplicates + counts")
    f = np.sort(ol.splitmix_fill(300001, ol.U32, 8111, 0xFFFFFFFF))
    check(f, ol.U32, what="sorted, all bits")
    check(f[::-1].copy(), ol.U32, what="descending input")
    check(dup[::-1].copy(), ol.U32, count_bytes=4, what="descending input with duplicates")
    check(dup[::-1].copy(), ol.U32, order=ol.DESC, what="descending input, descending order")


def test_distinct_u64_keys():
    n = 1 << 20
    rng = np.random.default_rng(8112)
    a = (rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    assert np.unique(a).size == n
    keys, _, info = check(a, ol.U64, what="2^20 distinct u64")
    assert keys.size == n
    keys, cn, _ = check(a, ol.U64, count_bytes=4, route=rsa.UNIQUE_SORT, what="2^20 distinct u64 + counts")
    assert np.all(cn == 1)


@pytest.mark.parametrize("mask,route", [(0x00F0FF0F, rsa.UNIQUE_BITMAP_LDS), (0x0C3FFFF0, rsa.UNIQUE_BITMAP_LDS),
                                        (0x003FFFFF, rsa.UNIQUE_BITMAP_GLOBAL), (0x30FFFFF0, rsa.UNIQUE_BITMAP_GLOBAL)])
def test_bitmap_word_boundaries(mask, route):
    """Packed value 0, 2^V - 1 and both sides of every 64-bit word boundary of the bitmap -- and nothing else."""
    v = bin(mask).count("1")
    edges = np.arange(64, 1 << v, 64, dtype=np.uint64)
    packed = np.unique(np.r_[np.uint64(0), np.uint64((1 << v) - 1), edges - np.uint64(1), edges])
    keys = ul.deposit(packed, mask).astype(np.uint32)
    rng = np.random.default_rng(8113)
    a = np.repeat(keys, 3)
    rng.shuffle(a)
    got, _, info = check(a, ol.U32, route=route, what="word boundaries of mask %#x" % mask)
    assert info.varying_bits == v and got.size == packed.size
    got_d, _, _ = check(a, ol.I32, order=ol.DESC, route=route, what="word boundaries, i32 descending")
    assert got_d.size == packed.size


def test_non_default_stream():
    s = torch.cuda.Stream()
    a = ol.splitmix_fill(N22, ol.U32, 8114, 0x00F0FF0F)
    check(a, ol.U32, route=rsa.UNIQUE_BITMAP_LDS, what="side stream", stream=s)
    check(a, ol.U32, count_bytes=4, route=rsa.UNIQUE_SORT, what="side stream + counts", stream=s)
    b = ol.splitmix_fill(N22, ol.U32, 8115, 0x00FFFFFF)
    check(b, ol.U32, route=rsa.UNIQUE_BITMAP_GLOBAL, what="side stream, global bitmap", stream=s)
    rsa.release_stream(s)


def test_count_width_rule():
    src = torch.zeros(16, dtype=torch.int32, device="cuda")
    aux = torch.zeros_like(src)
    bad = torch.zeros(16, dtype=torch.int16, device="cuda")
    with pytest.raises(rsa.RsxError, match="count_bytes"):
        rsa.radix_sort_unique(src, aux, dtype=rsa.U32, counts=bad)


# ---- full size ----------------------------------------------------------------------------------------------------------

N28 = 1 << 28


@pytest.mark.parametrize("name,mask,route,cb", [("v20", 0x000FFFFF, rsa.UNIQUE_BITMAP_LDS, 0),
                                                ("v24", 0x00FFFFFF, rsa.UNIQUE_BITMAP_GLOBAL, 0),
                                                ("uniform", 0xFFFFFFFF, rsa.UNIQUE_SORT, 4)])
def test_full_size(name, mask, route, cb):
    """2^28 u32 keys, generated and checked on the device: torch.unique of the same keys (as int64, so that they order as
    unsigned), strict ascent, sum(counts) == n."""
    src = torch.empty(N28, dtype=torch.int32, device="cuda")
    rsa.fill_splitmix(src, 8200, mask)
    wide = src.to(torch.int64) & 0xFFFFFFFF
    want, wcnt = torch.unique(wide, sorted=True, return_counts=True)
    del wide
    aux = torch.empty_like(src)
    counts = torch.empty(N28, dtype=torch.int32, device="cuda") if cb else None
    out, cnt, info = rsa.radix_sort_unique(src, aux, dtype=rsa.U32, counts=counts)
    torch.cuda.synchronize()
    assert info.route == route, ROUTE.get(info.route)
    if name == "uniform":
        assert info.sort.hybrid == 5
    got = out.to(torch.int64) & 0xFFFFFFFF
    assert got.numel() == want.numel()
    assert bool(torch.all(got[1:] > got[:-1]))
    assert torch.equal(got, want)
    if cb:
        c64 = cnt.to(torch.int64) & 0xFFFFFFFF
        assert int(c64.sum()) == N28
        assert torch.equal(c64, wcnt)
