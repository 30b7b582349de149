"""Key + payload sorts with payloads that are NOT the input position, on every route such a sort can take.

Every other key + payload test gives arange(n) * a + b as payloads: ascending with the position, high bits zero.  A pass or a
leaf that broke ties by payload VALUE (a (key, payload) compound where the (key, position) one belongs), a carrier that lost a
payload's top bits, or a route that wrote the element's index for its payload would return the same bytes.  Here the payloads
come from tests/pairs_lib.py -- `random` (every bit used), `reversed` (the order inside every run of equal keys flips under a
tie-break by value), `edges` (top bit and sign of the carrier), `keybound` (wrong per element beside another key) -- on keys that
tie everywhere (every key twice; runs of four), and the expectation never comes from the library: the stable order of the derived
keys on the host (radix_sort_basic_kdf.hpp:19-46), gathered.  Bit for bit; result_in_aux, kept columns and early exit as the
oracle's; the route asserted wherever a test names one.  tests/test_pairs_lib_cpu.py shows which wrong sort each family exposes.

Sections: A the one-workgroup LDS kernel, B one pass per column, C one MSB pass + the pairs' leaves, D two levels that start
from the histogram, E without a histogram (every leaf shape), F an attempt called off after the spare buffers were written,
G the device-scheduled calls (plain, in a caller's workspace, in a captured graph), H under the library's own checker.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import pairs_lib as pl
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI = 1 << 20
_CARRIER = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
ORDERS = (ol.ASC, ol.DESC)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()     # (no back-off from an earlier attempt that was called off: the routes are asserted)
    yield
    torch.cuda.empty_cache()


def _dev(bits):
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(_CARRIER[a.itemsize]).copy()).cuda()


def _junk(t):
    return torch.full_like(t, 0x5A5A5A5A5A5A5A5A >> (64 - 8 * t.element_size()))


@functools.lru_cache(maxsize=4)
def _order(make, n, dt, seed, mask, order):
    """The keys of one case and what the reference decides about them: computed once, shared by the families that ride on them."""
    a = make(n, dt, seed, mask)
    return pl.Order(a, dt, order)


def _sort(want, family, width, seed, what, want_route=None, not_route=None):
    """One blocking key + payload sort of want.a with payloads of `family`, through the one comparison."""
    a = want.a
    vals = pl.payloads(family, a.size, width, seed, keys=a)
    keys, v = _dev(a), _dev(vals)
    kr, vr, info = rsa.radix_sort_pairs(keys, _junk(keys), v, _junk(v), dtype=want.dt, order=want.order)
    torch.cuda.synchronize()
    pl.compare(want, vals, kr, vr, info=info, want_route=want_route, not_route=not_route, what=(what, family, width, want.order))
    return info


# ---- A. the one-workgroup LDS kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("dt", [ol.U8, ol.I16, ol.U32, ol.F32, ol.U64, ol.F64], ids=lambda d: ol.DTYPE_NAMES[d])
def test_small_pairs_kernel_at_its_boundaries(dt, width):
    """Pairs that fit LDS twice (2 n (key + payload bytes) <= 128 KiB, csrc/rsx_small.hpp) at the sizes of
    test_small_pairs_and_rank_boundaries -- cap + 1 is the first size of the general kernels --, keys in runs of four."""
    cap = 131072 // (2 * (ol.DTYPE_SIZE[dt] + width))
    for n in sorted({2, 3, 64, 65, 1025, cap // 2 + 1, cap - 1, cap, cap + 1}):
        for order in ORDERS:
            want = _order(pl.runs_of_four, n, dt, 6100 + dt, None, order)
            if n >= 64 and ol.DTYPE_SIZE[dt] >= 4:
                pl.assert_ties(want.a)
            for family in ("random", "reversed"):
                _sort(want, family, width, 6100 + n, ("small", n))


# ---- B. one pass per column (route 0) ---------------------------------------------------------------------------------------
def _records_mask(dt):
    return 0xFFF000FF if dt in (ol.U32, ol.F32) else None     # (as test_pairs_vs_oracle_records masks its keys)


def _route0_cases(dt, width):
    for n, families in ((70001, ("random", "reversed")), (300007, ("edges", "keybound", "reversed"))):
        for order in ORDERS:
            want = _order(pl.runs_of_four, n, dt, 6200 + dt, _records_mask(dt), order)
            pl.assert_ties(want.a)
            for family in families:
                _sort(want, family, width, 6200 + n, ("route 0", n), want_route=0)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("dt", range(10), ids=ol.DTYPE_NAMES)
def test_one_pass_per_column(dt, width, monkeypatch):
    """All ten key types, both payload widths, both orders: rsx_scatter2_kernel<KT, VT> column by column (RSX_NO_HYBRID=1 keeps
    the 4-byte keys with 4-byte payloads off the leaves)."""
    monkeypatch.setenv("RSX_NO_HYBRID", "1")
    _route0_cases(dt, width)


def test_one_pass_per_column_on_the_table_ranking_kernel():
    """The same for u32 keys through rsx_scatter_kernel (RSX_FORCE_TABLE_RANK=1).  The library chooses its ranking kernel once per
    device and process, so those two cases run again in one child process (as tests/test_gpu_fallback.py does)."""
    env = dict(os.environ, RSX_FORCE_TABLE_RANK="1")
    ids = ["%s::test_one_pass_per_column[uint32_t-%d]" % (os.path.abspath(__file__), width) for width in (4, 8)]
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + ids,
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "2 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("family", ["random", "edges"])
def test_one_pass_per_column_with_8_byte_payloads_over_many_tiles(family):
    """u32 keys with 8-byte payloads at 4 Mi + 5: beyond every leaf's reach, 8-byte payloads never leave route 0."""
    want = _order(pl.every_key_twice, 4 * MI + 5, ol.U32, 6250, None, ol.ASC)
    _sort(want, family, 8, 6250, "4 Mi + 5, 8-byte payloads", want_route=0)


# ---- C. one MSB pass + the pairs' leaves (route 1) ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100000, 1000000])
@pytest.mark.parametrize("dt", [ol.U32, ol.I32, ol.F32], ids=["u32", "i32", "f32"])
def test_one_msb_pass_and_the_pairs_leaves(dt, n):
    """Mid-size arrays of 4-byte keys with 4-byte payloads: one (key, payload) pass by the top column, then rsx_leaf_pairs_kernel,
    which carries the pair as one 8-byte value through its LDS passes."""
    for order in ORDERS:
        want = _order(pl.every_key_twice, n, dt, 6300 + dt, None, order)
        pl.assert_ties(want.a)
        for family in ("random", "reversed"):
            _sort(want, family, 4, 6300 + dt, ("route 1", n), want_route=1 if dt != ol.F32 else None)


# ---- D. two levels that start from the histogram ----------------------------------------------------------------------------
def _two_levels(monkeypatch, no_slack):
    """Every sort compared with the oracle; returns the routes they took."""
    monkeypatch.setenv("RSX_TWO_LEVEL_MIN_LOG2", "22")
    monkeypatch.setenv("RSX_NO_BLIND", "1")
    if no_slack:
        monkeypatch.setenv("RSX_NO_SLACK", "1")
    routes = []
    for order in ORDERS:
        want = _order(pl.every_key_twice, (1 << 23) + 321, ol.U32, 6400, None, order)
        pl.assert_ties(want.a)
        for family in ("reversed", "random"):
            routes.append(int(_sort(want, family, 4, 6400, "two levels").hybrid))
    return routes


def test_two_levels_into_slack_slots(monkeypatch):
    """2^23 + 321 pairs with the threshold lowered: a (key, payload) pass by the top column, a second into slack slots without a
    count, rsx_leaf_pairs_kernel on the slots (info.hybrid == 4)."""
    assert _two_levels(monkeypatch, False) == [4, 4, 4, 4]


def test_two_levels_with_a_counted_second_pass(monkeypatch):
    """The same with RSX_NO_SLACK=1: the level-2 column counted per bucket, the second (key, payload) pass written densely into
    the first buffers, rsx_leaf_pairs_kernel on the dense buckets, in place (info.hybrid == 2)."""
    assert _two_levels(monkeypatch, True) == [2, 2, 2, 2]


@pytest.mark.parametrize("dt,order", [(ol.F32, ol.ASC), (ol.I32, ol.DESC)], ids=["f32", "i32 desc"])
def test_counted_second_pass_for_the_other_key_types(dt, order, monkeypatch):
    """... for keys whose derived form is not their bit pattern, and at a size that is no multiple of anything."""
    monkeypatch.setenv("RSX_TWO_LEVEL_MIN_LOG2", "22")
    monkeypatch.setenv("RSX_NO_BLIND", "1")
    monkeypatch.setenv("RSX_NO_SLACK", "1")
    want = _order(pl.every_key_twice, (1 << 22) + 12345, dt, 6450 + dt, None, order)
    pl.assert_ties(want.a)
    for family in ("reversed", "random", "keybound"):
        _sort(want, family, 4, 6450, "counted second pass", want_route=2)


def test_counted_second_pass_called_off_by_a_bucket_beyond_the_leaf(monkeypatch):
    """One (digit, digit) bucket with 6000 pairs more than its share does not fit the pairs' leaf (5120): known from the counts,
    before the second pass has written the first buffers -- the sort goes by one pass per column from them."""
    monkeypatch.setenv("RSX_TWO_LEVEL_MIN_LOG2", "22")
    monkeypatch.setenv("RSX_NO_BLIND", "1")
    monkeypatch.setenv("RSX_NO_SLACK", "1")
    n = (1 << 23) + 99
    a = pl.every_key_twice(n, ol.U32, 6460)
    a[1000:1000 + 6000 * 7:7] = (a[1000:1000 + 6000 * 7:7] & np.uint32(0x0000FFFF)) | np.uint32(0x12340000)
    want = pl.Order(pl.assert_ties(a), ol.U32)
    for family in ("reversed", "random"):
        _sort(want, family, 4, 6460, "bucket beyond the leaf", want_route=0)


# ---- E. without a histogram (route 5) -------------------------------------------------------------------------------------
BLIND_CASES = {
    # name: (n, switch, key mask, orders)
    "a wave per leaf, 256-pair slots": (5 * MI + 99, None, None, ORDERS),
    "a wave per leaf, 512-pair slots": (16 * MI + 99, None, None, ORDERS),
    "1280-pair leaves": (32 * MI + 99, None, None, (ol.ASC,)),
    "10240-pair leaves": (12 * MI + 1234, "RSX_PAIRS_LEAF_BIG", None, (ol.ASC,)),
    "level-1 slots all in scratch": (8 * MI + 5, "RSX_NO_AUX_SLOTS", None, (ol.ASC,)),
    "every leaf through the list": (10 * MI + 6, "RSX_LEAF16_MAXBIN", None, (ol.ASC,)),
    "fat bins": (10 * MI + 6, None, 0xFFFFFF0F, (ol.ASC,)),
}


@pytest.mark.parametrize("dt", [ol.F32, ol.U32], ids=["f32", "u32"])
@pytest.mark.parametrize("case", list(BLIND_CASES))
def test_without_histogram(case, dt, monkeypatch):
    """4-byte keys with 4-byte payloads from 4 Mi pairs on, nothing lowered: the level-1 pass reads the caller's payloads (the rank
    sort's pass makes the index there), rsx_leafp_kernel sorts (key half, position in the slot) compounds and gathers the payloads,
    rsx_leaf_pairs_kernel takes the leaves with fat bins -- in every shape the slots' capacity selects, with the level-1 slots in
    the spare buffers and in scratch, every leaf through the list launch (RSX_LEAF16_MAXBIN=0), and on keys whose low byte takes
    16 values.  Every key twice throughout."""
    n, switch, mask, orders = BLIND_CASES[case]
    if switch:
        monkeypatch.setenv(switch, "0" if switch == "RSX_LEAF16_MAXBIN" else "1")
    for order in orders:
        want = _order(pl.every_key_twice, n, dt, 6500 + dt, mask, order)
        pl.assert_ties(want.a)
        for family in ("reversed", "random"):
            _sort(want, family, 4, 6500 + dt, (case, n), want_route=5)


def _device_case(n, dt, seed, family):
    """Every key twice and one payload family, made on the device (the host's generator, counter-based: rsx_fill_splitmix_device)."""
    half = torch.empty(n - n // 2, dtype=torch.int32, device="cuda")
    rsa.fill_splitmix(half, seed)
    keys = torch.cat([half[: n // 2], half])
    del half
    if family == "random":
        vals = torch.empty(n, dtype=torch.int32, device="cuda")
        rsa.fill_splitmix(vals, pl.payload_seed(seed))
    else:
        vals = (n - 1 - torch.arange(n, dtype=torch.int64, device="cuda")).to(torch.int32)
    return keys, vals


def _device_checked_sort(n, dt, seed, family):
    keys, vals = _device_case(n, dt, seed, family)
    wk, wv, share = pl.device_expectation(keys, vals, dt)
    assert share >= 0.5, share
    ka, va = _junk(keys), _junk(vals)
    kr, vr, info = rsa.radix_sort_pairs(keys, ka, vals, va, dtype=dt)
    torch.cuda.synchronize()
    assert info.hybrid == 5 and info.result_in_aux == 0 and info.kept_columns() == [0, 1, 2, 3], (n, family, info.hybrid)
    assert torch.equal(kr, wk), (n, family, "keys")
    assert torch.equal(vr, wv), (n, family, "payloads")
    return wk, wv


def test_device_side_expectation_is_the_hosts():
    """The expectation of the two largest cases below -- derived keys as int64, a stable torch.sort, two gathers -- pinned to the
    host's at 5 Mi + 99, inputs included; and the sort itself checked against it once at that size."""
    n, dt = 5 * MI + 99, ol.F32
    a = pl.every_key_twice(n, dt, 6600)
    for order in ORDERS:
        want = pl.Order(a, dt, order)
        for family in ("random", "reversed"):
            keys, vals = _device_case(n, dt, 6600, family)
            hv = pl.payloads(family, n, 4, 6600)
            assert np.array_equal(keys.cpu().numpy().view(np.uint32), a) and np.array_equal(vals.cpu().numpy().view(np.uint32), hv)
            wk, wv, share = pl.device_expectation(keys, vals, dt, order)
            assert abs(share - pl.tied_fraction(a)) < 1e-6
            pl.compare(want, hv, wk, wv, what=("device-side expectation", family, order))
    for dt2 in (ol.U32, ol.I32):
        k2, v2 = _device_case(n, dt2, 6601, "random")
        wk, wv, _ = pl.device_expectation(k2, v2, dt2, ol.DESC)
        want = pl.Order(k2.cpu().numpy().view(np.uint32), dt2, ol.DESC)
        pl.compare(want, v2.cpu().numpy().view(np.uint32), wk, wv, what=("device-side expectation", dt2))
    _device_checked_sort(n, dt, 6600, "random")


@pytest.mark.parametrize("n_mi", [64, 160])
def test_without_histogram_in_the_largest_leaf_shapes(n_mi):
    """rsx_leafp_kernel's 2560- and 5120-pair shapes at the sizes that select them (64 Mi + 99 and 160 Mi + 99, as
    test_f32_ranks_and_pairs_without_histogram), against the device-side expectation pinned above."""
    if torch.cuda.mem_get_info()[0] < 16 * (1 << 30):
        pytest.skip("needs 16 GiB of free HBM")
    for family in ("reversed", "random"):
        _device_checked_sort(n_mi * MI + 99, ol.F32, 6600 + n_mi, family)
        torch.cuda.empty_cache()


# ---- F. an attempt called off after the spare buffers were written ----------------------------------------------------------
@pytest.mark.parametrize("digit", [0x05, 0xF3])
def test_attempt_called_off_after_the_spare_buffers_were_written(digit):
    """The construction of test_f32_pairs_level1_slot_overflows_after_the_spare_buffers_were_written: one top digit of the derived
    key with 1.4 times its share overflows its level-1 slot after the second key / payload buffers (0x05) or scratch (0xF3) were
    written.  The sort behind the attempt must start from the untouched first PAYLOAD buffer: random payloads say so per element."""
    n = 16 * MI + 3
    a = ol.splitmix_fill(n, ol.F32, 4660 + digit, 0xFFFFFFFF).view(np.uint32).copy()
    idx = np.arange(1000, 1000 + 26000 * 7, 7)
    top = (digit ^ 0x80) if digit >= 0x80 else (~digit & 0xFF)
    a[idx] = (a[idx] & np.uint32(0x00FFFFFF)) | np.uint32(top << 24)
    _sort(pl.Order(a, ol.F32), "random", 4, 6700 + digit, ("level-1 overflow", hex(digit)), not_route=5)


# ---- G. device-scheduled calls ---------------------------------------------------------------------------------------------
def _async_sort(want, family, seed, what, workspace=None, want_route=None):
    a = want.a
    vals = pl.payloads(family, a.size, 4, seed, keys=a)
    keys, v = _dev(a), _dev(vals)
    if workspace is None:
        rsa.radix_sort_pairs_inplace_async(keys, _junk(keys), v, _junk(v), dtype=want.dt, order=want.order)
        route = rsa.async_route()
    else:
        rsa.radix_sort_pairs_inplace_async_ws(keys, _junk(keys), v, _junk(v), workspace, dtype=want.dt, order=want.order)
        torch.cuda.synchronize()
        route = None
    pl.compare(want, vals, keys, v, route=route, want_route=want_route, what=(what, family, want.order))


@pytest.mark.parametrize("n,want_route", [(70001, 0), ((1 << 24) + 5, 5)])
@pytest.mark.parametrize("dt", [ol.F32, ol.U32], ids=["f32", "u32"])
def test_device_scheduled_pairs(dt, n, want_route):
    """rsx_sort_pairs_inplace_async: one pass per column at 70001 pairs, the attempt without a histogram from 16 Mi on; keys and
    payloads end in the first buffers."""
    for order in ORDERS if n < MI else (ol.ASC,):
        want = _order(pl.every_key_twice, n, dt, 6800 + dt, None, order)
        pl.assert_ties(want.a)
        for family in ("reversed", "random"):
            _async_sort(want, family, 6800 + dt, ("async", n), want_route=want_route)


@pytest.mark.parametrize("n", [70001, (1 << 24) + 5])
def test_device_scheduled_pairs_in_a_callers_workspace(n):
    """rsx_sort_pairs_inplace_async_ws with a workspace of exactly rsx_workspace_bytes(n, dtype, 4)."""
    ws = torch.empty(rsa.workspace_bytes(n, rsa.F32, 4), dtype=torch.uint8, device="cuda")
    want = _order(pl.every_key_twice, n, ol.F32, 6800 + ol.F32, None, ol.ASC)
    for family in ("reversed", "random", "edges"):
        _async_sort(want, family, 6850, ("async_ws", n), workspace=ws)


def test_device_scheduled_pairs_in_a_captured_graph():
    """One capture of the _ws call at 300001 pairs, replayed three times with keys AND payloads refilled: random, then reversed,
    then edges.  A graph that baked in anything about the first payloads fails the second replay."""
    n, dt = 300001, ol.F32
    s = torch.cuda.Stream()
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    vals = torch.empty(n, dtype=torch.int32, device="cuda")
    ks, vs = torch.empty_like(keys), torch.empty_like(vals)
    ws = torch.empty(rsa.workspace_bytes(n, dt, 4), dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(s):
        rsa.fill_splitmix(keys, seed=1, stream=s)
        rsa.fill_splitmix(vals, seed=2, stream=s)
        rsa.radix_sort_pairs_inplace_async_ws(keys, ks, vals, vs, ws, dtype=dt, stream=s)     # (the library's first use outside a capture)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rsa.radix_sort_pairs_inplace_async_ws(keys, ks, vals, vs, ws, dtype=dt, stream=torch.cuda.current_stream())
    for i, family in enumerate(("random", "reversed", "edges")):
        a = pl.assert_ties(pl.every_key_twice(n, dt, 6900 + i, 0xFFFFFFFF if i != 1 else 0x00FFFFFF))     # (four, then three kept columns)
        hv = pl.payloads(family, n, 4, 6900 + i, keys=a)
        keys.copy_(_dev(a))
        vals.copy_(_dev(hv))
        ks.fill_(0x5A5A5A5A)
        vs.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        pl.compare(pl.Order(a, dt), hv, keys, vals, what=("graph replay", i, family))


# ---- H. the library's own checker -------------------------------------------------------------------------------------------
def test_whole_result_verification_takes_any_payload(monkeypatch):
    """RSX_VERIFY=2 brackets a key + payload sort with a key sum and a PAIR mix: it must hold for payloads that are nothing like
    an index (the call succeeds), on one pass per column and on the route without a histogram, and the result is still right."""
    monkeypatch.setenv("RSX_VERIFY", "2")
    monkeypatch.setenv("RSX_NO_HYBRID", "1")
    _sort(pl.Order(pl.every_key_twice(300007, ol.U32, 7000), ol.U32), "random", 8, 7000, "verify=2, route 0", want_route=0)
    monkeypatch.delenv("RSX_NO_HYBRID")
    _sort(pl.Order(pl.every_key_twice(5 * MI + 99, ol.F32, 7001), ol.F32), "random", 4, 7001, "verify=2, route 5", want_route=5)


def test_pass_verification_of_a_device_scheduled_sort(monkeypatch):
    """RSX_VERIFY=1: one tile of every device-scheduled pass re-ranked with ballots; rsx_verify_poll finds no mismatch."""
    monkeypatch.setenv("RSX_VERIFY", "1")
    want = pl.Order(pl.every_key_twice(70001, ol.U32, 7002), ol.U32)
    _async_sort(want, "random", 7002, "verify=1, async")
    assert rsa.verify_poll() == 0
