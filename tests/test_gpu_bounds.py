"""Where the library writes: every writing entry point at every route, with every buffer it is given inside guard bands.

The rest of the suite compares results bit for bit; a result that is right says nothing about the memory around it.  The sort
without a histogram (rsx_info.hybrid == 5) puts up to 204 of its 256 level-1 slots into the caller's second buffer, the 8-byte
narrow level-1 form all 256 slots of four-byte places, key + payload and rank sorts spread theirs over both spares / both
halves of the index buffer, a called-off attempt has written there before the fallback runs, and the *_ws entry points keep
their state in a workspace the caller sized.  Here every buffer a call is handed -- sources, second buffers, spares, index
buffers, payloads, workspaces, histogram and destination arrays -- lies between two guard bands (tests/guard_lib.py: seeded
splitmix64 bytes), at 256-byte aligned and element-aligned-only residues; each case asserts the result against the oracle,
the route the size is meant to take, and that both bands of every buffer are intact afterwards.

Sizes are the library's own thresholds (the route-5 sizes in production geometry); RSX_TWO_LEVEL_MIN_LOG2=22 with
RSX_NO_BLIND=1 only for the histogram-first two-level route (4) at small sizes.  Guards of the cases whose slots could
overrun are sized from the slot geometry restated in guard_lib (slot_cap_for, level1_slot_cap) and asserted larger than
the largest overrun before anything is launched.
"""
import ctypes as C
import re

import numpy as np
import pytest

import guard_lib as gl
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MI = 1 << 20
GUARD = 4 << 20
_T = {4: torch.int32, 8: torch.int64}
LOW40 = (1 << 40) - 1
FULL64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()     # (no back-off from an earlier attempt that was called off: the route is asserted)
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


_oracle_memo = {}


def _oracle_sort(tag, a, dt, order):
    """ol.oracle_sort, kept for the next case on the same input (the aligned / unaligned pairs share one)."""
    key = (tag, dt, order)
    if key not in _oracle_memo:
        if len(_oracle_memo) >= 3:
            _oracle_memo.clear()
        _oracle_memo[key] = ol.oracle_sort(a, dt, order)
    return _oracle_memo[key]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def g_from(a, residue, guard=GUARD):
    a = np.ascontiguousarray(a)
    g = gl.guarded(a.size, _T[a.itemsize], residue, guard)
    g.load(a)
    return g


def g_empty(n, esize, residue, guard=GUARD):
    return gl.guarded(n, _T[esize], residue, guard)


def bits(t, dt):
    return t.cpu().numpy().view(ol.NP_BITS[dt])


def assert_keys_guard(n, ksize, guard, pad_kib=0, odd_stride=True):
    """A keys-only case of the sort without a histogram: the guard exceeds a whole slot past the last one in aux, and the narrow
    level-1 form's 256 slots (8-byte keys) if they did not fit."""
    cap1, lo = gl.level1_geometry(n, ksize, pad_kib, odd_stride)
    worst = max(gl.level1_slot_overrun(n, ksize, pad_kib, odd_stride), cap1 * ksize)
    if ksize == 8:
        worst = max(worst, gl.narrow1_overrun(n, 8, pad_kib, odd_stride))
    assert guard > worst, (guard, worst, cap1, lo)
    return cap1, lo


def sort_guarded(a, dt, order, src_res, aux_res, want_route, what, tag=None, guard=GUARD, route_not=None):
    """radix_sort (rsx_sort_device) with src and aux guarded; oracle result, returned buffer, kept columns, route, guards."""
    want, want_aux, winfo = _oracle_sort(tag, a, dt, order) if tag else ol.oracle_sort(a, dt, order)
    src = g_from(a, src_res, guard)
    aux = g_empty(a.size, a.itemsize, aux_res, guard)
    res, info = rsa.radix_sort(src.t, aux.t, dtype=dt, order=order)
    torch.cuda.synchronize()
    gl.check_all(("src " + what, src), ("aux " + what, aux))
    if route_not is not None:
        assert info.hybrid != route_not, (what, info.hybrid)
    else:
        assert info.hybrid == want_route, (what, info.hybrid)
    assert info.result_in_aux == want_aux, what
    assert info.kept_columns() == list(winfo.cols[:winfo.ncols]), what
    assert np.array_equal(bits(res, dt), want), what
    return info


# ---- route 5, 4-byte keys ------------------------------------------------------------------------------------------------

N64 = 64 * MI + 3


@pytest.mark.parametrize("dt,order,src_res,aux_res", [
    (ol.U32, ol.ASC, 0, 0), (ol.U32, ol.ASC, 0, 4), (ol.U32, ol.DESC, 4, 68), (ol.F32, ol.DESC, 0, 0), (ol.F32, ol.DESC, 0, 4)],
    ids=["u32-asc-aligned", "u32-asc-aux+4", "u32-desc-src+4-aux+68", "f32-desc-aligned", "f32-desc-aux+4"])
def test_route5_u32_64mi(dt, order, src_res, aux_res):
    """64 Mi keys: 195 level-1 slots in aux, the level-1 pass in 64-byte atoms -- into an aux that is 256-byte aligned and one
    that is only element-aligned (blind_wanted has no alignment gate: the atoms' 16-byte stores land off their boundaries)."""
    assert_keys_guard(N64, 4, GUARD)
    a = ol.splitmix_fill(N64, ol.U32, 9101)
    sort_guarded(a, dt, order, src_res, aux_res, 5, "route 5 %s" % ol.DTYPE_NAMES[dt], tag="u32-64mi")


N_FIT = 67092480     # 64 Mi - 16 Ki


def test_route5_u32_last_slot_ends_on_the_last_element():
    """n = 67 092 480: cap1 = 344 064 and lo = 195, so slot 194 ends exactly on aux's last element."""
    cap1, lo = assert_keys_guard(N_FIT, 4, GUARD)
    assert (cap1, lo) == (344064, 195) and lo * cap1 == N_FIT
    a = ol.splitmix_fill(N_FIT, ol.U32, 9102)
    for aux_res in (0, 4):
        sort_guarded(a, ol.U32, ol.ASC, 0, aux_res, 5, "exact fit, aux +%d" % aux_res, tag="u32-fit")


def test_route5_u32_called_off_after_level1_wrote():
    """At that size digit lo - 1 (its slot the last in aux) and digit 255 (the last slot, in scratch) get 1.4 times their share,
    spread evenly over the array -- too little for the sample to notice, too much for slots of 1.31 x the mean: the attempt is
    called off after its level-1 pass has written into aux, and the sort ends on one pass per column (route 0)."""
    cap1, lo = assert_keys_guard(N_FIT, 4, GUARD)
    mean = N_FIT >> 8
    assert 1.4 * mean > cap1 + 4 * int(np.sqrt(mean))      # (the two digits' counts lie far above their slots)
    a = ol.splitmix_fill(N_FIT, ol.U32, 9103).view(np.uint32).copy()
    extra = int(0.4 * (N_FIT >> 8))
    idx = np.arange(2 * extra, dtype=np.int64) * (N_FIT // (2 * extra)) + 17
    low = a[idx] & np.uint32(0x00FFFFFF)
    a[idx[0::2]] = low[0::2] | np.uint32((lo - 1) << 24)
    a[idx[1::2]] = low[1::2] | np.uint32(0xFF << 24)
    sort_guarded(a, ol.U32, ol.ASC, 0, 0, 0, "level-1 overflow in digits %d and 255" % (lo - 1))


# ---- 8-byte keys ---------------------------------------------------------------------------------------------------------

N24 = 3 * (1 << 23) + 4096      # the level-1 atom pass of 8-byte keys starts at 24 Mi keys


@pytest.mark.parametrize("aux_res", [0, 8], ids=["aux-aligned-narrow", "aux+8-wide"])
def test_route5_u64_below_2e40(aux_res):
    """Keys below 2^40: with a 64-byte aligned aux the level-1 slots hold four-byte low words, all 256 of them in aux (the narrow
    form); 8 bytes off, the form is not chosen and the slots hold whole keys -- route 5 either way."""
    assert_keys_guard(N24, 8, GUARD)
    assert gl.narrow1_overrun(N24) == 0
    a = ol.splitmix_fill(N24, ol.U64, 9201, LOW40)
    sort_guarded(a, ol.U64, ol.ASC, 0, aux_res, 5, "u64 < 2^40 aux +%d" % aux_res, tag="u64-40")


def test_route5_u64_full_width():
    assert_keys_guard(N24, 8, GUARD)
    a = ol.splitmix_fill(N24, ol.U64, 9202, FULL64)
    sort_guarded(a, ol.U64, ol.ASC, 8, 72, 5, "u64 full width, src +8, aux +72")
    sort_guarded(a, ol.I64, ol.DESC, 0, 0, 5, "i64 desc aligned")


def _zipf_like(n, seed, bmax=40):
    r = ol.splitmix_fill(n, ol.U64, seed)
    b = np.uint64(1) + ((r >> np.uint64(58)) % np.uint64(bmax))
    one = np.uint64(1)
    return (one << (b - one)) + (r & ((one << (b - one)) - one))


def test_route6_zipf_like_aligned_and_refused_unaligned():
    """(bit length, mantissa) digits: 64-byte atoms into aux.  8 bytes off, route 6 refuses the buffer -- the result is still
    right, and nothing is written outside it."""
    n = 3 * (1 << 23) + 77
    a = _zipf_like(n, 9203)
    sort_guarded(a, ol.U64, ol.ASC, 0, 0, 6, "zipf aligned", tag="zipf")
    sort_guarded(a, ol.U64, ol.ASC, 0, 8, None, "zipf aux +8", tag="zipf", route_not=6)
    sort_guarded(a, ol.U64, ol.ASC, 8, 0, None, "zipf src +8", tag="zipf", route_not=6)


# ---- pairs and ranks, route 5 ----------------------------------------------------------------------------------------------

N16 = 16 * MI + 5


def assert_pairs_guard(n, esize, guard):
    cap1, lo = gl.pairs_level1_geometry(n)
    assert guard > max((lo + 1) * cap1 * esize - n * esize, cap1 * esize), (guard, cap1, lo)


@pytest.mark.parametrize("dt,order,ks_res,vs_res", [(ol.U32, ol.ASC, 4, 68), (ol.F32, ol.DESC, 68, 0), (ol.F32, ol.ASC, 0, 4)],
                         ids=["u32-ks+4-vs+68", "f32-desc-ks+68-vs0", "f32-ks0-vs+4"])
def test_route5_pairs(dt, order, ks_res, vs_res):
    """Key + payload, 16 Mi + 5 pairs: the level-1 slots split over both spares, which lie at different residues."""
    assert_pairs_guard(N16, 4, GUARD)
    a = ol.splitmix_fill(N16, ol.U32, 9301).view(np.uint32).copy()
    a &= np.uint32(0xFFFFFF7F)          # (duplicates: stability shows in the payloads)
    perm = ol.stable_argsort_by_kdf(a, dt, order)
    _, want_aux, winfo = _oracle_sort("pairs", a, dt, order)
    vals = np.arange(N16, dtype=np.int32) * 3 + 1
    k, ks = g_from(a, 0), g_empty(N16, 4, ks_res)
    v, vs = g_from(vals, 0), g_empty(N16, 4, vs_res)
    rk, rv, info = rsa.radix_sort_pairs(k.t, ks.t, v.t, vs.t, dtype=dt, order=order)
    torch.cuda.synchronize()
    gl.check_all(("keys", k), ("keys spare", ks), ("vals", v), ("vals spare", vs))
    assert info.hybrid == 5, info.hybrid
    assert info.result_in_aux == want_aux and info.kept_columns() == list(winfo.cols[:winfo.ncols])
    assert np.array_equal(bits(rk, dt), a[perm])
    assert np.array_equal(rv.cpu().numpy().astype(np.int64), perm.astype(np.int64) * 3 + 1)


@pytest.mark.parametrize("dt,order,src_res,ib_res", [(ol.F32, ol.ASC, 4, 0), (ol.U32, ol.DESC, 0, 68)],
                         ids=["f32-src+4", "u32-desc-ib+68"])
def test_route5_rank(dt, order, src_res, ib_res):
    """Rank sort, 16 Mi + 5 keys: the slots in both halves of the index buffer; the source stays byte for byte as it was."""
    assert_pairs_guard(N16, 4, GUARD)
    a = ol.splitmix_fill(N16, ol.U32, 9302 + dt)
    want, whalf = ol.want_ranks(a, dt, order)
    src = g_from(a, src_res)
    before = src.t.clone()
    ib = g_empty(2 * N16, 4, ib_res)
    ranks, info = rsa.radix_sort_rank(src.t, ib.t, dtype=dt, order=order)
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("index buffer", ib))
    assert info.hybrid == 5, info.hybrid
    assert torch.equal(src.t, before), "the rank sort's source was written"
    assert info.result_in_aux == whalf
    assert np.array_equal(ranks.cpu().numpy().view(np.uint32), want)


def test_rank_sorted_input_leaves_the_second_half_alone():
    """rsx.h: pre-sorted input writes 0 .. n-1 to the first half and leaves the second untouched -- its contents are guarded
    like the bands around it."""
    a = np.sort(ol.splitmix_fill(N16, ol.U32, 9303))
    src = g_from(a, 4)
    ib = g_empty(2 * N16, 4, 0)
    second = ib.t[N16:].clone()
    ranks, info = rsa.radix_sort_rank(src.t, ib.t, dtype=ol.U32)
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("index buffer", ib))
    assert info.hybrid == 0 and info.early_exit == 2 and info.result_in_aux == 0, (info.hybrid, info.early_exit)
    assert torch.equal(ib.t[N16:], second), "the second half of the index buffer was written"
    assert np.array_equal(ranks.cpu().numpy(), np.arange(N16, dtype=np.int32))
    assert np.array_equal(bits(src.t, ol.U32), a)


# ---- routes 0, 1, 4 --------------------------------------------------------------------------------------------------------

N4 = (1 << 22) + 3


def test_route0_pairs_with_8byte_payloads():
    """8-byte payloads always go one pass per column."""
    a = ol.splitmix_fill(N4, ol.U32, 9401)
    perm = ol.stable_argsort_by_kdf(a, ol.U32)
    _, want_aux, _ = ol.oracle_sort(a, ol.U32)
    vals = np.arange(N4, dtype=np.int64) * 5 + (1 << 40)
    k, ks = g_from(a, 4), g_empty(N4, 4, 0)
    v, vs = g_from(vals, 8), g_empty(N4, 8, 72)
    rk, rv, info = rsa.radix_sort_pairs(k.t, ks.t, v.t, vs.t, dtype=ol.U32)
    torch.cuda.synchronize()
    gl.check_all(("keys", k), ("keys spare", ks), ("vals", v), ("vals spare", vs))
    assert info.hybrid == 0 and info.result_in_aux == want_aux, info.hybrid
    assert np.array_equal(bits(rk, ol.U32), a[perm])
    assert np.array_equal(rv.cpu().numpy(), perm.astype(np.int64) * 5 + (1 << 40))


def test_route0_rank_with_8byte_indices():
    a = ol.splitmix_fill(N4, ol.F32, 9402)
    want, whalf, _, _ = ol.oracle_rank(a, ol.F32, 8, ol.DESC)
    src = g_from(a, 0)
    before = src.t.clone()
    ib = g_empty(2 * N4, 8, 8)
    ranks, info = rsa.radix_sort_rank(src.t, ib.t, dtype=ol.F32, order=ol.DESC)
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("index buffer", ib))
    assert info.hybrid == 0 and info.result_in_aux == whalf, info.hybrid
    assert torch.equal(src.t, before)
    assert np.array_equal(ranks.cpu().numpy().view(np.uint64), want)


def test_route1_mid_size():
    """One MSB pass and leaves: keys, and a rank sort."""
    n = (1 << 21) + 3
    a = ol.splitmix_fill(n, ol.U32, 9403)
    sort_guarded(a, ol.U32, ol.ASC, 4, 68, 1, "keys route 1")
    b = ol.splitmix_fill(1000000, ol.U32, 9404)
    want, whalf, _, _ = ol.oracle_rank(b, ol.U32, 4)
    src, ib = g_from(b, 68), g_empty(2 * b.size, 4, 4)
    ranks, info = rsa.radix_sort_rank(src.t, ib.t, dtype=ol.U32)
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("index buffer", ib))
    assert info.hybrid == 1 and info.result_in_aux == whalf, info.hybrid
    assert np.array_equal(ranks.cpu().numpy().view(np.uint32), want)


def test_route4_histogram_first_slots(monkeypatch):
    """Two MSB passes with the second written into slack slots after the histogram (thresholds lowered for the size)."""
    monkeypatch.setenv("RSX_TWO_LEVEL_MIN_LOG2", "22")
    monkeypatch.setenv("RSX_NO_BLIND", "1")
    n = (1 << 23) + 4567
    a = ol.splitmix_fill(n, ol.U32, 9405)
    want, whalf, _, _ = ol.oracle_rank(a, ol.U32, 4, ol.DESC)
    src, ib = g_from(a, 4), g_empty(2 * n, 4, 68)
    ranks, info = rsa.radix_sort_rank(src.t, ib.t, dtype=ol.U32, order=ol.DESC)
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("index buffer", ib))
    assert info.hybrid == 4 and info.result_in_aux == whalf, info.hybrid
    assert np.array_equal(ranks.cpu().numpy().view(np.uint32), want)
    m = (1 << 23) + 321
    b = ol.splitmix_fill(m, ol.U32, 9406).view(np.uint32).copy()
    b &= np.uint32(0xFFFFFF0F)
    perm = ol.stable_argsort_by_kdf(b, ol.U32)
    vals = np.arange(m, dtype=np.int32) * 3 + 1
    k, ks, v, vs = g_from(b, 0), g_empty(m, 4, 4), g_from(vals, 68), g_empty(m, 4, 0)
    rk, rv, info = rsa.radix_sort_pairs(k.t, ks.t, v.t, vs.t, dtype=ol.U32)
    torch.cuda.synchronize()
    gl.check_all(("keys", k), ("keys spare", ks), ("vals", v), ("vals spare", vs))
    assert info.hybrid == 4, info.hybrid
    assert np.array_equal(bits(rk, ol.U32), b[perm])
    assert np.array_equal(rv.cpu().numpy().astype(np.int64), perm.astype(np.int64) * 3 + 1)


@pytest.mark.parametrize("dt", [ol.U32, ol.U64], ids=["u32", "u64"])
def test_small_one_workgroup_kernels_at_cap_and_cap_plus_one(dt):
    """n * key bytes = 64 KiB takes the one-launch kernel (route 0), one key more the general path (one MSB pass: route 1); the
    same for pairs and ranks at 2 n (key + payload bytes) = 128 KiB."""
    kb = ol.DTYPE_SIZE[dt]
    cap = 65536 // kb
    for n, route in ((cap, 0), (cap + 1, 1)):
        a = ol.splitmix_fill(n, dt, 9500 + n)
        sort_guarded(a, dt, ol.ASC, kb, 64 + kb, route, "keys n=%d" % n)
    pcap = 131072 // (2 * (kb + 4))
    for n in (pcap, pcap + 1):
        a = ol.splitmix_fill(n, dt, 9600 + n)
        perm = ol.stable_argsort_by_kdf(a, dt, ol.DESC)
        _, want_aux, _ = ol.oracle_sort(a, dt, ol.DESC)
        vals = np.arange(n, dtype=np.int32) + 11
        k, ks, v, vs = g_from(a, kb), g_empty(n, kb, 0), g_from(vals, 4), g_empty(n, 4, 68)
        rk, rv, info = rsa.radix_sort_pairs(k.t, ks.t, v.t, vs.t, dtype=dt, order=ol.DESC)
        torch.cuda.synchronize()
        gl.check_all(("keys", k), ("keys spare", ks), ("vals", v), ("vals spare", vs))
        if n == pcap:
            assert info.hybrid == 0, (n, info.hybrid)
        assert info.result_in_aux == want_aux, n
        assert np.array_equal(bits(rk, dt), a[perm]) and np.array_equal(rv.cpu().numpy(), perm.astype(np.int32) + 11), n
        want, whalf, _, _ = ol.oracle_rank(a, dt, 4)
        src, ib = g_from(a, 64 + kb), g_empty(2 * n, 4, 4)
        ranks, info = rsa.radix_sort_rank(src.t, ib.t, dtype=dt)
        torch.cuda.synchronize()
        gl.check_all(("src", src), ("index buffer", ib))
        if n == pcap:
            assert info.hybrid == 0, (n, info.hybrid)
        assert info.result_in_aux == whalf and np.array_equal(ranks.cpu().numpy().view(np.uint32), want), n


# ---- device-scheduled sorts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,n,mask,buf_res,scr_res", [(ol.U32, 16 * MI + 3, 0xFFFFFFFF, 0, 4), (ol.F32, 16 * MI + 3, 0xFFFFFFFF, 4, 68),
                                                         (ol.U64, N24, LOW40, 0, 0), (ol.U64, N24, FULL64, 8, 8)],
                         ids=["u32-scratch+4", "f32-buf+4-scratch+68", "u64-40-aligned", "u64-full-buf+8-scratch+8"])
def test_route5_inplace_async(dt, n, mask, buf_res, scr_res):
    kb = ol.DTYPE_SIZE[dt]
    assert_keys_guard(n, kb, GUARD)
    a = ol.splitmix_fill(n, dt, 9700 + dt, mask)
    want, _, _ = ol.oracle_sort(a, dt)
    buf, scr = g_from(a, buf_res), g_empty(n, kb, scr_res)
    rsa.radix_sort_inplace_async(buf.t, scr.t, dtype=dt)
    assert rsa.async_route() == 5
    gl.check_all(("buf", buf), ("scratch", scr))
    assert np.array_equal(bits(buf.t, dt), want)


def test_route5_pairs_and_rank_inplace_async():
    a = ol.splitmix_fill(N16, ol.U32, 9710)
    perm = ol.stable_argsort_by_kdf(a, ol.F32, ol.DESC)
    assert_pairs_guard(N16, 4, GUARD)
    vals = np.arange(N16, dtype=np.int32) * 7 + 2
    k, ks, v, vs = g_from(a, 4), g_empty(N16, 4, 68), g_from(vals, 0), g_empty(N16, 4, 4)
    rsa.radix_sort_pairs_inplace_async(k.t, ks.t, v.t, vs.t, dtype=ol.F32, order=ol.DESC)
    assert rsa.async_route() == 5
    gl.check_all(("keys", k), ("keys scratch", ks), ("vals", v), ("vals scratch", vs))
    assert np.array_equal(bits(k.t, ol.F32), a[perm])
    assert np.array_equal(v.t.cpu().numpy().astype(np.int64), perm.astype(np.int64) * 7 + 2)
    want, _ = ol.want_ranks(a, ol.U32)
    src, ib = g_from(a, 68), g_empty(2 * N16, 4, 4)
    before = src.t.clone()
    ranks = rsa.radix_sort_rank_inplace_async(src.t, ib.t, dtype=ol.U32)
    assert rsa.async_route() == 5
    gl.check_all(("src", src), ("index buffer", ib))
    assert torch.equal(src.t, before)
    assert np.array_equal(ranks.cpu().numpy().view(np.uint32), want)



_DEBUG_ROUTE = re.compile(r"narrow (\d+) .*slots in the second buffer (\d+) cap1 (\d+)")


@pytest.mark.parametrize("case", ["u32", "u64-40-aligned", "u64-40-scratch+8", "u64-40-pad512"])
def test_level1_geometry_as_the_library_reports_it(case, monkeypatch, capfd):
    """rsx_async_route under RSX_DEBUG_ROUTE=1 prints what the attempt used: the restated cap1 and `lo` (how many slots lie in
    the caller's scratch buffer) are the library's, and the narrow level-1 form (SegCtl::narrow == 2) runs exactly where its 256
    slots fit a 64-byte aligned scratch buffer -- not 8 bytes off, and not with RSX_CAP1_PAD_KIB=512, where they would end
    ~8 MiB past its end (the guard is larger than that)."""
    dt, n, mask, scr_res, pad = {"u32": (ol.U32, 16 * MI + 3, 0xFFFFFFFF, 0, 0), "u64-40-aligned": (ol.U64, N24, LOW40, 0, 0),
                                 "u64-40-scratch+8": (ol.U64, N24, LOW40, 8, 0), "u64-40-pad512": (ol.U64, N24, LOW40, 0, 512)}[case]
    kb = ol.DTYPE_SIZE[dt]
    guard = 16 << 20
    cap1, lo = assert_keys_guard(n, kb, guard, pad)
    narrow_fits = kb == 8 and gl.narrow1_overrun(n, kb, pad) == 0
    assert narrow_fits == (case == "u64-40-aligned" or case == "u64-40-scratch+8")
    if pad:
        monkeypatch.setenv("RSX_CAP1_PAD_KIB", str(pad))
    monkeypatch.setenv("RSX_DEBUG_ROUTE", "1")
    a = ol.splitmix_fill(n, dt, 9740 + dt, mask)
    want, _, _ = ol.oracle_sort(a, dt)
    buf, scr = g_from(a, 0, guard), g_empty(n, kb, scr_res, guard)
    capfd.readouterr()
    rsa.radix_sort_inplace_async(buf.t, scr.t, dtype=dt)
    assert rsa.async_route() == 5
    m = _DEBUG_ROUTE.search(capfd.readouterr().err)
    assert m, "rsx_async_route printed nothing under RSX_DEBUG_ROUTE=1"
    narrow, got_lo, got_cap1 = (int(x) for x in m.groups())
    assert (got_cap1, got_lo) == (cap1, lo), case
    assert (narrow == 2) == (case == "u64-40-aligned"), (case, narrow)
    gl.check_all(("buf", buf), ("scratch", scr))
    assert np.array_equal(bits(buf.t, dt), want)

@pytest.mark.parametrize("dt,n,mask,scr_res", [(ol.U32, 16 * MI + 3, 0xFFFFFFFF, 4), (ol.U64, N24, LOW40, 0), (ol.U64, N24, LOW40, 8)],
                         ids=["u32-scratch+4", "u64-40-aligned", "u64-40-scratch+8"])
def test_route5_inplace_async_ws(dt, n, mask, scr_res):
    """rsx_sort_inplace_async_ws inside a workspace of exactly rsx_workspace_bytes_fast(n) bytes, 256-byte aligned, guarded."""
    kb = ol.DTYPE_SIZE[dt]
    assert_keys_guard(n, kb, GUARD)
    a = ol.splitmix_fill(n, dt, 9720 + dt, mask)
    want, _, _ = ol.oracle_sort(a, dt)
    ws = gl.Guarded(rsa.workspace_bytes_fast(n, dt), torch.uint8, 0, GUARD)
    buf, scr = g_from(a, 0), g_empty(n, kb, scr_res)
    rsa.radix_sort_inplace_async_ws(buf.t, scr.t, ws.t, dtype=dt)
    assert rsa.async_route_ws(ws.t, n, dt) == 5
    gl.check_all(("buf", buf), ("scratch", scr), ("workspace", ws))
    assert np.array_equal(bits(buf.t, dt), want)


def test_pairs_inplace_async_ws():
    """rsx_sort_pairs_inplace_async_ws inside a workspace of exactly rsx_workspace_bytes(n, dtype, 4) bytes: histogram first."""
    a = ol.splitmix_fill(N16, ol.U32, 9730)
    perm = ol.stable_argsort_by_kdf(a, ol.U32)
    vals = np.arange(N16, dtype=np.int32) ^ 0x55
    ws = gl.Guarded(rsa.workspace_bytes(N16, ol.U32, 4), torch.uint8, 0, GUARD)
    k, ks, v, vs = g_from(a, 0), g_empty(N16, 4, 4), g_from(vals, 68), g_empty(N16, 4, 0)
    rsa.radix_sort_pairs_inplace_async_ws(k.t, ks.t, v.t, vs.t, ws.t, dtype=ol.U32)
    assert rsa.async_route_ws(ws.t, N16, ol.U32) == 0
    gl.check_all(("keys", k), ("keys scratch", ks), ("vals", v), ("vals scratch", vs), ("workspace", ws))
    assert np.array_equal(bits(k.t, ol.U32), a[perm])
    assert np.array_equal(v.t.cpu().numpy(), vals[perm])


# ---- other writers ---------------------------------------------------------------------------------------------------------

def test_records_tagged_device():
    """12-byte records with a u32 key at byte 4, both buffers off 256-byte boundaries: key extraction, rank sort, gather."""
    n, rb, off = 1000003, 12, 4
    rng = np.random.default_rng(9801)
    rec = rng.integers(0, 256, size=(n, rb), dtype=np.uint8)
    rec[:, off:off + 4] = ol.splitmix_fill(n, ol.U32, 9802).view(np.uint8).reshape(n, 4)
    s2, a2 = rec.copy(), np.full_like(rec, 0x5A)
    oinfo = ol.Info()
    r = ol.oracle().rso_sort_records(ol.ptr(s2), ol.ptr(a2), n, rb, off, ol.U32, ol.ASC, C.byref(oinfo))
    want = a2 if r else s2
    src = gl.Guarded(n * rb, torch.uint8, 4, GUARD)
    src.load(rec)
    aux = gl.Guarded(n * rb, torch.uint8, 68, GUARD)
    res, info = rsa.radix_sort_records_tagged(src.t, aux.t, rb, off, ol.U32)
    torch.cuda.synchronize()
    gl.check_all(("records", src), ("records aux", aux))
    assert info.hybrid == 1 and info.result_in_aux == r, info.hybrid
    assert np.array_equal(res.cpu().numpy().reshape(n, rb), want)


@pytest.mark.parametrize("dt", [ol.U32, ol.U64], ids=["u32", "u64"])
def test_histogram_and_msd_split_device(dt):
    """rsx_histogram_device into a guarded count array and flag word; rsx_msd_split_device and rsx_msd_split_async into a guarded
    destination."""
    kb = ol.DTYPE_SIZE[dt]
    n = 3000017
    a = ol.splitmix_fill(n, dt, 9900 + dt)
    src = g_from(a, kb)
    hist = gl.guarded(256 * kb, torch.int64, 8, 1 << 16)
    flag = gl.guarded(1, torch.int32, 4, 1 << 16)
    rsa.check(rsa.lib().rsx_histogram_device(src.t.data_ptr(), n, dt, 0, hist.t.data_ptr(), flag.t.data_ptr(), _stream()))
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("d_hist", hist), ("d_unsorted", flag))
    k = ol.kdf_keys(a, dt)
    got = hist.t.cpu().numpy()
    for j in range(kb):
        dig = ((k >> ol.NP_BITS[dt](8 * j)) & ol.NP_BITS[dt](0xFF)).astype(np.int64)
        assert np.array_equal(got[256 * j:256 * j + 256], np.bincount(dig, minlength=256)), j
    assert int(flag.t.item()) == 1
    top = (k >> ol.NP_BITS[dt](8 * (kb - 1))).astype(np.int64)
    want = a[np.argsort(top, kind="stable")]
    dst = g_empty(n, kb, 64 + kb)
    top_hist = np.zeros(256, dtype=np.uint64)
    rsa.check(rsa.lib().rsx_msd_split_device(src.t.data_ptr(), dst.t.data_ptr(), n, dt, 0, -1, top_hist.ctypes.data, _stream()))
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("d_dst", dst))
    assert np.array_equal(top_hist, np.bincount(top, minlength=256).astype(np.uint64))
    assert np.array_equal(bits(dst.t, dt), want)
    assert np.array_equal(bits(src.t, dt), a)
    dst2 = g_empty(n, kb, 0)
    rsa.check(rsa.lib().rsx_msd_split_async(src.t.data_ptr(), dst2.t.data_ptr(), n, dt, 0, kb - 1, hist.t.data_ptr(), _stream()))
    torch.cuda.synchronize()
    gl.check_all(("src", src), ("d_hist", hist), ("d_dst", dst2))
    assert np.array_equal(bits(dst2.t, dt), want)


# ---- probe switches that change the slot geometry (8-byte keys below 2^40, route 5) ---------------------------------------

def test_cap1_pad_at_the_narrow_form_size(monkeypatch):
    """RSX_CAP1_PAD_KIB=512: 256 slots of cap1 four-byte places would end ~8 MiB past aux (the narrow form must not be chosen);
    the guard is larger than that whole overrun, so every write stays inside this test's allocation either way."""
    pad = 512
    overrun = gl.narrow1_overrun(N24, 8, pad)
    assert overrun == 8355840
    guard = 16 << 20
    assert_keys_guard(N24, 8, guard, pad)
    assert guard > overrun
    monkeypatch.setenv("RSX_CAP1_PAD_KIB", str(pad))
    a = ol.splitmix_fill(N24, ol.U64, 9201, LOW40)
    sort_guarded(a, ol.U64, ol.ASC, 0, 0, 5, "RSX_CAP1_PAD_KIB=%d" % pad, tag="u64-40", guard=guard)


def test_pass32_lowered(monkeypatch):
    """RSX_PASS32_MIN_MI=8: the level-1 atom pass (and the narrow form) at 10 Mi keys, slots of 51 200 keys."""
    n = 10 * MI + 7
    assert_keys_guard(n, 8, GUARD)
    assert gl.narrow1_overrun(n) == 0
    monkeypatch.setenv("RSX_PASS32_MIN_MI", "8")
    a = ol.splitmix_fill(n, ol.U64, 9211, LOW40)
    sort_guarded(a, ol.U64, ol.ASC, 0, 0, 5, "RSX_PASS32_MIN_MI=8")
    sort_guarded(a, ol.U64, ol.DESC, 0, 8, 5, "RSX_PASS32_MIN_MI=8, desc, aux +8")


def test_no_odd_stride(monkeypatch):
    """RSX_NO_ODD_STRIDE=1 at 2^25 + 4096 keys, where the slots are a MiB and more: 204 slots of 164 096 keys in aux instead of
    195 of 172 032."""
    n = (1 << 25) + 4096
    assert gl.level1_geometry(n, 8, odd_stride=False) == (164096, 204)
    assert_keys_guard(n, 8, GUARD, odd_stride=False)
    monkeypatch.setenv("RSX_NO_ODD_STRIDE", "1")
    a = ol.splitmix_fill(n, ol.U64, 9221, LOW40)
    sort_guarded(a, ol.U64, ol.ASC, 0, 0, 5, "RSX_NO_ODD_STRIDE=1")
