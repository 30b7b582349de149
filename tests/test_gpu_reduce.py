"""rsx_sort_reduce_device on the GPU: the groups' keys, counts, sums, minima and maxima against the oracle (tests/reduce_lib.py),
every route asserted where a case was written for it (so that none passes by falling back): the cells in LDS with every value
type, both orders, one and many copies, a heavy key for both branches of the peel, the cut-off to the cells in device memory;
the sort route's tile boundaries, seams and sorted input; wide sums, sign extension, wrap-around, special floats by bit pattern,
exact and bounded float sums; every subset of the outputs, both index widths, and the host form."""
import functools
import itertools

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa
import reduce_lib as rl
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_IT = {4: torch.int32, 8: torch.int64}
ROUTE = {0: "TRIVIAL", 1: "CELLS_LDS", 2: "CELLS_GLOBAL", 3: "SORT"}
ALL = rl.SUM | rl.MIN | rl.MAX
TILE = {1: 32768, 2: 16384, 4: 8192, 8: 4096}     # unique_heads_tile<KT>(): 4 sweeps of 512 threads x one 16-byte vector
N20 = (1 << 20) + 3
MASK12 = 0x00F0F00F                              # 12 varying bits in three runs


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(bits, dt):
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    return torch.from_numpy(a.view(ul.SIGNED[ol.DTYPE_SIZE[dt]]).copy()).cuda()


def run(kbits, dt, vbits, vdt, order=ol.ASC, ib=4, ops=ALL, keys=True, counts=True):
    """radix_sort_reduce on device copies: (keys, counts, sum, min, max, info), the arrays back on the host as bit patterns (counts
    and sums as uint64), None where one was not asked for.  Keys and values on the device are compared with the copies
    afterwards: neither is ever written."""
    ka = np.ascontiguousarray(kbits, dtype=ol.NP_BITS[dt])
    va = np.ascontiguousarray(vbits, dtype=ol.NP_BITS[vdt])
    k, v = dev(ka, dt), dev(va, vdt)
    out = rsa.radix_sort_reduce(k, v, dtype=dt, val_dtype=vdt, order=order, idx_dtype=_IT[ib], sum=bool(ops & rl.SUM), min=bool(ops & rl.MIN),
                                max=bool(ops & rl.MAX), counts=counts, keys_out=keys)
    torch.cuda.synchronize()
    assert np.array_equal(k.cpu().numpy().view(ol.NP_BITS[dt]), ka), "keys were written"
    assert np.array_equal(v.cpu().numpy().view(ol.NP_BITS[vdt]), va), "values were written"
    ok, cn, sm, mn, mx, info = out
    host = lambda t, w: None if t is None else t.cpu().numpy().view(w)
    cn = host(cn, np.uint32 if ib == 4 else np.uint64)
    return (host(ok, ol.NP_BITS[dt]), None if cn is None else cn.astype(np.uint64), host(sm, np.uint64), host(mn, ol.NP_BITS[vdt]),
            host(mx, ol.NP_BITS[vdt]), info)


@functools.lru_cache(maxsize=8)
def _groups_cached(key):
    return rl.groups(*_GROUP_ARGS[key])


_GROUP_ARGS = {}


def groups_of(kbits, dt, order, tag=None):
    """rl.groups, computed once per tagged input and shared by the cases that use it."""
    if tag is None:
        return rl.groups(kbits, dt, order)
    _GROUP_ARGS[(tag, dt, order)] = (kbits, dt, order)
    return _groups_cached((tag, dt, order))


def compare(got, want, tag, sums=True):
    for name, g, w in zip(("keys", "counts", "sum", "min", "max"), got, want):
        if g is None or w is None or (name == "sum" and not sums):
            continue
        assert g.size == w.size, "%s: %s has %d entries, oracle %d" % (tag, name, g.size, w.size)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s: %s differs from the oracle in %d places, first at %d: %#x != %#x" % (
            tag, name, bad.size, bad[0], int(g[bad[0]]), int(w[bad[0]]))


def check(kbits, dt, vbits, vdt, order=ol.ASC, route=None, ib=4, ops=ALL, what="", tag=None, sums=True):
    grp = groups_of(kbits, dt, order, tag)
    want = rl.want_reduce(grp, vbits, vdt, float_sums=sums)
    got = run(kbits, dt, vbits, vdt, order, ib, ops)
    info = got[5]
    label = "%s kdt=%d vdt=%d order=%d n=%d ib=%d route=%s" % (what, dt, vdt, order, np.asarray(kbits).size, ib, ROUTE.get(info.route))
    if route is not None:
        assert info.route == route, label + ": expected route " + ROUTE[route]
    compare(got[:5], want, label, sums)
    assert info.sort.key_bytes == ol.DTYPE_SIZE[dt]
    return got, want


# ---- the cells in LDS ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def keys12():
    return ol.splitmix_fill(N20, ol.U32, 9101, MASK12)


@pytest.mark.parametrize("vdt", rl.VAL_DTYPES)
def test_cells_lds_every_value_type(keys12, vdt):
    v = rl.small_ints(N20, vdt, 9110 + vdt)
    got, _ = check(keys12, ol.U32, v, vdt, route=rsa.REDUCE_CELLS_LDS, what="12 bits, three runs", tag="keys12")
    assert got[5].varying_bits == 12 and got[5].table_bytes == 4096 * (16 + 2 * ol.DTYPE_SIZE[vdt])
    assert got[0].size == 4096


def test_cells_lds_descending_and_small(keys12):
    v = rl.small_ints(N20, ol.I32, 9120)
    check(keys12, ol.U32, v, ol.I32, order=ol.DESC, route=rsa.REDUCE_CELLS_LDS, what="desc", tag="keys12")
    check(keys12[:77], ol.U32, v[:77], ol.I32, route=rsa.REDUCE_CELLS_LDS, what="77 keys")
    check(keys12[:77], ol.U32, v[:77], ol.I32, order=ol.DESC, route=rsa.REDUCE_CELLS_LDS, ib=8, what="77 keys desc, 8-byte counts")
    check(keys12[:2], ol.U32, v[:2], ol.I32, what="two keys")


def test_cells_lds_one_byte_keys_and_float_keys():
    b = ol.splitmix_fill(N20 + 4, ol.U8, 9130)
    b[b == 7] = 9                 # (an empty cell inside the column)
    v = rl.small_ints(b.size, ol.F64, 9131)
    got, _ = check(b, ol.I8, v, ol.F64, order=ol.DESC, route=rsa.REDUCE_CELLS_LDS, what="i8 desc")
    assert got[0].size == 255 and got[5].varying_bits == 8
    check(b[:100], ol.U8, v[:100], ol.F64, route=rsa.REDUCE_CELLS_LDS, what="u8, 100 keys")
    # float keys of one sign, +0.0 among them: few bits vary
    f = np.array([0.0, 1.0, 2.0, 0.5, 4.0, 0.25], dtype=np.float32).view(np.uint32)
    rng = np.random.default_rng(9132)
    fk = f[rng.integers(0, f.size, 50001)]
    fv = rl.small_ints(fk.size, ol.U32, 9133)
    for order in (ol.ASC, ol.DESC):
        got, _ = check(fk, ol.F32, fv, ol.U32, order, rsa.REDUCE_CELLS_LDS, what="f32 keys of one sign")
        assert got[0].size == 6 and int(got[0][0 if order == ol.ASC else 5]) == 0
    # -0.0 beside +0.0: the float KDF complements negative keys, so EVERY bit differs between the two zeros -- keys that hold both
    # cannot have few varying bits, and take the sort route; the zeros are groups of their own, -0.0 below +0.0
    g = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dtype=np.float32).view(np.uint32)
    gk = g[rng.integers(0, g.size, 50001)]
    for order in (ol.ASC, ol.DESC):
        got, _ = check(gk, ol.F32, fv, ol.U32, order, rsa.REDUCE_SORT, what="f32 keys with both zeros")
        assert got[0].size == 8 and got[5].varying_bits == 32
        z = [int(x) for x in got[0] if (int(x) & 0x7FFFFFFF) == 0]
        assert z == ([0x80000000, 0] if order == ol.ASC else [0, 0x80000000])


def test_cells_lds_one_copy_and_many(keys12, monkeypatch):
    """RSX_REDUCE_REPLICAS=1: every lane on the one copy; the default for sums alone of 256 cells: 32 copies."""
    k8 = ol.splitmix_fill(N20, ol.U32, 9140, 0x0000FF00)
    v = rl.small_ints(N20, ol.F32, 9141)
    check(k8, ol.U32, v, ol.F32, route=rsa.REDUCE_CELLS_LDS, ops=rl.SUM, what="256 cells, sums, default copies")
    monkeypatch.setenv("RSX_REDUCE_REPLICAS", "1")
    rsa.reload_env()
    check(k8, ol.U32, v, ol.F32, route=rsa.REDUCE_CELLS_LDS, ops=rl.SUM, what="256 cells, sums, one copy")
    check(keys12, ol.U32, v, ol.F32, route=rsa.REDUCE_CELLS_LDS, what="4096 cells, one copy", tag="keys12")
    monkeypatch.setenv("RSX_REDUCE_REPLICAS", "4")
    rsa.reload_env()
    check(k8, ol.U32, v, ol.F32, route=rsa.REDUCE_CELLS_LDS, what="256 cells, four copies")


def skewed(n, dt, mask, seed, share=0.95):
    """`share` of the elements on one key, the rest spread under `mask`: whole waves on one cell and waves with a few strays."""
    a = ol.splitmix_fill(n, dt, seed, mask)
    heavy = np.random.default_rng(seed).random(n) < share
    a[heavy] = a[0]
    return a


@pytest.mark.parametrize("vdt", [ol.U32, ol.F64, ol.I64])
def test_cells_lds_heavy_key(vdt):
    a = skewed(N20, ol.U32, MASK12, 9150)
    v = rl.small_ints(N20, vdt, 9151)
    got, _ = check(a, ol.U32, v, vdt, route=rsa.REDUCE_CELLS_LDS, what="95 % on one key", tag="skew12")
    assert int(got[1].max()) > 0.9 * N20


def test_cells_cut_off_between_lds_and_device_memory(monkeypatch):
    """V = 12 is the last size whose cells lie in LDS.  V = 13 takes the sort by default (RSX_REDUCE_MAX_BITS = 12: the cells in
    device memory lost every measured row) and the cells in device memory where RSX_REDUCE_MAX_BITS admits them."""
    v = rl.small_ints(N20, ol.F32, 9160)
    keys = {}
    for vbits in (12, 13):
        a = ol.splitmix_fill(N20, ol.U32, 9161 + vbits, (1 << vbits) - 1)
        a[:2] = (0, (1 << vbits) - 1)
        keys[vbits] = a
    for vbits, route in ((12, rsa.REDUCE_CELLS_LDS), (13, rsa.REDUCE_SORT)):
        got, _ = check(keys[vbits], ol.U32, v, ol.F32, route=route, what="v%d" % vbits, tag="cut%d" % vbits)
        # (13 bits are proven by the sample of the keys: no plan is made, and the varying bits are "not computed")
        assert got[5].varying_bits == (vbits if vbits == 12 else 0)
    monkeypatch.setenv("RSX_REDUCE_MAX_BITS", "16")
    rsa.reload_env()
    for vbits, route in ((12, rsa.REDUCE_CELLS_LDS), (13, rsa.REDUCE_CELLS_GLOBAL)):
        got, _ = check(keys[vbits], ol.U32, v, ol.F32, route=route, what="v%d, MAX_BITS=16" % vbits, tag="cut%d" % vbits)
        assert got[5].varying_bits == vbits


def test_cells_lds_bits_switch(monkeypatch, keys12):
    monkeypatch.setenv("RSX_REDUCE_LDS_BITS", "8")
    rsa.reload_env()
    v = rl.small_ints(N20, ol.U32, 9165)
    check(keys12, ol.U32, v, ol.U32, route=rsa.REDUCE_CELLS_GLOBAL, what="LDS_BITS=8", tag="keys12")
    monkeypatch.setenv("RSX_REDUCE_MAX_BITS", "8")
    rsa.reload_env()
    check(keys12, ol.U32, v, ol.U32, route=rsa.REDUCE_SORT, what="MAX_BITS=8", tag="keys12")


# ---- ... in device memory ---------------------------------------------------------------------------------------------------

GLOBAL_CASES = [("u32-v13", ol.U32, 0x1FFF, 13), ("u32-v16", ol.U32, 0x00F0FF0F, 16), ("u64-v13", ol.U64, 0x1FFF00000000, 13),
                ("u64-v16", ol.U64, 0xFF000000FF00, 16)]


@pytest.mark.parametrize("case", GLOBAL_CASES, ids=[c[0] for c in GLOBAL_CASES])
def test_cells_global(case, monkeypatch):
    """V = 13 and V = RSX_REDUCE_MAX_BITS, here 16 (the route is off by default)."""
    monkeypatch.setenv("RSX_REDUCE_MAX_BITS", "16")
    rsa.reload_env()
    name, dt, mask, vbits = case
    n = (1 << 19) + 5
    a = ol.splitmix_fill(n, dt, 9170 + vbits, mask)
    v = rl.small_ints(n, ol.F64, 9171)
    got, _ = check(a, dt, v, ol.F64, route=rsa.REDUCE_CELLS_GLOBAL, what=name)
    assert got[5].varying_bits == vbits and got[5].table_bytes == (1 << vbits) * 32
    w = rl.small_ints(n, ol.I32, 9172)
    check(a, dt, w, ol.I32, order=ol.DESC, route=rsa.REDUCE_CELLS_GLOBAL, what=name + " desc")
    s = skewed(n, dt, mask, 9173 + vbits)
    check(s, dt, w, ol.I32, route=rsa.REDUCE_CELLS_GLOBAL, what=name + " 95 % on one key")


def test_first_size_beyond_the_cells(monkeypatch):
    monkeypatch.setenv("RSX_REDUCE_MAX_BITS", "16")
    rsa.reload_env()
    n = (1 << 18) + 1
    a = ol.splitmix_fill(n, ol.U32, 9180, 0x1FFFF)
    a[:2] = (0, 0x1FFFF)
    v = rl.small_ints(n, ol.U32, 9181)
    got, _ = check(a, ol.U32, v, ol.U32, route=rsa.REDUCE_SORT, what="v17")
    assert got[5].varying_bits == 0 and got[5].table_bytes == 0       # (the sample proves 17 bits: no plan, nothing computed)
    got, _ = check(a[:60001], ol.U32, v[:60001], ol.U32, route=rsa.REDUCE_SORT, what="v17, below the sample's floor")
    assert got[5].varying_bits == 17 and got[5].table_bytes == 0


# ---- the sort route -----------------------------------------------------------------------------------------------------------

def runs_of(sizes, dt, seed):
    """Keys whose SORTED order has runs of the given sizes, shuffled: the group keys are distinct random bit patterns."""
    rng = np.random.default_rng(seed)
    width = ol.DTYPE_SIZE[dt] * 8
    vals = set()
    while len(vals) < len(sizes):
        vals.add(int(rng.integers(0, 1 << min(width, 40))) if width > 16 else int(rng.integers(0, 1 << width)))
    vals = np.array(sorted(vals), dtype=ol.NP_BITS[dt])
    a = np.repeat(vals, sizes)
    return a, rng.permutation(a.size)


@pytest.mark.parametrize("dt,vdt", [(ol.U32, ol.I32), (ol.U64, ol.F64), (ol.U32, ol.U64), (ol.U64, ol.F32)])
def test_sort_tile_boundaries_and_seams(dt, vdt):
    """In the sorted array: group boundaries at tile - 1, tile and tile + 1, a head exactly on a tile start (2 tile), a run over
    three whole tiles with heads on both sides, and the last run ending at n."""
    t = TILE[ol.DTYPE_SIZE[dt]]
    sizes = [t - 1, 1, 1, t - 1, 3, 4 * t + 11, 9, 100]
    a, perm = runs_of(sizes, dt, 9200 + dt)
    assert np.cumsum(sizes)[3] == 2 * t
    v = rl.small_ints(a.size, vdt, 9201)
    got, _ = check(a[perm], dt, v, vdt, route=rsa.REDUCE_SORT, what="boundaries")
    assert list(got[1]) == sizes and got[5].sort.early_exit == 0
    # the same keys in order: nothing is copied and nothing is sorted
    got, _ = check(a, dt, v, vdt, route=rsa.REDUCE_SORT, what="boundaries, sorted input")
    assert list(got[1]) == sizes and got[5].sort.early_exit == 2
    got, _ = check(a[::-1].copy(), dt, v, vdt, order=ol.DESC, route=rsa.REDUCE_SORT, ib=8, what="boundaries, sorted descending")
    assert list(got[1]) == sizes[::-1] and got[5].sort.early_exit == 2


def test_sort_all_keys_equal_is_trivial():
    for dt, vdt in ((ol.U32, ol.F32), (ol.U64, ol.I64)):
        n = 3 * TILE[ol.DTYPE_SIZE[dt]] + 5
        a = np.full(n, 0x1234567, dtype=ol.NP_BITS[dt])
        v = rl.small_ints(n, vdt, 9210)
        got, _ = check(a, dt, v, vdt, route=rsa.REDUCE_TRIVIAL, what="all equal")
        assert got[0].size == 1 and int(got[1][0]) == n and got[5].varying_bits == 0


def test_sort_random_keys():
    n = (1 << 18) + 77
    v8 = rl.small_ints(n, ol.U64, 9220)
    check(ol.splitmix_fill(n, ol.U32, 9221), ol.U32, v8, ol.U64, route=rsa.REDUCE_SORT, what="uniform u32, 8-byte values")
    check(ol.splitmix_fill(n, ol.U64, 9222, (1 << 40) - 1), ol.U64, v8, ol.I64, order=ol.DESC, route=rsa.REDUCE_SORT, what="u64 below 2^40")
    # duplicates: 2^18 draws from 2^17 + 3 distinct wide keys
    pool = ol.splitmix_fill((1 << 17) + 3, ol.U32, 9223)
    a = pool[np.random.default_rng(9224).integers(0, pool.size, n)]
    check(a, ol.F32, rl.small_ints(n, ol.F32, 9225), ol.F32, route=rsa.REDUCE_SORT, what="f32 keys with duplicates")
    got, _ = check(np.sort(a), ol.U32, v8, ol.U64, route=rsa.REDUCE_SORT, what="sorted u32 with duplicates")
    assert got[5].sort.early_exit == 2


def test_sort_forced(monkeypatch, keys12):
    monkeypatch.setenv("RSX_REDUCE_FORCE", "2")
    rsa.reload_env()
    v = rl.small_ints(N20, ol.F64, 9230)
    check(keys12, ol.U32, v, ol.F64, route=rsa.REDUCE_SORT, what="FORCE=2 on a cells input", tag="keys12")
    h = ol.splitmix_fill((1 << 17) + 9, ol.U16, 9231)
    got, _ = check(h, ol.U16, v[:h.size], ol.F64, order=ol.DESC, route=rsa.REDUCE_SORT, what="u16 keys")
    assert got[0].size > 50000
    b = ol.splitmix_fill(70001, ol.U8, 9232)
    check(b, ol.I8, v[:b.size], ol.F64, route=rsa.REDUCE_SORT, what="i8 keys")


# ---- values ---------------------------------------------------------------------------------------------------------------------

ROUTE_ENVS = [("default", {}), ("global", {"RSX_REDUCE_LDS_BITS": "0", "RSX_REDUCE_MAX_BITS": "16"}), ("sort", {"RSX_REDUCE_FORCE": "2"})]


@pytest.fixture(params=ROUTE_ENVS, ids=[r[0] for r in ROUTE_ENVS])
def each_route(request, monkeypatch):
    for k, val in request.param[1].items():
        monkeypatch.setenv(k, val)
    rsa.reload_env()
    return {"default": rsa.REDUCE_CELLS_LDS, "global": rsa.REDUCE_CELLS_GLOBAL, "sort": rsa.REDUCE_SORT}[request.param[0]]


def test_sums_are_64_bits_wide(each_route):
    n = 40003
    k = ol.splitmix_fill(n, ol.U32, 9300, 0x3F0)
    # u32 values of all ones: a group of c of them sums to c * (2^32 - 1), far beyond 32 bits
    got, want = check(k, ol.U32, np.full(n, 0xFFFFFFFF, dtype=np.uint32), ol.U32, route=each_route, what="u32 all ones")
    assert np.array_equal(got[2], got[1] * np.uint64(0xFFFFFFFF))
    # negative i32 values: sign extension
    neg = (-(np.arange(n, dtype=np.int64) % 1000) - 1).astype(np.int32).view(np.uint32)
    got, _ = check(k, ol.U32, neg, ol.I32, route=each_route, what="negative i32")
    assert np.all(got[2].view(np.int64) < 0)
    # u64 values whose sum wraps past 2^64
    big = ol.splitmix_fill(n, ol.U64, 9301) | np.uint64(1 << 63)
    check(k, ol.U32, big, ol.U64, route=each_route, what="u64 wrap-around")
    # i64 minimum and maximum at the ends of the range
    wide = ol.splitmix_fill(n, ol.U64, 9302)
    wide[:2] = (np.uint64(1 << 63), np.uint64((1 << 63) - 1))
    got, _ = check(k, ol.U32, wide, ol.I64, route=each_route, what="i64 min / max")
    assert int(got[3].view(np.int64).min()) == -(1 << 63) and int(got[4].view(np.int64).max()) == (1 << 63) - 1


@pytest.mark.parametrize("vdt", rl.FLOATS)
def test_special_floats_by_bit_pattern(each_route, vdt):
    """+-0.0, +-inf and NaNs of both signs among the values: min and max bit for bit by the float KDF's total order (a NaN does not
    poison them); the sums of such groups are whatever IEEE makes of them and are not compared."""
    w = np.float32 if vdt == ol.F32 else np.float64
    nb = ol.DTYPE_SIZE[vdt] * 8
    qnan = 0x7FC00000 if vdt == ol.F32 else 0x7FF8000000000000
    special = np.r_[np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -2.5, 3e-40, -3e-40], dtype=w).view(ol.NP_BITS[vdt]),
                    np.array([qnan, qnan | (1 << (nb - 1)), qnan | 5, (qnan | 5) | (1 << (nb - 1))], dtype=ol.NP_BITS[vdt])]
    n = 30011
    rng = np.random.default_rng(9310)
    v = special[rng.integers(0, special.size, n)]
    k = ol.splitmix_fill(n, ol.U32, 9311, 0x7F00)
    k[rng.random(n) < 0.3] = k[0]
    got, want = check(k, ol.U32, v, vdt, route=each_route, what="special floats", sums=False, ops=rl.MIN | rl.MAX)
    top = 1 << (nb - 1)
    assert any(int(x) == ((qnan | 5) | top) for x in got[3]) and any(int(x) == (qnan | 5) for x in got[4])
    # groups of zeros alone: -0.0 is the minimum, +0.0 the maximum
    z = np.where(rng.random(n) < 0.5, 0, top).astype(ol.NP_BITS[vdt])
    got, _ = check(k, ol.U32, z, vdt, route=each_route, what="zeros of both signs", sums=False, ops=rl.MIN | rl.MAX)
    assert int(got[3][0]) == top and int(got[4][0]) == 0


@pytest.mark.parametrize("vdt", rl.FLOATS)
def test_float_sums_of_integers_are_exact(each_route, vdt):
    """Integers |v| < 2^24 stored as floats: every partial sum is below 2^45 and exact in f64, so any order gives the same bits."""
    n = (1 << 19) + 3
    k = skewed(n, ol.U32, 0x0F0F, 9320, share=0.5)
    v = rl.small_ints(n, vdt, 9321)
    check(k, ol.U32, v, vdt, route=each_route, what="exact float sums", ops=rl.SUM)


def test_general_float_sums_are_within_the_bound(each_route):
    """Finite normal doubles of mixed sign and magnitude: per group of c values |got - fsum| <= ((c - 1) u / (1 - (c - 1) u)) *
    sum|v_i| + u |fsum|, u = 2^-53 -- the first term the standard bound of recursive summation in any order, the second fsum's
    own rounding."""
    n = 200003
    rng = np.random.default_rng(9330)
    x = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))
    v = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    k = skewed(n, ol.U32, 0x3F3, 9331, share=0.3)
    grp = rl.groups(k, ol.U32)
    want = rl.want_reduce(grp, v, ol.F64)
    got = run(k, ol.U32, v, ol.F64, ops=rl.SUM)
    assert got[5].route == each_route
    compare(got[:2], want[:2], "general floats")
    g, w = got[2].view(np.float64), want[2].view(np.float64)
    bound = rl.fsum_bound(grp, v, ol.F64) + 2.0 ** -53 * np.abs(w)
    err = np.abs(g - w)
    print("general float sums: largest error / bound = %.3g" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    # f32 values: converted exactly, added as doubles
    v32 = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    want = rl.want_reduce(grp, v32, ol.F32)
    got = run(k, ol.U32, v32, ol.F32, ops=rl.SUM)
    bound = rl.fsum_bound(grp, v32, ol.F32) + 2.0 ** -53 * np.abs(want[2].view(np.float64))
    assert np.all(np.abs(got[2].view(np.float64) - want[2].view(np.float64)) <= bound)


def test_sort_route_float_sums_repeat(monkeypatch):
    monkeypatch.setenv("RSX_REDUCE_FORCE", "2")
    rsa.reload_env()
    n = 100003
    rng = np.random.default_rng(9340)
    v = np.ascontiguousarray(rng.standard_normal(n) * 1e6, dtype=np.float64).view(np.uint64)
    k = ol.splitmix_fill(n, ol.U32, 9341, 0xFF)
    a, b = run(k, ol.U32, v, ol.F64, ops=rl.SUM), run(k, ol.U32, v, ol.F64, ops=rl.SUM)
    assert a[5].route == rsa.REDUCE_SORT and np.array_equal(a[2], b[2])


# ---- outputs ----------------------------------------------------------------------------------------------------------------------

def test_every_subset_of_the_outputs(each_route):
    n = 20011
    k = ol.splitmix_fill(n, ol.U32, 9400, 0x7F0)
    v = rl.small_ints(n, ol.F32, 9401)
    want = rl.want_reduce(rl.groups(k, ol.U32), v, ol.F32)
    for keys, counts, s, mn, mx in itertools.product((False, True), repeat=5):
        ops = (rl.SUM if s else 0) | (rl.MIN if mn else 0) | (rl.MAX if mx else 0)
        got = run(k, ol.U32, v, ol.F32, ops=ops, keys=keys, counts=counts)
        tag = "outputs keys=%d counts=%d ops=%d" % (keys, counts, ops)
        assert got[5].route == each_route, tag
        assert [x is not None for x in got[:5]] == [keys, counts, s, mn, mx], tag
        compare(got[:5], want, tag)


def test_outputs_given_as_tensors_and_index_width():
    n = 5003
    k = ol.splitmix_fill(n, ol.U32, 9410, 0x1F)
    v = rl.small_ints(n, ol.I64, 9411)
    want = rl.want_reduce(rl.groups(k, ol.U32), v, ol.I64)
    kd, vd = dev(k, ol.U32), dev(v, ol.I64)
    for ib in (4, 8):
        cn = torch.full((n,), -1, dtype=_IT[ib], device="cuda")
        sm = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        ok, c2, s2, mn, mx, info = rsa.radix_sort_reduce(kd, vd, dtype=ol.U32, val_dtype=ol.I64, idx_dtype=_IT[ib], counts=cn, sum=sm, keys_out=False)
        torch.cuda.synchronize()
        g = want[0].size
        assert ok is None and mn is None and mx is None and c2.data_ptr() == cn.data_ptr() and s2.data_ptr() == sm.data_ptr()
        assert c2.numel() == g and np.array_equal(c2.cpu().numpy().astype(np.uint64), want[1])
        assert np.array_equal(s2.cpu().numpy().view(np.uint64), want[2])
    with pytest.raises(rsa.RsxError, match="room"):
        rsa.radix_sort_reduce(kd, vd, dtype=ol.U32, val_dtype=ol.I64, sum=torch.zeros(n - 1, dtype=torch.int64, device="cuda"))


def test_host_form():
    n = 30007
    for dt, mask, vdt, route in ((ol.U32, 0xFF0, ol.F32, rsa.REDUCE_CELLS_LDS), (ol.U64, (1 << 40) - 1, ol.I32, rsa.REDUCE_SORT),
                                 (ol.U8, 0xFF, ol.U64, rsa.REDUCE_CELLS_LDS)):
        k = ol.splitmix_fill(n, dt, 9420, mask)
        v = rl.small_ints(n, vdt, 9421)
        want = rl.want_reduce(rl.groups(k, dt, ol.DESC), v, vdt)
        kc, vc = k.copy(), v.copy()
        ok, cn, sm, mn, mx, info = rsa.radix_sort_reduce_host(kc, vc, dt, vdt, order=ol.DESC, idx_dtype=np.uint64, min=True, max=True, counts=True)
        assert info.route == route and np.array_equal(kc, k) and np.array_equal(vc, v)
        compare((ok, cn, sm.view(np.uint64), mn, mx), want, "host form dt=%d" % dt)
