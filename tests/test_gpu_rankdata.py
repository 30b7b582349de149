"""rsx_sort_rankdata_device on the GPU: place, less and equal against the oracle side (tests/rankdata_lib.py), every route asserted
where a case was written for it (so that none passes by falling back), the share, tile and seam boundaries of each route's
kernels, every non-empty subset of the outputs, RSX_RANKDATA_NO_TABLES=1 against the table results, and rankdata()."""
import itertools

import numpy as np
import pytest

import group_lib as gr
import oracle_lib as ol
import radix_sorting_amd as rsa
import rankdata_lib as rl
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_IT = {4: torch.int32, 8: torch.int64}
_KT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
ROUTE = {0: "TRIVIAL", 1: "TABLE", 2: "COUNT16", 3: "SORT"}
PLACE_TILE = 2048        # RANKDATA_PLACE_TILE: 8 rounds of 256 threads x one key
PLACE_MAX_WGS = 1024     # RANKDATA_PLACE_MAX_WGS: a share is n / 1024 keys rounded up to whole tiles
HEADS_TILE = {4: 8192, 8: 4096}   # unique_heads_tile<KT>(): 4 sweeps of 512 threads x one 16-byte vector
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(bits, dt, skew=0):
    """A device copy of `bits`, `skew` elements past an allocation's (256-byte aligned) start."""
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    t = torch.zeros(a.size + skew, dtype=_KT[ol.DTYPE_SIZE[dt]], device="cuda")
    t[skew:] = torch.from_numpy(a.view(ul.SIGNED[ol.DTYPE_SIZE[dt]]).copy()).cuda()
    return t[skew:]


def run(bits, dt, order=ol.ASC, ib=4, what=(True, True, True), skew=0):
    """radix_sort_rankdata on a device copy of `bits`: (place, less, equal, info), the arrays back on the host as uint64, None
    where one was not asked for.  The keys on the device are compared with the copy afterwards: src is never written."""
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    src = dev(a, dt, skew)
    assert src.data_ptr() % 16 == (skew * ol.DTYPE_SIZE[dt]) % 16
    out = rsa.radix_sort_rankdata(src, dtype=dt, order=order, idx_dtype=_IT[ib], place=what[0], less=what[1], equal=what[2])
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(ol.NP_BITS[dt]), a), "src was written"
    idx = lambda t: None if t is None else t.cpu().numpy().view(np.uint32 if ib == 4 else np.uint64).astype(np.uint64)
    return idx(out[0]), idx(out[1]), idx(out[2]), out[3]


def check(bits, dt, order=ol.ASC, route=None, ib=4, what=(True, True, True), tag="", skew=0, want=None):
    want = rl.want_rankdata(bits, dt, order) if want is None else want
    got = run(bits, dt, order, ib, what, skew)
    info = got[3]
    tag = "%s dt=%d order=%d n=%d ib=%d what=%s route=%s" % (tag, dt, order, np.asarray(bits).size, ib, what, ROUTE.get(info.route))
    if route is not None:
        assert info.route == route, tag + ": expected route " + ROUTE[route]
    for name, asked, g, w in zip(("place", "less", "equal"), what, got[:3], want):
        assert (g is not None) == bool(asked), tag
        if g is not None:
            assert g.size == w.size and np.array_equal(g, w), "%s: %s differs from the oracle" % (tag, name)
    assert info.sort.key_bytes == ol.DTYPE_SIZE[dt]
    return info, want


# ---- one kept column: lookups in its offsets, the place in three launches ---------------------------------------------------------

def _u8_all_digits(n, seed):
    a = ol.splitmix_fill(n, ol.U8, seed)
    a[:256] = np.arange(256, dtype=np.uint8)[::-1]
    return a


def _u8_skewed(n, seed):
    """digit 7 absent, digit 200 nine keys in ten: long stretches of one digit inside a round"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n).astype(np.uint8)
    a[a == 7] = 9
    a[rng.random(n) < 0.9] = 200
    a[:3] = (0, 255, 201)
    return a


def _f32_top_byte(n, seed):
    """negative floats that differ in their sign / exponent byte alone.  (Of one sign: the KDF complements a negative float
    and flips only the sign of a positive one, so with both signs the constant low bytes become two values each and all four
    columns are kept.)"""
    return (ol.splitmix_fill(n, ol.U32, seed, 0x7F000000) | np.uint32(0x80400000)).astype(np.uint32)


TABLE_SIZES = [3 * PLACE_TILE + 5, PLACE_TILE - 1, PLACE_TILE, PLACE_TILE + 1]
TABLE_KEYS = [
    ("u8-all-digits", ol.U8, ol.ASC, _u8_all_digits),
    ("u8-skewed", ol.U8, ol.ASC, _u8_skewed),
    ("u32-one-byte", ol.U32, ol.ASC, lambda n, seed: ol.splitmix_fill(n, ol.U32, seed, 0x00FF0000) | np.uint32(0x13000042)),
    ("i8-desc", ol.I8, ol.DESC, lambda n, seed: ol.splitmix_fill(n, ol.U8, seed)),
    ("f32-top-byte", ol.F32, ol.ASC, _f32_top_byte),
]


@pytest.mark.parametrize("case", TABLE_KEYS, ids=[c[0] for c in TABLE_KEYS])
def test_table(case):
    name, dt, order, make = case
    for n in TABLE_SIZES:
        a = make(n, 8701 + n)
        info, want = check(a, dt, order, rsa.RANKDATA_TABLE, tag=name)
        assert info.varying_bits <= 8 and info.table_bytes == 256 * 8 * (1 + (n + PLACE_TILE - 1) // PLACE_TILE)
        check(a, dt, order, rsa.RANKDATA_TABLE, what=(False, True, True), tag=name + " less+equal", want=want)
    a = make(TABLE_SIZES[0], 8702)
    info, want = check(a, dt, order, rsa.RANKDATA_TABLE, ib=8, tag=name + " 8-byte indices")
    check(a, dt, order, rsa.RANKDATA_TABLE, skew=1, tag=name + " src one element off", want=want)
    check(a, dt, order, rsa.RANKDATA_TABLE, ib=8, skew=1, what=(False, True, True), tag=name + " one element off, less+equal", want=want)


def test_table_shares_of_several_tiles():
    """2^22 + 3 keys: 4097 keys per workgroup round up to shares of three tiles, 683 workgroups, the last share short."""
    n = (1 << 22) + 3
    share = ((n + PLACE_MAX_WGS - 1) // PLACE_MAX_WGS + PLACE_TILE - 1) // PLACE_TILE * PLACE_TILE
    assert share == 3 * PLACE_TILE
    info, _ = check(_u8_skewed(n, 8703), ol.U8, ol.ASC, rsa.RANKDATA_TABLE, tag="u8 skewed, 2^22 + 3")
    assert info.table_bytes == 256 * 8 * (1 + (n + share - 1) // share)
    check(ol.splitmix_fill(n, ol.U32, 8704, 0x0000FF00), ol.U32, ol.DESC, rsa.RANKDATA_TABLE, tag="u32 one byte desc, 2^22 + 3")


# ---- at most 16 varying bits, no place: the count table ---------------------------------------------------------------------------

N20 = (1 << 20) + 3
NO_PLACE = (False, True, True)
COUNT16_CASES = [("u32-3runs-v16", ol.U32, 0x00F0FF0F), ("u16-full", ol.U16, 0xFFFF), ("u64-v16-at-20", ol.U64, 0xFFFF << 20)]
SEAM = np.array([0, 0x7FFF, 0x8000, 0xFFFF], dtype=np.uint64)   # the last bin of one kind of workgroup, the first of the other


def _count16_keys(n, dt, mask, seed):
    a = ol.splitmix_fill(n, dt, seed, mask)
    a[5:5 + SEAM.size] = ul.deposit(SEAM, mask).astype(a.dtype)
    return a


@pytest.mark.parametrize("case", COUNT16_CASES, ids=[c[0] for c in COUNT16_CASES])
def test_count16(case):
    name, dt, mask = case
    a = _count16_keys(N20, dt, mask, 8711)
    info, _ = check(a, dt, ol.ASC, rsa.RANKDATA_COUNT16, what=NO_PLACE, tag=name)
    assert info.varying_bits == 16 and info.table_bytes == 65536 * 4 + 65537 * 8
    check(a[:77], dt, ol.ASC, rsa.RANKDATA_COUNT16, what=NO_PLACE, tag=name + " 77 keys")
    check(a[:77], dt, ol.DESC, rsa.RANKDATA_COUNT16, what=NO_PLACE, ib=8, tag=name + " 77 keys desc, 8-byte indices")
    check(a[:50001], dt, ol.DESC, rsa.RANKDATA_COUNT16, what=(False, True, False), skew=1, tag=name + " desc, one element off")
    # with the place wanted, two kept columns and more have no table
    check(a[:5003], dt, ol.ASC, rsa.RANKDATA_SORT, tag=name + " with the place")


def test_count16_one_key_and_the_rest():
    a = np.zeros(N20, dtype=np.uint16)
    a[70001] = 0xFFFF
    info, want = check(a, ol.U16, ol.ASC, rsa.RANKDATA_COUNT16, what=NO_PLACE, tag="one key and the rest")
    assert want[2][70001] == 1 and want[1][70001] == N20 - 1 and want[2][0] == N20 - 1
    check(a, ol.I16, ol.DESC, rsa.RANKDATA_COUNT16, what=NO_PLACE, tag="one key and the rest, i16 desc")


def test_count16_ends_at_sixteen_bits():
    a = ol.splitmix_fill(N20, ol.U32, 8712, 0x1FFFF)
    a[:2] = (0, 0x1FFFF)
    info, _ = check(a, ol.U32, ol.ASC, rsa.RANKDATA_SORT, what=NO_PLACE, tag="v17")
    assert info.varying_bits == 17 and info.table_bytes == 0
    b = ol.splitmix_fill(N20, ol.U32, 8713, 0xFFFF)
    b[:2] = (0, 0xFFFF)
    info, _ = check(b, ol.U32, ol.ASC, rsa.RANKDATA_COUNT16, what=NO_PLACE, tag="v16")
    assert info.varying_bits == 16


# ---- everything else: the sort, then the inverse scatter or the heads and the runs pass ----------------------------------------------

@pytest.mark.parametrize("dt", [ol.U32, ol.U64])
def test_sort_uniform_at_the_tiles_of_the_heads_pass(dt):
    tile = HEADS_TILE[ol.DTYPE_SIZE[dt]]
    for n in (tile - 1, tile, tile + 1, 3 * tile + 1):
        a = ol.splitmix_fill(n, dt, 8721 + n)
        a[1::2] = a[0::2][:a[1::2].size]          # every key twice, nearly: runs of two all over the tiles
        a = a[np.random.default_rng(n).permutation(n)]
        info, want = check(a, dt, ol.ASC, rsa.RANKDATA_SORT, tag="uniform")
        assert info.table_bytes == 0
        check(a, dt, ol.DESC, rsa.RANKDATA_SORT, ib=8, tag="uniform desc, 8-byte indices")
        check(a, dt, ol.ASC, rsa.RANKDATA_SORT, what=(True, False, False), tag="uniform, place alone", want=want)


def _with_run(n, at, length, seed):
    """u32 keys whose sorted order has distinct keys in [0, at), one key `length` times from `at` on, distinct keys behind"""
    s = np.arange(n, dtype=np.uint32) * np.uint32(641) + np.uint32(0x10000)
    s[at:at + length] = s[at]
    assert np.all(s[1:] >= s[:-1]) and s[at + length] > s[at]
    return s[np.random.default_rng(seed).permutation(n)]


def test_sort_runs_at_tile_boundaries():
    tile = HEADS_TILE[4]
    # a run that starts on a tile's last element and ends in the next tile
    a = _with_run(3 * tile + 100, tile - 1, 40, 8731)
    _, want = check(a, ol.U32, ol.ASC, rsa.RANKDATA_SORT, tag="run from a tile's last element")
    assert np.count_nonzero(want[2] == 40) == 40 and want[1][want[2] == 40][0] == tile - 1
    # a run that spans three whole tiles and parts of their neighbours
    b = _with_run(5 * tile + 77, tile - 3, 3 * tile + 9, 8732)
    check(b, ol.U32, ol.ASC, rsa.RANKDATA_SORT, tag="run over three tiles")
    check(b, ol.U32, ol.DESC, rsa.RANKDATA_SORT, what=NO_PLACE, tag="run over three tiles desc")
    # the last run ends at n, the end of a tile it shares with distinct keys: no head follows it
    s = np.arange(2 * tile, dtype=np.uint32) * np.uint32(641) + np.uint32(0x10000)
    s[-5:] = s[-5]
    c = s[np.random.default_rng(8733).permutation(s.size)]
    _, want = check(c, ol.U32, ol.ASC, rsa.RANKDATA_SORT, tag="last run")
    assert np.count_nonzero(want[2] == 5) == 5 and want[1].max() == s.size - 5


def test_sort_all_distinct_multiple_of_64():
    n = 2 * HEADS_TILE[4]
    a = (np.random.default_rng(8734).permutation(n).astype(np.uint32) * np.uint32(2654435761))
    assert np.unique(a).size == n and n % 64 == 0
    _, want = check(a, ol.U32, ol.ASC, rsa.RANKDATA_SORT, tag="all distinct")
    assert np.all(want[2] == 1) and np.array_equal(want[0], want[1])
    check(a, ol.U32, ol.ASC, rsa.RANKDATA_SORT, ib=8, what=NO_PLACE, tag="all distinct, 8-byte indices")


def test_sort_two_distinct_keys():
    a = np.where(np.random.default_rng(8735).random(3 * HEADS_TILE[4] + 5) < 0.3, 0x00010001, 0x00020002).astype(np.uint32)
    info, _ = check(a, ol.U32, ol.ASC, rsa.RANKDATA_SORT, tag="two keys")
    assert info.varying_bits == 4
    check(a, ol.U32, ol.DESC, rsa.RANKDATA_SORT, tag="two keys desc")


def test_sort_presorted_input():
    a = np.sort(ol.splitmix_fill(100003, ol.U32, 8736, 0x000FFFFF))
    assert np.unique(a).size < a.size
    for what in ((True, True, True), (True, False, False), NO_PLACE):
        info, want = check(a, ol.U32, ol.ASC, rsa.RANKDATA_SORT, what=what, tag="sorted input")
        assert info.sort.early_exit == 2
    assert np.array_equal(want[0], np.arange(a.size, dtype=np.uint64))


def test_sort_f64_zeros_and_nans():
    a = ol.splitmix_fill(20011, ol.F64, 8737, 0xC00F000000000003)
    special = np.array([0, 1 << 63, 0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000000,
                        0xFFF0000000000000], dtype=np.uint64)
    a[100:100 + 3 * special.size] = np.tile(special, 3)
    for order in (ol.ASC, ol.DESC):
        check(a, ol.F64, order, rsa.RANKDATA_SORT, ib=8, tag="f64")


# ---- every subset of the outputs on every route ---------------------------------------------------------------------------------------

SUBSET_INPUTS = [
    ("table", ol.U32, lambda: ol.splitmix_fill(5003, ol.U32, 8741, 0x0000FF00), lambda s: rsa.RANKDATA_TABLE),
    ("count16", ol.U32, lambda: _count16_keys(5003, ol.U32, 0x00F0FF0F, 8742), lambda s: rsa.RANKDATA_SORT if s[0] else rsa.RANKDATA_COUNT16),
    ("sort", ol.U64, lambda: ol.splitmix_fill(5003, ol.U64, 8743, 0xFFFFF), lambda s: rsa.RANKDATA_SORT),
    ("trivial", ol.U16, lambda: np.full(5003, 0x1234, dtype=np.uint16), lambda s: rsa.RANKDATA_TRIVIAL),
]


@pytest.mark.parametrize("case", SUBSET_INPUTS, ids=[c[0] for c in SUBSET_INPUTS])
def test_every_subset_of_the_outputs(case):
    name, dt, make, route_of = case
    a = make()
    want = rl.want_rankdata(a, dt)
    for what in SUBSETS:
        for ib in (4, 8):
            check(a, dt, ol.ASC, route_of(what), ib=ib, what=what, tag=name, want=want)


def test_no_tables_switch(monkeypatch):
    t = ol.splitmix_fill(70001, ol.U8, 8751)
    c = _count16_keys(70001, ol.U32, 0x00F0FF0F, 8752)
    with_tables = [run(t, ol.U8), run(c, ol.U32, what=NO_PLACE)]
    assert [g[3].route for g in with_tables] == [rsa.RANKDATA_TABLE, rsa.RANKDATA_COUNT16]
    monkeypatch.setenv("RSX_RANKDATA_NO_TABLES", "1")
    rsa.reload_env()
    forced = [check(t, ol.U8, route=rsa.RANKDATA_SORT, tag="NO_TABLES u8")[0], check(c, ol.U32, route=rsa.RANKDATA_SORT, what=NO_PLACE, tag="NO_TABLES v16")[0]]
    assert all(i.table_bytes == 0 for i in forced)
    again = [run(t, ol.U8), run(c, ol.U32, what=NO_PLACE)]
    for g, h in zip(with_tables, again):
        assert h[3].route == rsa.RANKDATA_SORT
        assert all(x is None and y is None or np.array_equal(x, y) for x, y in zip(g[:3], h[:3]))
    monkeypatch.delenv("RSX_RANKDATA_NO_TABLES")
    rsa.reload_env()
    assert run(t, ol.U8)[3].route == rsa.RANKDATA_TABLE


def test_trivial():
    a = np.full(70001, 0x01020304, dtype=np.uint32)
    for ib in (4, 8):
        info, want = check(a, ol.U32, ol.DESC, rsa.RANKDATA_TRIVIAL, ib=ib, tag="all equal")
        assert info.varying_bits == 0
    assert np.array_equal(want[0], np.arange(a.size, dtype=np.uint64)) and not want[1].any() and np.all(want[2] == a.size)
    info, _ = check(a[:1], ol.U32, ol.ASC, rsa.RANKDATA_TRIVIAL, tag="one key")
    assert info.sort.early_exit == 1


# ---- the convenience layer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
def test_rankdata_methods(order):
    a = ol.splitmix_fill(5003, ol.F32, 8761, 0xC0700000)
    a[:2] = (0x00000000, 0x80000000)
    src = dev(a, ol.F32).view(torch.float32)
    place, less, equal = rl.want_rankdata(a, ol.F32, order)
    for method in ("ordinal", "min", "max", "average"):
        got, info = rsa.rankdata(src, method=method, order=order)
        want = rl.by_method(place, less, equal, method)
        assert got.dtype == (torch.float64 if method == "average" else torch.int32)
        assert np.array_equal(got.cpu().numpy().astype(np.float64), np.asarray(want, dtype=np.float64)), method
        assert info.route == rsa.RANKDATA_SORT, method   # (floats of both signs: the KDF makes every low bit vary)
    got, info = rsa.rankdata(src, method="dense", order=order)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), gr.want_group(a, ol.F32, order)[0])
    assert isinstance(info, rsa.GroupInfo)
    assert np.array_equal(src.cpu().numpy().view(np.uint32), a)


def test_rankdata_min_max_take_the_tables():
    a = _count16_keys(50001, ol.U32, 0x00F0FF0F, 8762)
    src = dev(a, ol.U32)
    _, less, equal = rl.want_rankdata(a, ol.U32)
    for method, route in (("min", rsa.RANKDATA_COUNT16), ("max", rsa.RANKDATA_COUNT16), ("average", rsa.RANKDATA_COUNT16), ("ordinal", rsa.RANKDATA_SORT)):
        got, info = rsa.rankdata(src, method=method, dtype=rsa.U32)
        assert info.route == route, method
        if method != "ordinal":
            assert np.array_equal(got.cpu().numpy().astype(np.float64), np.asarray(rl.by_method(None, less, equal, method), dtype=np.float64))


def test_host_form():
    a = ol.splitmix_fill(30001, ol.U16, 8771)
    want = rl.want_rankdata(a, ol.U16, ol.DESC)
    place, less, equal, info = rsa.radix_sort_rankdata_host(a.copy(), rsa.U16, rsa.DESCENDING, idx_dtype=np.uint64, less=True, equal=True)
    assert info.route == rsa.RANKDATA_SORT
    assert np.array_equal(place, want[0]) and np.array_equal(less, want[1]) and np.array_equal(equal, want[2])
    place, less, equal, info = rsa.radix_sort_rankdata_host(a.copy(), rsa.U16, rsa.DESCENDING, place=False, less=True)
    assert info.route == rsa.RANKDATA_COUNT16 and place is None and equal is None and np.array_equal(less, want[1])
