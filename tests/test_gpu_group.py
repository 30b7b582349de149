"""rsx_sort_group_device on the GPU: the inverse, the groups' keys, counts and first indices against the oracle
(tests/group_lib.py), every route asserted where a case was written for it (so that none passes by falling back), the chunk and
tile boundaries of the rank cells and of the heads pass, RSX_GROUP_MAX_BITS=0 against the bitmap results, every subset of the
outputs left out, and the host form."""
import itertools

import numpy as np
import pytest

import group_lib as gr
import oracle_lib as ol
import radix_sorting_amd as rsa
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_IT = {4: torch.int32, 8: torch.int64}
ROUTE = {0: "TRIVIAL", 1: "RANK_LDS", 2: "RANK_GLOBAL", 3: "TABLE", 4: "SORT"}
TILE = 8192     # unique_heads_tile<u32>(): 4 sweeps of 512 threads x one 16-byte vector


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


def run(bits, dt, order=ol.ASC, ib=4, inverse=True, keys=True, counts=False, first=False):
    """radix_sort_group on a device copy of `bits`: (inverse, keys, counts, first, info), the arrays back on the host (the
    index arrays as uint64, the keys as bit patterns), None where one was not asked for.  The keys on the device are compared
    with the copy afterwards: src is never written."""
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    src = dev(a, dt)
    out = rsa.radix_sort_group(src, dtype=dt, order=order, idx_dtype=_IT[ib], keys=keys, counts=counts, first=first, inverse=inverse)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(ol.NP_BITS[dt]), a), "src was written"
    idx = lambda t: None if t is None else t.cpu().numpy().view(np.uint32 if ib == 4 else np.uint64).astype(np.uint64)
    inv, k, cn, fi, info = out
    return idx(inv), (None if k is None else k.cpu().numpy().view(ol.NP_BITS[dt])), idx(cn), idx(fi), info


def compare(got, want, tag):
    for name, g, w in zip(("inverse", "keys", "counts", "first"), got, want):
        if g is None:
            continue
        assert g.size == w.size, "%s: %s has %d entries, oracle %d" % (tag, name, g.size, w.size)
        assert np.array_equal(g, w), "%s: %s differs from the oracle" % (tag, name)


def check(bits, dt, order=ol.ASC, route=None, ib=4, what="", with_counts=False):
    """The call the route was written for (inverse + keys; + counts where `with_counts`; everything on the sort route), its
    route asserted, then all four outputs in one call -- each array of both calls against the oracle."""
    want = gr.want_group(bits, dt, order)
    everything = route == rsa.GROUP_SORT
    got = run(bits, dt, order, ib, counts=with_counts or everything, first=everything)
    tag = "%s dt=%d order=%d n=%d ib=%d route=%s" % (what, dt, order, np.asarray(bits).size, ib, ROUTE.get(got[4].route))
    if route is not None:
        assert got[4].route == route, tag + ": expected route " + ROUTE[route]
    compare(got[:4], want, tag)
    info = got[4]
    if not everything:
        allof = run(bits, dt, order, ib, counts=True, first=True)
        assert allof[4].route in (rsa.GROUP_SORT, rsa.GROUP_TRIVIAL), tag + ": first indices come from the sort route"
        compare(allof[:4], want, tag + " (all four)")
    assert info.sort.key_bytes == ol.DTYPE_SIZE[dt]
    return got, want


# ---- rank cells over the bitmap, read from LDS ---------------------------------------------------------------------------------

N20 = (1 << 20) + 3
RANK_LDS_CASES = [("u32-3runs-v16", ol.U32, 0x00F0FF0F, 16), ("u64-v18", ol.U64, 0x3FFFF, 18), ("u16-full", ol.U16, 0xFFFF, 16)]


@pytest.mark.parametrize("case", RANK_LDS_CASES, ids=[c[0] for c in RANK_LDS_CASES])
def test_rank_lds(case):
    name, dt, mask, vbits = case
    a = ol.splitmix_fill(N20, dt, 8301, mask)
    got, _ = check(a, dt, route=rsa.GROUP_RANK_LDS, what=name)
    words = max(1024, (1 << vbits) // 32)
    assert got[4].varying_bits == vbits and got[4].table_bytes == words * 12, (got[4].varying_bits, got[4].table_bytes)
    check(a, dt, order=ol.DESC, route=rsa.GROUP_RANK_LDS, what=name + " desc")
    check(a[:77], dt, order=ol.DESC, route=rsa.GROUP_RANK_LDS, what=name + " 77 keys")
    check(a[:77], dt, route=rsa.GROUP_RANK_LDS, ib=8, what=name + " 77 keys, 8-byte indices")


def test_rank_cells_at_word_and_chunk_boundaries():
    """Packed values on bits 0 and 31 of a word, and in words 1023 and 1024 -- the last cell of one chunk of the bitmap and the
    first of the next: a wrong chunk base or an off-by-one in the mask below the bit shows in the inverse."""
    special = np.array([0, 31, 32, 63, 1023 * 32, 1023 * 32 + 31, 1024 * 32, 1024 * 32 + 31, 2047 * 32 + 31, 0x5555, 0xAAAA], dtype=np.uint16)
    rng = np.random.default_rng(8302)
    a = special[rng.integers(0, special.size, 5003)]
    a[:special.size] = special[::-1]
    for order in (ol.ASC, ol.DESC):
        got, want = check(a, ol.U16, order, rsa.GROUP_RANK_LDS, what="word and chunk boundaries")
        assert got[1].size == special.size and got[4].varying_bits == 16
    # the same values spread over three runs of a 4-byte key (the packing on the way in, its inverse for the keys)
    b = ul.deposit(a.astype(np.uint64), 0x00F0FF0F).astype(np.uint32) | np.uint32(0x13000000)
    check(b, ol.U32, ol.ASC, rsa.GROUP_RANK_LDS, what="word and chunk boundaries, three runs")


# ---- ... read from device memory --------------------------------------------------------------------------------------------

def test_rank_global():
    a = ol.splitmix_fill((1 << 21) + 5, ol.U32, 8303, 0x00FFFFFF)
    got, _ = check(a, ol.U32, route=rsa.GROUP_RANK_GLOBAL, what="u32 v24")
    assert got[4].varying_bits == 24 and got[4].table_bytes == (1 << 19) * 12
    b = ol.splitmix_fill((1 << 21) + 1, ol.U64, 8304, 0x3FFFFF00000)
    check(b, ol.I64, ol.DESC, rsa.GROUP_RANK_GLOBAL, what="i64 v22 desc")
    check(b, ol.I64, ol.ASC, rsa.GROUP_RANK_GLOBAL, ib=8, what="i64 v22, 8-byte indices")


def test_first_global_size():
    """V = 18 is the last size whose cells fit LDS, V = 19 the first that reads them from device memory."""
    for vbits, route in ((18, rsa.GROUP_RANK_LDS), (19, rsa.GROUP_RANK_GLOBAL)):
        a = ol.splitmix_fill(N20, ol.U32, 8305 + vbits, (1 << vbits) - 1)
        a[:2] = (0, (1 << vbits) - 1)
        got, _ = check(a, ol.U32, route=route, what="v%d" % vbits)
        assert got[4].varying_bits == vbits


# ---- one kept column ------------------------------------------------------------------------------------------------------------

def test_table(monkeypatch):
    a = ol.splitmix_fill(N20, ol.U32, 8306, 0x00FF0000)
    b = ol.splitmix_fill(N20 + 4, ol.U8, 8307)
    b[b == 7] = 9                 # (an empty bin inside the column)
    for bits, dt, order in ((a, ol.U32, ol.ASC), (b, ol.U8, ol.ASC), (b, ol.I8, ol.DESC), (b[:100], ol.I8, ol.ASC)):
        got, _ = check(bits, dt, order, rsa.GROUP_TABLE, with_counts=True, what="one column + counts")
        assert got[4].table_bytes == 2048 + 64
        check(bits, dt, order, rsa.GROUP_TABLE, ib=8, what="one column")
        # first indices are not the table's to give
        allof = run(bits, dt, order, counts=True, first=True)
        assert allof[4].route == rsa.GROUP_SORT
    monkeypatch.setenv("RSX_GROUP_MAX_BITS", "0")
    check(a, ol.U32, route=rsa.GROUP_SORT, what="one column, MAX_BITS=0")
    got = run(b, ol.U8, counts=True)
    assert got[4].route == rsa.GROUP_SORT and got[4].table_bytes == 0


def test_trivial():
    a = np.full(70001, 0x01020304, dtype=np.uint32)
    for ib in (4, 8):
        got = run(a, ol.U32, ib=ib, counts=True, first=True)
        assert got[4].route == rsa.GROUP_TRIVIAL
        compare(got[:4], gr.want_group(a, ol.U32), "all equal")
    got = run(a[:2], ol.U32, counts=True, first=True)
    compare(got[:4], gr.want_group(a[:2], ol.U32), "two equal keys")


# ---- the sort route ---------------------------------------------------------------------------------------------------------------

def test_sort_route():
    a = ol.splitmix_fill(300001, ol.F32, 8308, 0xFFF000FF)      # mixed signs
    check(a, ol.F32, route=rsa.GROUP_SORT, what="f32 mixed signs")
    check(a, ol.F32, ol.DESC, rsa.GROUP_SORT, ib=8, what="f32 mixed signs desc, 8-byte indices")
    check(a[:1000], ol.F32, route=rsa.GROUP_SORT, what="1000 keys")
    z = np.array([0x80000000, 0, 0x7FC00000, 0x7FC00001, 0, 0x80000000, 0x3F800000, 0x7FC00000], dtype=np.uint32)
    got, _ = check(z, ol.F32, route=rsa.GROUP_SORT, what="both zeros, two NaN payloads")
    assert got[1].size == 5
    rng = np.random.default_rng(8309)
    d = rng.permutation(50021).astype(np.uint32) * np.uint32(0x9E3779B1)     # (odd multiplier: a bijection -- all distinct)
    got, _ = check(d, ol.U32, route=rsa.GROUP_SORT, what="all distinct")
    assert got[1].size == d.size and np.all(got[2] == 1)
    e = ol.splitmix_fill(N20, ol.U32, 8310, 0x000FFFFF)          # V = 20: a bitmap input, but counts are wanted
    got = run(e, ol.U32, counts=True)
    assert got[4].route == rsa.GROUP_SORT and got[4].varying_bits == 20
    compare(got[:4], gr.want_group(e, ol.U32), "v20 + counts")


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("shape", ["straddle", "head"])
def test_sort_route_tile_boundaries(n, shape):
    """The sorted order has one group across the boundary of the heads pass's tiles (elements TILE - 2 .. TILE + 1), or a head
    exactly on a tile's first element with a group that ends on the element before."""
    s = np.arange(n, dtype=np.uint64) * 3 + 5
    if shape == "straddle":
        s[TILE - 2:TILE + 2] = s[min(TILE - 2, n - 1)]
    else:
        s[TILE - 3:TILE] = s[min(TILE - 3, n - 1)]
    if n > 2 * TILE:
        s[2 * TILE - 1:] = s[2 * TILE - 1]        # the last tile holds one element, of the group before
    keys = s.astype(np.uint32) << np.uint32(9)      # (order-preserving: `keys` is the sorted order the heads pass sees)
    if n > TILE:
        assert (keys[TILE] != keys[TILE - 1]) == (shape == "head") and keys[TILE - 1] == keys[TILE - 2]
    a = keys[np.random.default_rng(8311 + n).permutation(n)]
    check(a, ol.U32, route=rsa.GROUP_SORT, what="%s at the tile boundary" % shape)


def test_sorted_input_makes_no_sort():
    a = np.sort(ol.splitmix_fill(N20 + 6, ol.U32, 8312, 0x0FFFFFFF) >> np.uint32(3))
    got, _ = check(a, ol.U32, route=rsa.GROUP_SORT, what="sorted with duplicates")
    assert got[4].sort.early_exit == 2 and got[1].size < a.size
    assert np.all(np.diff(got[0].astype(np.int64)) >= 0)


@pytest.mark.parametrize("case", RANK_LDS_CASES + [("u32-v24", ol.U32, 0x00FFFFFF, 24)], ids=lambda c: c[0])
def test_forced_sort_gives_the_bitmap_results(case, monkeypatch):
    name, dt, mask, vbits = case
    a = ol.splitmix_fill(N20, dt, 8313, mask)
    inv, keys, _, _, info = run(a, dt)
    assert info.route in (rsa.GROUP_RANK_LDS, rsa.GROUP_RANK_GLOBAL)
    monkeypatch.setenv("RSX_GROUP_MAX_BITS", "0")
    got = run(a, dt)
    assert got[4].route == rsa.GROUP_SORT and got[4].table_bytes == 0
    compare(got[:4], gr.want_group(a, dt), name + " MAX_BITS=0")
    assert np.array_equal(got[0], inv) and np.array_equal(got[1], keys)
    monkeypatch.setenv("RSX_GROUP_MAX_BITS", str(vbits - 1))
    assert run(a, dt)[4].route == rsa.GROUP_SORT
    monkeypatch.setenv("RSX_GROUP_MAX_BITS", str(vbits))
    assert run(a, dt)[4].route == info.route


def test_pair_sort_route_under_the_heads_pass():
    """Uniform u32 at a size where the key + payload sort goes without a histogram: the group call reports the route that
    rsx_sort_pairs_device reports for the same keys and an iota payload on its own."""
    n = (1 << 22) + (1 << 20) + 3
    a = ol.splitmix_fill(n, ol.U32, 8314)
    k0 = dev(a, ol.U32)
    v0 = torch.arange(n, dtype=torch.int32, device="cuda")
    _, _, pinfo = rsa.radix_sort_pairs(k0, torch.empty_like(k0), v0, torch.empty_like(v0), dtype=rsa.U32)
    torch.cuda.synchronize()
    got = run(a, ol.U32, counts=True, first=True)
    assert got[4].route == rsa.GROUP_SORT
    assert got[4].sort.hybrid == pinfo.hybrid, (got[4].sort.hybrid, pinfo.hybrid)
    compare(got[:4], gr.want_group(a, ol.U32), "uniform u32, n = %d" % n)


# ---- outputs left out, the sibling feature, the host form ---------------------------------------------------------------------

SUBSET_INPUTS = [("rank", ol.U32, 0x00F0FF0F, 200003), ("sort", ol.U32, 0xFFFFFFFF, 100003)]


@pytest.mark.parametrize("case", SUBSET_INPUTS, ids=[c[0] for c in SUBSET_INPUTS])
def test_every_subset_of_the_outputs(case):
    name, dt, mask, n = case
    a = ol.splitmix_fill(n, dt, 8315, mask)
    a[1::2] = a[0:-1:2][:a[1::2].size]          # (every key at least twice: counts and first indices say something)
    want = gr.want_group(a, dt)
    for sel in itertools.product((False, True), repeat=4):
        got = run(a, dt, inverse=sel[0], keys=sel[1], counts=sel[2], first=sel[3])
        tag = "%s input, outputs %s, route %s" % (name, sel, ROUTE.get(got[4].route))
        assert [g is not None for g in got[:4]] == list(sel), tag
        compare(got[:4], want, tag)
        if name == "sort" or sel[3] or sel[2]:
            assert got[4].route == rsa.GROUP_SORT, tag
        else:
            assert got[4].route == rsa.GROUP_RANK_LDS, tag
    # n_groups alone
    src = dev(a, dt)
    _, k, _, _, _ = rsa.radix_sort_group(src, dtype=dt, keys=True, inverse=False)
    assert k.numel() == want[1].size


@pytest.mark.parametrize("dt,mask,order", [(ol.U32, 0x00F0FF0F, ol.ASC), (ol.F32, 0xFFF000FF, ol.DESC), (ol.U16, 0xFFFF, ol.DESC),
                                           (ol.I8, 0xFF, ol.ASC), (ol.U64, 0x3FFFFF00000, ol.ASC)])
def test_keys_are_radix_sort_uniques(dt, mask, order):
    a = ol.splitmix_fill(300001, dt, 8316, mask)
    _, keys, _, _, _ = run(a, dt, order)
    src = dev(a, dt)
    out, _, _ = rsa.radix_sort_unique(src, torch.empty_like(src), dtype=dt, order=order)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(ol.NP_BITS[dt]), keys)
    assert np.array_equal(keys, ul.want_unique(a, dt, order)[0])


@pytest.mark.parametrize("name,dt,mask,route", [("rank", ol.U32, 0x00F0FF0F, rsa.GROUP_RANK_LDS), ("sort", ol.F32, 0xFFF000FF, rsa.GROUP_SORT)])
def test_host_form(name, dt, mask, route):
    a = ol.splitmix_fill(200001, dt, 8317, mask)
    want = gr.want_group(a, dt)
    everything = route == rsa.GROUP_SORT
    before = a.copy()
    for idt in (np.uint32, np.uint64):
        inv, keys, counts, first, info = rsa.radix_sort_group_host(a, dt, idx_dtype=idt, keys=True, counts=everything, first=everything)
        assert info.route == route and np.array_equal(a, before)
        got = [None if x is None else x.astype(np.uint64) for x in (inv, None, counts, first)]
        got[1] = keys
        compare(got, want, "host form, " + name)
