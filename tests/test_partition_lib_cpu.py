"""tests/partition_lib.py against the definition written out, without a GPU: the expected keys / idx / offsets of every GPU test of
rsx_sort_partition* come from partition_lib.Want.split, so it is checked here against the O(n m) definition -- the bin of a key is
the count of the edges at or below (BELOW: below) its derived key, one pair at a time; the output lists the bins in ascending
order and inside a bin the input positions in ascending order; offsets[j] counts the keys whose bin is below j -- on tiny inputs
with ties, repeated edges and both flags: all ten dtypes, both orders, f32 / f64 with NaNs of both signs and +-0.0.  Also the
restated shape (shares, rank_form, natural_route) on cases worked out by hand."""
import numpy as np
import pytest

import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa

SPECIAL = {ol.F32: [0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000],
           ol.F64: [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x0000000000000000, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000, 0xBFF0000000000000]}


def _data(dt, seed, n, m):
    """n keys and m >= 12 edges: a crowd of small keys, half of the edges taken from the keys, floats with the special values"""
    rng = np.random.default_rng(seed)
    t = ol.NP_BITS[dt]
    top = 8 * ol.DTYPE_SIZE[dt]
    draw = lambda k: (rng.integers(0, 1 << 62, size=k, dtype=np.uint64) >> np.uint64(62 - min(top, 62))).astype(t) if top < 62 else \
        (rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)).astype(t)
    keys, edges = draw(n), draw(m)
    keys[: n // 3] &= t(0x3F)
    edges[: m // 2] = keys[rng.integers(0, n, size=m // 2)]
    if dt in SPECIAL:
        sp = np.array(SPECIAL[dt], dtype=t)
        if n >= sp.size:
            keys[-sp.size:] = sp
        edges[-sp.size:] = sp[::-1]
    return keys, edges


def _definition(keys, edges, dt, order, below):
    kk = [int(x) for x in ol.kdf_keys(keys, dt, order)]
    ke = [int(x) for x in ol.kdf_keys(edges, dt, order)]
    bins = [sum(1 for e in ke if (e < k if below else e <= k)) for k in kk]
    idx = [i for p in range(len(ke) + 1) for i in range(len(kk)) if bins[i] == p]
    offsets = [sum(1 for b in bins if b < j) for j in range(len(ke) + 2)]
    return idx, [int(keys[i]) for i in idx], offsets


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt", list(range(10)))
def test_split_against_the_definition(dt, order):
    for seed, n, m in ((1, 120, 40), (2, 37, 60), (3, 1, 12), (4, 64, 1), (5, 50, 0)):
        keys, edges = _data(dt, 100 * dt + seed, n, max(m, 12))
        edges = edges[len(edges) - m:]          # (the tail: the special floats first)
        if m >= 8:
            edges[1] = edges[0]                 # repeated edges: empty parts
            edges[2:5] = edges[5]
        want = pl.Want(keys, dt, order)
        for below in (False, True):
            idx, out, offsets = want.split(edges, below)
            didx, dout, doff = _definition(keys, edges, dt, order, below)
            assert [int(x) for x in idx] == didx, (dt, order, seed, below)
            assert [int(x) for x in out] == dout, (dt, order, seed, below)
            assert [int(x) for x in offsets] == doff and doff[0] == 0 and doff[-1] == n, (dt, order, seed, below)


def test_ties_on_an_edge_go_up_or_down_with_the_flag():
    keys = np.array([5, 1, 5, 9, 5, 0], dtype=np.uint32)
    want = pl.Want(keys, ol.U32)
    idx, out, off = want.split(np.array([5], dtype=np.uint32), False)
    assert list(idx) == [1, 5, 0, 2, 3, 4] and list(out) == [1, 0, 5, 5, 9, 5] and list(off) == [0, 2, 6]
    idx, out, off = want.split(np.array([5], dtype=np.uint32), True)
    assert list(idx) == [0, 1, 2, 4, 5, 3] and list(out) == [5, 1, 5, 5, 0, 9] and list(off) == [0, 5, 6]
    idx, out, off = want.split(np.array([5, 5, 9], dtype=np.uint32), False)      # a repeated edge: part 1 is empty
    assert list(off) == [0, 2, 2, 5, 6] and list(idx) == [1, 5, 0, 2, 4, 3]
    # the equivalent form: offsets[1 .. m] is searchsorted of the sorted edges in the sorted keys, left (BELOW: right)
    rng = np.random.default_rng(5)
    k = rng.integers(0, 50, size=300).astype(np.uint32)
    e = rng.integers(0, 50, size=40).astype(np.uint32)
    w = pl.Want(k, ol.U32)
    assert np.array_equal(w.split(e, False)[2][1:-1], np.searchsorted(np.sort(k), np.sort(e), side="left"))
    assert np.array_equal(w.split(e, True)[2][1:-1], np.searchsorted(np.sort(k), np.sort(e), side="right"))


def test_the_restated_shape_by_hand():
    u = lambda *a: np.array(a, dtype=np.uint32)
    assert pl.TILE == 8192 and pl.SHARE == 16384 and pl.BALLOT_PARTS == rsa.PARTITION_BALLOT_PARTS == 7
    assert pl.distinct_edges(u(5, 5, 7), ol.U32) == 2
    assert pl.natural_route(np.arange(255, dtype=np.uint32), ol.U32) == rsa.PARTITION_SCATTER
    assert pl.natural_route(np.arange(256, dtype=np.uint32), ol.U32) == rsa.PARTITION_SORT
    assert pl.natural_route(np.arange(300, dtype=np.uint32) % 200, ol.U32) == rsa.PARTITION_SCATTER
    assert pl.natural_route(u(1, 2, 3), ol.U32, max_edges=2) == rsa.PARTITION_SORT
    assert pl.rank_form(u(1, 2, 3), ol.U32, seam=4) == 1 and pl.rank_form(u(1, 2, 3, 4), ol.U32, seam=4) == 2
    assert pl.shares(1, 0, 4) == 1 and pl.shares(pl.SHARE + pl.TILE - 1, 0, 4) == 1 and pl.shares(pl.SHARE + pl.TILE, 0, 4) == 2
    assert pl.shares(pl.SHARE + pl.TILE + 2, 4, 4) == 1 and pl.shares(256 * pl.SHARE, 0, 8) == 256 and pl.shares(1 << 30, 0, 4) == 256
