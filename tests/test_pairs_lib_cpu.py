"""The tests of the key + payload tests (tests/pairs_lib.py), without a GPU.

1. The helper's expectation (stable order of the derived keys, gathered) is what the C restatement of the reference's sort
   gives on {key, payload} records (rso_sort_records; radix_sort.hpp:31-93 moves whole records, so the payload rides along).
2. Every payload family has teeth: three wrong sorts are modelled on the host --
     (a) equal keys ordered by payload value, (b) payloads with their top four bits cleared, (c) the input index written for
     the payload --
   and each family must differ from the wrong models it is there to expose.  The arange(n) * a + b family every key + payload
   test used before equals (a) and (b) bit for bit: the finding tests/test_gpu_payloads.py rests on.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import pairs_lib as pl

ALL = list(range(10))
TIE_INPUTS = {"every key twice": pl.every_key_twice, "runs of four": pl.runs_of_four}


def _record_sort(a, vals, dt, order):
    """(keys, payloads) after rso_sort_records of records that hold the key at offset 0 and the payload behind it."""
    kb, vb = a.itemsize, vals.itemsize
    n = a.size
    recs = np.empty((n, kb + vb), dtype=np.uint8)
    recs[:, :kb] = a.view(np.uint8).reshape(n, kb)
    recs[:, kb:] = vals.view(np.uint8).reshape(n, vb)
    aux = np.full_like(recs, 0xA5)
    info = ol.Info()
    r = ol.oracle().rso_sort_records(ol.ptr(recs), ol.ptr(aux), n, kb + vb, 0, dt, order, C.byref(info))
    assert r in (0, 1)
    out = aux if r else recs
    return (np.ascontiguousarray(out[:, :kb]).view(a.dtype).ravel(), np.ascontiguousarray(out[:, kb:]).view(vals.dtype).ravel(),
            r, info)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("dt", ALL, ids=ol.DTYPE_NAMES)
def test_expectation_is_the_oracles_record_sort(dt, width):
    for n in (2, 1000, 70001):
        a = pl.runs_of_four(n, dt, 100 + dt) if n > 2 else ol.splitmix_fill(n, dt, 100 + dt)
        for order in (ol.ASC, ol.DESC):
            want = pl.Order(a, dt, order)
            for family in pl.FAMILIES:
                vals = pl.payloads(family, n, width, 100 + dt, keys=a)
                keys, got, r, info = _record_sort(a, vals, dt, order)
                assert np.array_equal(keys, want.keys), (n, order, family)
                assert np.array_equal(got, want.vals(vals)), (n, order, family)
                assert r == want.in_aux and list(info.cols[:info.ncols]) == want.cols and info.early_exit == want.early_exit
                pl.compare(want, vals, keys, got, what=(n, order, family))      # (the comparison routine itself, on a right answer)


def test_families_are_what_they_say():
    for width in (4, 8):
        w = 8 * width
        full = (1 << w) - 1
        keys = ol.splitmix_fill(13, ol.U16, 5)
        assert [int(x) for x in pl.payloads("reversed", 13, width)] == list(range(12, -1, -1))
        assert [int(x) for x in pl.payloads("edges", 8, width)] == [0, full, 1 << (w - 1), (1 << (w - 1)) - 1, 1, full - 1, 0, full]
        kb = pl.payloads("keybound", 13, width, keys=keys)
        for k, p in zip(keys, kb):
            x = int(k) ^ (0xA5A5A5A5A5A5A5A5 & full)
            assert int(p) == ((x << 7) | (x >> (w - 7))) & full
        r = pl.payloads("random", 1000, width, 3)
        assert r.dtype.itemsize == width and np.array_equal(r, pl.payloads("random", 1000, width, 3))
        assert not np.array_equal(r, pl.payloads("random", 1000, width, 4))
        assert int(np.bitwise_or.reduce(r)) == full and int(np.bitwise_and.reduce(r)) == 0       # every bit both ways
        assert not np.array_equal(r, ol.splitmix_fill(1000, ol.U32 if width == 4 else ol.U64, 3))   # not the keys' stream
    wide = ol.splitmix_fill(9, ol.U64, 6)
    assert np.array_equal(pl.payloads("keybound", 9, 4, keys=wide), pl.payloads("keybound", 9, 4, keys=wide & np.uint64(0xFFFFFFFF)))


@pytest.mark.parametrize("name", list(TIE_INPUTS))
def test_tie_inputs_tie(name):
    for dt in (ol.U32, ol.F32, ol.U64):
        for n in (1000, 70001):
            a = TIE_INPUTS[name](n, dt, 7)
            assert a.size == n and pl.tied_fraction(a) >= 0.99
            pl.assert_ties(a)
    # what some "duplicates" inputs of the suite are: a mask that leaves 2^28 values for 2^23 keys -- about 3 % of them tie
    weak = ol.splitmix_fill(1 << 23, ol.U32, 9, 0xFFFFFF0F)
    assert pl.tied_fraction(weak) < 0.05
    with pytest.raises(AssertionError):
        pl.assert_ties(weak)


def _differs(x, y):
    return float(np.count_nonzero(x != y)) / x.size


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", list(TIE_INPUTS))
def test_each_family_has_teeth(name, width):
    """Share of the output places at which each family differs from each wrong model (0: the family cannot see that error)."""
    n, dt = 70001, ol.U32
    a = pl.assert_ties(TIE_INPUTS[name](n, dt, 11))
    table = {}
    for order in (ol.ASC, ol.DESC):
        want = pl.Order(a, dt, order)
        for family in pl.FAMILIES + ("increasing",):
            vals = pl.increasing(n, width) if family == "increasing" else pl.payloads(family, n, width, 11, keys=a)
            right = want.vals(vals)
            table[family, order] = (_differs(right, pl.wrong_tie_break_by_value(a, dt, vals, order)),
                                    _differs(right, pl.wrong_top_bits_lost(right)),
                                    _differs(right, pl.wrong_index_for_payload(want).astype(right.dtype)))
    print("\n%s, %d-byte payloads: share of places that differ from (a) ties by value, (b) top bits lost, (c) index for payload" % (name, width))
    for (family, order), row in table.items():
        print("  %-10s %s  (a) %.3f  (b) %.3f  (c) %.3f" % (family, "desc" if order else "asc ", *row))
    for order in (ol.ASC, ol.DESC):
        # reversed: the order inside every run of equal keys flips -- at least half of the places, as at least half of the keys tie
        assert table["reversed", order][0] >= 0.5
        # random: 15 of 16 values have a top nibble; edges: four of its six values do; neither is the index
        assert table["random", order][1] >= 0.9 and table["random", order][2] >= 0.99
        assert table["edges", order][1] >= 0.6 and table["edges", order][2] >= 0.99
        assert table["keybound", order][2] >= 0.99
        # ... and what the suite used: ascending with the position and below 2^28 -- (a) and (b) give the same bytes
        assert table["increasing", order][0] == 0.0 and table["increasing", order][1] == 0.0
    # arange(n) itself (the rank sorts' neighbours in tests/test_gpu_routes.py) cannot see (c) either
    want = pl.Order(a, dt, ol.ASC)
    ident = np.arange(n, dtype=np.uint32 if width == 4 else np.uint64)
    assert np.array_equal(want.vals(ident), pl.wrong_index_for_payload(want).astype(ident.dtype))


def test_compare_rejects_each_wrong_model():
    """The comparison routine fails on every wrong model a family exposes, and names the first place."""
    n, dt = 5000, ol.F32
    a = pl.every_key_twice(n, dt, 13)
    want = pl.Order(a, dt)
    for family, wrong in (("reversed", lambda v: pl.wrong_tie_break_by_value(a, dt, v)),
                          ("random", lambda v: pl.wrong_top_bits_lost(want.vals(v))),
                          ("edges", lambda v: pl.wrong_top_bits_lost(want.vals(v))),
                          ("keybound", lambda v: pl.wrong_index_for_payload(want).astype(np.uint32))):
        vals = pl.payloads(family, n, 4, 13, keys=a)
        pl.compare(want, vals, want.keys, want.vals(vals))
        with pytest.raises(AssertionError, match="payloads differ, first at"):
            pl.compare(want, vals, want.keys, wrong(vals), what=family)
    vals = pl.payloads("random", n, 4, 13)
    with pytest.raises(AssertionError, match="keys differ"):
        pl.compare(want, vals, want.keys[::-1], want.vals(vals))

    class FakeInfo:
        result_in_aux, early_exit, hybrid = want.in_aux, want.early_exit, 0

        def kept_columns(self):
            return want.cols

    pl.compare(want, vals, want.keys, want.vals(vals), info=FakeInfo(), want_route=0, not_route=5)
    with pytest.raises(AssertionError, match="wanted route"):
        pl.compare(want, vals, want.keys, want.vals(vals), info=FakeInfo(), want_route=5)
    with pytest.raises(AssertionError, match="any route but"):
        pl.compare(want, vals, want.keys, want.vals(vals), route=5, not_route=5)
    FakeInfo.result_in_aux = 1 - want.in_aux
    with pytest.raises(AssertionError):
        pl.compare(want, vals, want.keys, want.vals(vals), info=FakeInfo())


def test_large_expectation_agrees_with_the_small_one():
    """4-byte keys beyond pairs_lib.BIG take oracle_lib.want_ranks' sorted compounds: the same permutation as numpy's stable
    argsort of the derived keys, for every 4-byte type and both orders."""
    n = pl.BIG + 77
    for dt in (ol.U32, ol.I32, ol.F32):
        a = pl.every_key_twice(n, dt, 17 + dt)
        for order in (ol.ASC, ol.DESC):
            assert np.array_equal(pl.Order(a, dt, order).perm, ol.stable_argsort_by_kdf(a, dt, order))
