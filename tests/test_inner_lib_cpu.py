"""tests/inner_lib.py on the CPU: every input construction of tests/test_gpu_inner_routes.py has the property it was made for
(tie fractions, the overflowing digit's share, what the two samples see, varying bits, the join's pair count), and every
comparison that file relies on refuses the two wrong results inner_lib models -- two payloads of equal keys exchanged, and a
result made from a first buffer with one level-1 slot's worth of elements overwritten."""
import types

import numpy as np
import pytest

import inner_lib as il
import join_lib as jl
import lex_lib as xl
import locate_lib as ll
import nth_lib as nl
import oracle_lib as ol
import pairs_lib as pl
import partition_lib as ptl
import radix_sorting_amd as rsa
import reduce_lib as rl
import topk_lib as tl

N = 40009          # the comparisons do not depend on the size: small inputs with the same properties
SLOT = il.level1_slot(N)


# ---- the constructions at the sizes the GPU tests use -----------------------------------------------------------------------------
def test_slot_capacity_restated():
    # 1.25 x the mean from means of 1024 on, seven standard deviations below that, multiples of 256
    assert il.slot_cap(16384) == 20480 and il.slot_cap(65536) == 81920 and il.slot_cap(200) == 512 and il.slot_cap(64) == 256
    assert il.level1_slot(il.N22) == 20480 and il.level1_slot(1 << 24) == 81920


@pytest.mark.parametrize("dt", [ol.U32, ol.F32, ol.I32, ol.U64])
def test_wide_keys(dt):
    a = il.wide(il.N22 if dt != ol.U64 else il.N64, dt, 7101)
    kb = ol.DTYPE_SIZE[dt]
    assert il.varying_bits(a, dt) == 8 * kb
    assert il.columns_varying(a, dt, il.unique_sample_index(a.size)) == kb
    assert il.columns_varying(a, dt, il.blind_sample_index(a.size)) == kb and il.sample_sees_descent(a, dt, il.blind_sample_index(a.size))
    assert pl.tied_fraction(a) < 0.01
    assert kb == 8 or (il.slots_fit(a, dt) and il.slots_fit(a, dt, ol.DESC))


def test_wide_ties():
    a = il.wide_ties(il.N22, ol.U32, 7102)
    assert a.size == il.N22 and pl.tied_fraction(a) > 0.3
    assert np.unique(a).size <= il.N22 // 2 + 3
    for dt in (ol.U32, ol.F32, ol.I32):
        for index in (il.unique_sample_index(a.size), il.blind_sample_index(a.size)):
            assert il.columns_varying(a, dt, index) == 4
    pool = il.distinct_wide(1000, ol.U32, 5)
    assert np.unique(pool).size == 1000 and not np.array_equal(pool, np.sort(pool))
    f = il.with_specials(a, ol.F32, 7401)
    sp = il.float_specials(ol.F32)
    assert all(np.count_nonzero(f == s) >= 8 for s in sp) and pl.tied_fraction(f) > 0.3
    assert il.slots_fit(a, ol.U32) and il.slots_fit(a, ol.I32, ol.DESC) and il.slots_fit(f, ol.F32) and il.slots_fit(f, ol.F32, ol.DESC)
    g = il.with_specials(il.wide_ties(il.N22, ol.I32, 7304), ol.F32, 7303)          # (the other float inputs of the GPU tests)
    assert il.slots_fit(il.with_specials(a, ol.F32, 7303), ol.F32, ol.DESC) and il.slots_fit(g, ol.F32)
    assert not il.slots_fit(il.with_specials(a, ol.F32, 7401, every=2053), ol.F32)   # (eight times as many: 0 and 1 overflow their slot)
    assert np.unique(ol.kdf_keys(sp, ol.F32)).size == sp.size         # (twelve different places in the order)


@pytest.mark.parametrize("dt", [ol.U32, ol.F32])
@pytest.mark.parametrize("digit", [0x05, 0xF3])
def test_overflowing(digit, dt):
    a = il.overflowing(il.N22, 7700 + digit, digit, dt)
    share = il.digit_share(a, dt, digit)
    assert share >= 1.4, share
    # more than the level-1 slot holds, and every other digit fits its slot
    k = ol.kdf_keys(a, dt)
    counts = np.bincount((k >> np.uint32(24)).astype(np.int64), minlength=256)
    cap = il.level1_slot(a.size)
    assert counts[digit] > cap and np.count_nonzero(counts > cap) == 1 and not il.slots_fit(a, dt)
    # neither sample sees it coming: all four columns vary, a descent is seen, and the digit is no more frequent than any other
    for index in (il.unique_sample_index(a.size), il.blind_sample_index(a.size)):
        assert il.columns_varying(a, dt, index) == 4
    blind = il.blind_sample_index(a.size)
    assert il.sample_sees_descent(a, dt, blind)
    seen = np.bincount((k[blind] >> np.uint32(24)).astype(np.int64), minlength=256)
    assert seen[digit] <= 2 * seen.mean() + 8


def test_join_sides():
    for m, dt, specials, seed in ((il.JOIN_RIGHT, ol.U32, False, 7201), (il.JOIN_RIGHT, ol.F32, True, 7202), (il.JOIN_RIGHT_BIG, ol.U32, False, 7203)):
        left, right = il.join_sides(il.JOIN_LEFT, m, dt, seed, specials)
        assert left.size == il.JOIN_LEFT and right.size == m
        assert il.varying_bits(right, dt) > 16 and il.varying_bits(left, dt) > 16                      # not the table route
        assert il.JOIN_LEFT >= 1 << 22 and 4 * m >= 1 << 22                                             # the merge route's gate
        order = ol.DESC if specials else ol.ASC
        want = jl.Want(left, right, dt, order)
        assert want.n_pairs(True) <= il.JOIN_MAX_PAIRS and want.n_pairs(False) <= il.JOIN_MAX_PAIRS
        matched = np.count_nonzero(want.count)
        assert 0.45 * left.size < matched < 0.55 * left.size and int(want.count.max()) == 2
        assert np.unique(right).size == m - 5 - (2 if specials else 0)      # (two of the special values stand twice)
        if specials:
            sp = il.float_specials(dt)
            assert np.isin(sp, left).all() and np.isin(sp, right).all()
        assert il.columns_varying(left, dt, il.blind_sample_index(left.size), order) == 4 and il.slots_fit(left, dt, order)


def test_nth_ranks():
    want = il.Ranked(il.wide_ties(N, ol.U32, 3), ol.U32)
    ranks, (lo, hi) = il.nth_ranks(want.kd, 65)
    assert np.unique(ranks).size == 65 and int(ranks.max()) == N - 1 and int(ranks.min()) == 0
    assert want.kd[lo] == want.kd[hi] and hi > lo and {lo, hi} <= set(int(r) for r in ranks)
    assert (lo == 0 or want.kd[lo - 1] != want.kd[lo]) and (hi == N - 1 or want.kd[hi + 1] != want.kd[hi])


def test_ranked_is_the_c_restatement():
    a = il.with_specials(il.wide_ties(N, ol.F32, 4), ol.F32, 5, every=101)
    for order in (ol.ASC, ol.DESC):
        r = il.Ranked(a, ol.F32, order)
        w = nl.Want(a, ol.F32, order)
        assert np.array_equal(r.ranks, w.ranks) and np.array_equal(r.kd, w.kd)
        assert r.first(N // 2)[2:] == tl.Want(a, ol.F32, order).first(N // 2)[2:]


def test_first_k_without_a_full_argsort():
    a = il.wide_ties(N, ol.U32, 6)
    full = tl.Want(a, ol.U32)
    for k in (1, N // 8, N // 8 + 1, N):
        got, want = il.FirstK(a, ol.U32, k).first(k), full.first(k)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), k


# ---- the comparisons refuse the wrong results -------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(AssertionError):
        call()


def _reduce_result(kbits, vbits, perm):
    """What a reduce over the sorted pairs (kbits[perm], vbits[perm]) gives when min and max keep the FIRST of equal values."""
    k, v = kbits[perm], vbits[perm]
    heads = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    counts = np.diff(np.r_[heads, k.size]).astype(np.uint64)
    total = np.add.reduceat(v.astype(np.uint64), heads)
    return k[heads], counts, total


def test_reduce_comparison_refuses():
    a = il.wide_ties(N, ol.U32, 11)
    v = pl.payloads("random", N, 4, 12)
    want = rl.want_reduce(rl.groups(a, ol.U32), v, ol.U32)
    perm = ol.stable_argsort_by_kdf(a, ol.U32)
    good = _reduce_result(a, v, perm) + (want[3], want[4])
    il.compare_reduce("the oracle's own", good, want)
    # a value that travelled with the other of two tied keys stays in its group: a reduce cannot see that, and must not
    swapped = il.wrong_ties_swapped(a, ol.U32, perm)
    il.compare_reduce("ties swapped", _reduce_result(a, v, swapped) + (want[3], want[4]), want)
    # ... but a value beside ANOTHER key, which is what a wrong slice offset gives, shows
    shifted = np.roll(v[perm], 1)
    inv = np.empty(N, dtype=np.int64)
    inv[perm] = np.arange(N)
    _refused(lambda: il.compare_reduce("values one place off", _reduce_result(a, shifted[inv], perm) + (None, None), want))
    for buf, name in ((a, "keys"), (v, "values")):
        bad = il.wrong_slot_overwritten(buf, 3, SLOT)
        kb, vb = (bad, v) if name == "keys" else (a, bad)
        res = rl.want_reduce(rl.groups(kb, ol.U32), vb, ol.U32)
        _refused(lambda: il.compare_reduce("first %s buffer overwritten" % name, res, want))


def _fake_join_info(route):
    return types.SimpleNamespace(route=route, key_bytes=4, left_sorted=1 if route == rsa.JOIN_MERGE else 0, table_bytes=0)


def test_join_comparison_refuses():
    left, right = il.join_sides(N, N // 4, ol.U32, 21)
    right = np.concatenate([right, right[:50]])          # (more ties on the right side)
    left = np.concatenate([left, right])                 # (... and every right key asked for)
    want = jl.Want(left, right, ol.U32)
    info = _fake_join_info(rsa.JOIN_MERGE)
    u = lambda x: np.asarray(x).astype(np.uint32)
    jl.check("the oracle's own", want, u(want.start), u(want.count), u(want.perm), want.n_pairs(), info, False, rsa.JOIN_MERGE)
    # the right side's index sort not stable: right_perm with two rows of equal keys exchanged
    bad_perm = il.wrong_ties_swapped(right, ol.U32, want.perm.astype(np.int64))
    _refused(lambda: jl.check("ties swapped", want, u(want.start), u(want.count), u(bad_perm), want.n_pairs(), info, False, rsa.JOIN_MERGE))
    wl, wr = want.pairs()
    _refused(lambda: il.same("ties swapped", "right_idx", jl.pairs_of(want.start, want.count, bad_perm)[1], wr))
    # the left side's first key buffer overwritten: start / count of those rows are other keys'
    for side in ("left", "right"):
        bad = jl.Want(il.wrong_slot_overwritten(left, 2, SLOT), right, ol.U32) if side == "left" else jl.Want(left, il.wrong_slot_overwritten(right, 2, SLOT), ol.U32)
        _refused(lambda: jl.check(side + " overwritten", want, u(bad.start), u(bad.count), u(bad.perm), bad.n_pairs(), info, False, rsa.JOIN_MERGE))
    # the left side's first INDEX buffer overwritten: start and count scattered back to other rows
    rows = want.left.size
    pos = il.wrong_slot_overwritten(np.arange(rows, dtype=np.uint32), 2, SLOT) % np.uint32(rows)
    _refused(lambda: jl.check("iota overwritten", want, u(want.start[pos]), u(want.count[pos]), u(want.perm), want.n_pairs(), info, False, rsa.JOIN_MERGE))
    # the route asserted
    _refused(lambda: jl.check("route", want, None, None, None, want.n_pairs(), _fake_join_info(rsa.JOIN_SEARCH), False, rsa.JOIN_MERGE))


def test_lex_comparison_refuses():
    cols = [il.wide_ties(N, ol.U32, 31) & np.uint32(0xFF), il.wide_ties(N, ol.U32, 32) & np.uint32(0x3)]     # (rows that tie in both)
    dts, orders = [ol.U32, ol.U32], [ol.ASC, ol.DESC]
    want = xl.lexsort_perm(cols, dts, orders)
    assert np.array_equal(want, xl.want_perm(cols, dts, orders))
    il.same("the oracle's own", "the permutation", want, want)
    # rows that tie in every column, exchanged
    rows = (cols[0].astype(np.uint64) << np.uint64(32)) | (~cols[1]).astype(np.uint64)
    _refused(lambda: il.same("ties swapped", "the permutation", il.wrong_ties_swapped(rows, ol.U64, want), want))
    # the last group's first payload buffer (the permutation of the first group) overwritten
    first = ol.stable_argsort_by_kdf(cols[1], ol.U32, ol.DESC)
    bad_first = (il.wrong_slot_overwritten(first.astype(np.uint32), 1, SLOT) % np.uint32(N)).astype(np.int64)
    bad = bad_first[ol.stable_argsort_by_kdf(cols[0][first], ol.U32)]
    assert np.array_equal(first[ol.stable_argsort_by_kdf(cols[0][first], ol.U32)], want)      # (the model is the sort when nothing is damaged)
    _refused(lambda: il.same("payloads overwritten", "the permutation", bad, want))
    # ... and its first key buffer
    bad_keys = il.wrong_slot_overwritten(cols[0][first], 1, SLOT)
    _refused(lambda: il.same("keys overwritten", "the permutation", first[ol.stable_argsort_by_kdf(bad_keys, ol.U32)], want))


def test_topk_and_nth_comparisons_refuse():
    a = il.wide_ties(N, ol.U32, 41)
    want = il.Ranked(a, ol.U32)
    k = N // 2
    keys, idx, kth, less, equal = want.first(k)
    tinfo = types.SimpleNamespace(route=rsa.TOPK_SORT, key_bytes=4, kth_key=kth, n_less=less, n_equal=equal, input_reads=0, digit_passes=0)
    t = lambda x, w=np.uint32: types.SimpleNamespace(cpu=lambda: types.SimpleNamespace(numpy=lambda: np.ascontiguousarray(x).astype(w)))
    tl.check("the oracle's own", want, k, t(keys), t(idx), tinfo, rsa.TOPK_SORT)
    swapped = il.wrong_ties_swapped(a, ol.U32, want.ranks[:k].astype(np.int64))
    assert np.array_equal(a[swapped], keys)                                   # (the keys alone cannot tell)
    _refused(lambda: tl.check("ties swapped", want, k, t(a[swapped]), t(swapped), tinfo, rsa.TOPK_SORT))
    bad = il.Ranked(il.wrong_slot_overwritten(a, 5, SLOT), ol.U32)
    _refused(lambda: tl.check("keys overwritten", want, k, t(bad.first(k)[0]), t(bad.first(k)[1]), tinfo, rsa.TOPK_SORT))
    _refused(lambda: tl.check("route", want, k, t(keys), t(idx), tinfo, rsa.TOPK_SELECT))
    ranks, (lo, hi) = il.nth_ranks(want.kd, 65)
    wk, wi, wl, we = want.at(ranks)
    ninfo = types.SimpleNamespace(route=rsa.NTH_SORT, key_bytes=4, input_reads=0, digit_passes=0, active_buckets=0, from_prefix=0, candidates=0)
    nl.check("the oracle's own", want, ranks, wk, wi.astype(np.uint32), wl, we, ninfo, rsa.NTH_SORT)
    # the two ends of a run of ties exchanged: the same keys, other indices
    j, jj = int(np.flatnonzero(ranks == lo)[0]), int(np.flatnonzero(ranks == hi)[0])
    si = wi.copy()
    si[[j, jj]] = si[[jj, j]]
    assert wk[j] == wk[jj]
    _refused(lambda: nl.check("ties swapped", want, ranks, wk, si.astype(np.uint32), wl, we, ninfo, rsa.NTH_SORT))
    bk, bi, bl, be = bad.at(ranks)
    _refused(lambda: nl.check("keys overwritten", want, ranks, bk, bi.astype(np.uint32), bl, be, ninfo, rsa.NTH_SORT))


def test_locate_and_partition_comparisons_refuse():
    a = il.wide(N, ol.U32, 51)
    want = ptl.Want(a, ol.U32)
    rng = np.random.default_rng(52)
    vals = np.unique(np.concatenate([a[rng.integers(0, N, 150)], il.wide(150, ol.U32, 53)]))[:300]
    less, equal = want.at(vals)
    bins = want.bins(vals, False)
    linfo = types.SimpleNamespace(route=rsa.LOCATE_SORT, key_bytes=4, input_reads=0, search_steps=0, counter_sets=0)
    u = lambda x: np.asarray(x).astype(np.uint32)
    ll.check("the oracle's own", want, vals, None, None, u(less), u(equal), u(bins), False, linfo, rsa.LOCATE_SORT)
    bad = ll.Want(il.wrong_slot_overwritten(a, 1, SLOT), ol.U32)
    _refused(lambda: ll.check("keys overwritten", want, vals, None, None, u(bad.at(vals)[0]), u(equal), None, False, linfo, rsa.LOCATE_SORT))
    idx, keys, offsets = want.split(vals, False)
    pinfo = types.SimpleNamespace(route=rsa.PARTITION_SORT, key_bytes=4, input_reads=0, search_steps=0, rank_form=0, shares=0,
                                  locate=types.SimpleNamespace(route=rsa.LOCATE_SORT))
    ptl.check("the oracle's own", want, vals, None, None, keys, u(idx), u(offsets), False, pinfo, rsa.PARTITION_SORT)
    # two keys of one part exchanged: the parts hold the same keys, the split is no longer stable
    same_part = il.wrong_ties_swapped(bins, ol.U64, idx.astype(np.int64))
    _refused(lambda: ptl.check("ties swapped", want, vals, None, None, a[same_part], u(same_part), u(offsets), False, pinfo, rsa.PARTITION_SORT))
    bidx, bkeys, boff = ptl.Want(il.wrong_slot_overwritten(a, 1, SLOT), ol.U32).split(vals, False)
    _refused(lambda: ptl.check("keys overwritten", want, vals, None, None, bkeys, u(bidx), u(boff), False, pinfo, rsa.PARTITION_SORT))


def test_wrong_results_are_wrong_where_they_should_be():
    a = il.wide_ties(N, ol.U32, 61)
    perm = ol.stable_argsort_by_kdf(a, ol.U32)
    swapped = il.wrong_ties_swapped(a, ol.U32, perm)
    assert np.count_nonzero(swapped != perm) == 2 and np.array_equal(a[swapped], a[perm])
    bad = il.wrong_slot_overwritten(a, 2, SLOT)
    at = np.flatnonzero(bad != a)
    assert at.size > 0.99 * SLOT and at.min() >= 2 * SLOT and at.max() < 3 * SLOT
    assert il.wrong_slot_overwritten(np.arange(N, dtype=np.uint64), 0, SLOT).dtype == np.uint64
