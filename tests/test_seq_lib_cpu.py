"""seq_lib without a GPU: the circuit really holds every ordered pair of kinds once, what expect() says agrees with a second,
independent statement in numpy (np.sort / np.unique / np.lexsort on the derived keys), check() accepts the reference's own
answer and rejects every stale one (seq_lib.wrong_*), and the references of a piece of the circuit are cheap enough for a
test that has to stay quick."""
import collections
import time

import numpy as np
import pytest

import lex_lib as ll
import oracle_lib as ol
import seq_lib as sq

# Steps per piece (seq_lib.M).  Measured: the references of the whole circuit (325 steps) take about 12 s of CPU time, half of it
# for the nineteen sorts of 2^22 keys (0.33 s each), which the walk visits every other step for a stretch: pieces of 12 steps reach
# 2.2 s, of 8 steps 1.9 s, of 7 steps 1.5 s.
M = sq.M
WALK = sq.circuit(sq.KINDS)
PIECES = sq.pieces(WALK, M)


def piece_steps(i):
    return sq.piece_steps(WALK, M, i)


# ---- the circuit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 7, len(sq.KINDS)])
def test_circuit_holds_every_ordered_pair_once(k):
    kinds = sq.KINDS[:k]
    walk = sq.circuit(kinds)
    assert len(walk) == k * k + 1 and walk[0] == walk[-1]
    pairs = collections.Counter(zip(walk, walk[1:]))
    assert set(pairs) == {(a, b) for a in kinds for b in kinds}
    assert set(pairs.values()) == {1}
    assert walk == sq.circuit(list(kinds)), "the same arguments give the same walk"


def test_there_are_about_eighteen_kinds():
    assert len(sq.KINDS) == 18 and len(WALK) == 18 * 18 + 1


@pytest.mark.parametrize("m", [2, 5, M, 400])
def test_pieces_overlap_by_one_kind_and_lose_no_pair(m):
    ps = sq.pieces(WALK, m)
    assert all(2 <= len(p) <= m for p in ps)
    for p, q in zip(ps, ps[1:]):
        assert q[0] == p[-1]
    got = collections.Counter(pair for p in ps for pair in zip(p, p[1:]))
    assert got == collections.Counter(zip(WALK, WALK[1:]))
    assert sq.pieces(WALK, m) == ps


def test_steps_rotate_types_orders_and_sizes():
    steps = sq.steps_of(WALK)
    assert steps == sq.steps_of(WALK)
    assert [s.kind for s in steps] == WALK
    for kind, (lo, hi, dts) in sq.SPEC.items():
        mine = [s for s in steps if s.kind == kind]
        assert {s.dt for s in mine} == set(dts), kind
        assert all(lo <= s.n <= hi for s in mine) and {lo, hi} <= {s.n for s in mine}, kind
        if kind != "replay":
            assert {s.order for s in mine} == {0, 1}, kind
    assert {sq.refusal(s) for s in steps if s.kind == "refused"} == {"nth", "topk", "records"}
    assert {s.seed % 2 for s in steps if s.kind == "sub_async"} == {0, 1}
    assert all(s.n <= 300001 for s in steps if s.kind != "keys_nohist")
    assert all(s.style == 0 for s in steps if s.kind == "keys_nohist"), "even keys: the sort without a histogram has to take them"
    for s in steps:
        if s.kind == "lex":
            assert ol.DTYPE_SIZE[s.dt] != ol.DTYPE_SIZE[sq.lex_second_dtype(s.dt)]


# ---- expect() against a second statement ---------------------------------------------------------------------------------------
def second(step):
    """What the step must deliver, said again in numpy on the derived keys (ol.kdf_keys): equal derived keys are equal bit
    patterns, so the sorted derived keys fix the sorted array, and (derived key, position) fixes the stable permutation."""
    inp = sq.inputs(step)
    a, dt, order, n = inp["keys"], step.dt, step.order, step.n
    k = ol.kdf_keys(a, dt, order)
    perm = np.lexsort((np.arange(n), k))
    u, first, inverse, counts = np.unique(k, return_index=True, return_inverse=True, return_counts=True)
    kind = step.kind
    kdf = lambda x: ol.kdf_keys(x, dt, order)
    w = {}
    if kind in sq.KEY_SORTS or kind in ("keys_async", "replay"):
        w["kdf(out)"] = np.sort(k)
        if kind in sq.KEY_SORTS:
            sorted_already = bool(np.all(k[1:] >= k[:-1]))
            kb = ol.DTYPE_SIZE[dt]
            cols = [j for j in range(kb) if np.unique((k >> ol.NP_BITS[dt](8 * j)) & ol.NP_BITS[dt](0xFF)).size > 1]
            w["early_exit"] = 2 if sorted_already else 0
            if not sorted_already:
                w["cols"] = cols
                w["result_in_aux"] = len(cols) & 1
    elif kind == "pairs" or (kind == "sub_async" and step.seed % 2):
        w["keys"], w["vals"] = a[perm], inp["vals"][perm]
    elif kind == "rank" or kind == "sub_async":
        w["ranks"] = perm.astype(np.uint64)
    elif kind == "unique":
        w["kdf(keys)"], w["counts"] = u, counts.astype(np.uint64)
    elif kind == "group":
        w["kdf(keys)"], w["counts"] = u, counts.astype(np.uint64)
        w["inverse"], w["first"] = inverse.reshape(-1).astype(np.uint64), first.astype(np.uint64)
    elif kind == "rankdata":
        place = np.empty(n, dtype=np.uint64)
        place[perm] = np.arange(n, dtype=np.uint64)
        below = np.cumsum(counts) - counts
        w["place"], w["less"], w["equal"] = place, below[inverse.reshape(-1)].astype(np.uint64), counts[inverse.reshape(-1)].astype(np.uint64)
    elif kind == "topk":
        kk = inp["k"]
        w["keys"], w["idx"] = a[perm[:kk]], perm[:kk].astype(np.uint64)
        w["n_less"], w["n_equal"] = int((k < k[perm[kk - 1]]).sum()), int((k == k[perm[kk - 1]]).sum())
        w["kth_key"] = int(a[perm[kk - 1]])
    elif kind == "nth":
        r = inp["ranks"].astype(np.int64)
        w["keys"], w["idx"] = a[perm[r]], perm[r].astype(np.uint64)
        w["n_less"] = np.array([(k < k[perm[x]]).sum() for x in r], dtype=np.uint64)
        w["n_equal"] = np.array([(k == k[perm[x]]).sum() for x in r], dtype=np.uint64)
    elif kind == "lex":
        dts = [dt, sq.lex_second_dtype(dt)]
        w["perm"] = ll.lexsort_perm([a, inp["col1"]], dts, [order, order ^ 1]).astype(np.uint64)
    elif kind == "records":
        w["out"] = inp["records"][perm].reshape(-1)
    elif kind == "refused":
        w["rc"] = sq.EINVAL
    return w, kdf


EDGE_STEPS = [sq.make_step(kind, j) for kind in sq.KINDS for j in (0, 1, 12, 13)]   # smallest n, largest n, another type, the other order


@pytest.mark.parametrize("step", EDGE_STEPS, ids=sq.describe)
def test_expect_agrees_with_numpy_on_the_derived_keys(step):
    lo, hi, _ = sq.SPEC[step.kind]
    assert lo <= step.n <= hi
    want = sq.expect(step)
    again, kdf = second(step)
    assert again
    for name, val in again.items():
        if name.startswith("kdf("):
            got = kdf(want[name[4:-1]])
        else:
            got = want[name]
        assert sq._same(got, val), (sq.describe(step), name)
    if step.kind == "presorted":
        assert want["early_exit"] == 2 and want["result_in_aux"] == 0 and np.all(want["aux"].view(np.uint8) == sq.FILL)
        assert np.array_equal(want["out"], sq.inputs(step)["keys"])


def test_the_smallest_and_largest_n_of_every_kind_are_among_the_edge_steps():
    for kind, (lo, hi, _) in sq.SPEC.items():
        assert {lo, hi} <= {s.n for s in EDGE_STEPS if s.kind == kind}


# ---- check() accepts the right answer and rejects the stale ones ------------------------------------------------------------------
SMALL = {kind: sq.make_step(kind, 3, n=min(max(sq.SPEC[kind][0], 3000), sq.SPEC[kind][1])) for kind in sq.KINDS
         if kind != "keys_nohist"}
SMALL["keys_nohist"] = sq.make_step("keys_nohist", 0)
# the steps "before": a longer unsorted result of other keys, and a pre-sorted one (other flags)
BEFORE = [sq.make_step("keys_mid", 5, n=9000), sq.make_step("presorted", 6, n=9000), sq.make_step("pairs", 7, n=9000),
          sq.make_step("rankdata", 8, n=9000)]
APPLIES = {
    "wrong_stale_previous": set(sq.KINDS),
    "wrong_stale_histogram": set(sq.KEY_SORTS) | {"pairs", "keys_async", "sub_async", "replay"},
    "wrong_stale_flag": set(sq.FLAGGED),
    "wrong_stale_tail": set(sq.KINDS) - {"refused"},
}


_WANTS = {}


def want_of(step):
    if step not in _WANTS:
        _WANTS[step] = sq.expect(step)
    return _WANTS[step]


@pytest.mark.parametrize("kind", sq.KINDS)
def test_check_accepts_the_reference_and_rejects_every_stale_answer(kind):
    step = SMALL[kind]
    want = want_of(step)
    sq.check(step, sq.clean_answer(step, want), want)
    for gen in sq.WRONG:
        made = 0
        for prev in BEFORE:
            got = gen(step, want, prev, want_of(prev))
            if got is None:
                continue
            made += 1
            got = sq.clean_answer(step, got) if gen is not sq.wrong_stale_tail else got
            bad = sq.mismatches(step, got, want)
            assert bad, (kind, gen.__name__, sq.describe(prev), "a stale answer passed")
            with pytest.raises(AssertionError, match="wrong after"):
                sq.check(step, got, want, before=prev)
        rank_async = step.kind == "sub_async" and step.seed % 2 == 0
        if kind in APPLIES[gen.__name__] and not (rank_async and gen is sq.wrong_stale_histogram):
            assert made, (kind, gen.__name__, "no stale answer could be made")


def test_check_names_the_step_before():
    step, prev = SMALL["keys_mid"], BEFORE[1]
    got = sq.wrong_stale_flag(step, want_of(step), prev, want_of(prev))
    with pytest.raises(AssertionError) as e:
        sq.check(step, sq.clean_answer(step, got), want_of(step), before=prev)
    assert sq.describe(prev) in str(e.value) and "early_exit" in str(e.value)


def test_a_missing_field_and_dirty_tails_are_mismatches():
    step = SMALL["topk"]
    want = want_of(step)
    got = sq.clean_answer(step, want)
    del got["n_less"]
    assert sq.mismatches(step, got, want) == ["n_less (missing)"]
    got = sq.clean_answer(step, want)
    got["tails"] = got["tails"].copy()
    got["tails"][-1] ^= 1
    assert sq.mismatches(step, got, want) == ["tails"]


# ---- the back-off rule, restated --------------------------------------------------------------------------------------------------
def test_backoff_routes():
    assert sq.backoff_routes([False] * 4) == [True] * 4
    # lost: skip 1; lost again: skip 3; won: back to attempting every sort
    assert sq.backoff_routes([True, False, True, False, False, False, False, False]) == \
        [True, False, True, False, False, False, True, True]
    # the skips grow 1, 3, 7, 15, 31 and stay at 31
    out = sq.backoff_routes([True] * 200)
    gaps = np.diff(np.flatnonzero(out)) - 1
    assert list(gaps[:6]) == [1, 3, 7, 15, 31, 31] and set(gaps[5:]) == {31}
    # the device's rule for the device-scheduled sorts: 1, 2, 4 .. 64
    gaps = np.diff(np.flatnonzero(sq.backoff_routes([True] * 400, device=True))) - 1
    assert list(gaps[:8]) == [1, 2, 4, 8, 16, 32, 64, 64] and set(gaps[7:]) == {64}


# ---- the references of a piece are cheap ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PIECES)))
def test_references_of_a_piece(i):
    """expect() over the whole circuit, piece by piece.  The CPU time of a piece is printed (python -m pytest -s), not asserted:
    how long a host takes says nothing about the references being right.  M was chosen from these figures (see above)."""
    steps = piece_steps(i)
    assert [s.kind for s in steps] == PIECES[i]
    t0 = time.process_time()
    for s in steps:
        want = sq.expect(s)
        assert want["tails"] == "clean" and want["rc"] in (0, sq.EINVAL)
    print("piece %d: %d steps, %.2f s of CPU time for the references" % (i, len(steps), time.process_time() - t0))
