"""tests/decide_lib.py against the reference restatement (oracle/): every input tests/test_gpu_decisions.py sorts does what that
module assumes of it -- no GPU, no library.

For every (dtype, order, size, position) of the pre-sorted family: the derived keys descend exactly once, at p; the O(n)
expected result (the sorted base with one element moved) is the oracle's, at every position of the arrays up to 65536 keys and
at eight positions of each larger one; the oracle takes the early exit (early_exit == 2) on every base and does not take it
(early_exit == 0) on the perturbed arrays it is given; decide_lib.one_descent refuses NONE of the cases (asserted, with the
number of cases printed).  For the arrays beyond 65536 keys the count of descents at every position is exact but local (the
base, checked whole, has none: only a patched element's neighbours can descend), and the oracle itself and the count over the
whole array run at the eight spot positions.  For the kept-columns family: the oracle's kept columns are
the base's plus the stray key's column, result_in_aux follows, and the O(n) expected result is the oracle's.
"""
import numpy as np
import pytest

import decide_lib as dl
import oracle_lib as ol

_counts = {"descent_cases": 0, "refused": 0, "oracle_sorts": 0, "stray_cases": 0}


def _oracle(bits, dt, order):
    _counts["oracle_sorts"] += 1
    want, in_aux, info = ol.oracle_sort(bits, dt, order)
    return want, in_aux, info


def _check_spec(spec):
    s = dl.spec_base(spec)
    dt, order, n = spec.dtype, spec.order, spec.n
    assert dl.descents(s, dt, order).size == 0
    want, in_aux, info = _oracle(s, dt, order)
    assert info.early_exit == 2 and in_aux == 0 and info.ncols == 0 and np.array_equal(want, s), dl.spec_id(spec)
    if n >= 1000:                                   # duplicates, and no constant halves
        assert np.unique(s).size < n and s[0] != s[n // 2 - 1] and s[n // 2] != s[n - 1]
    keys = ol.kdf_keys(s, dt, order).copy()
    per_offset = [dl.spec_positions(spec, off) for off in spec.offsets]
    _counts["descent_cases"] += sum(len(ps) for ps in per_offset)
    ps = sorted(set().union(*per_offset))          # (the offsets of a base share most positions: each is checked once)
    spots = set(ps) if n <= dl.SMALL else set(dl.spot_positions(ps))
    for p in ps:
        try:
            case = dl.descent_case(s, dt, order, p)
        except dl.NoDescent:
            _counts["refused"] += 1
            continue
        # exactly one descent, at p.  The base has none (checked above over the whole array), so only the neighbours of a
        # patched element can descend: those are looked at here at every position, the whole array again at the spot positions
        saved = [(i, keys[i]) for i, _ in case.patches]
        for i, v in case.patches:
            keys[i] = ol.kdf_keys(np.array([v], dtype=s.dtype), dt, order)[0]
        lo, hi = max(min(i for i, _ in case.patches) - 1, 0), min(max(i for i, _ in case.patches) + 2, n)
        where = lo + np.flatnonzero(keys[lo:hi - 1] > keys[lo + 1:hi])
        for i, v in saved:
            keys[i] = v
        assert where.tolist() == [p], (dl.spec_id(spec), p, where[:4])
        if p in spots:
            a, expect = dl.one_descent(s, dt, order, p)
            assert dl.descents(a, dt, order).tolist() == [p]
            want, in_aux, info = _oracle(a, dt, order)
            assert info.early_exit == 0, (dl.spec_id(spec), p)
            assert np.array_equal(expect, want), (dl.spec_id(spec), p)
            assert list(info.cols[:info.ncols]) == dl.kept_columns(a, dt, order) and in_aux == (info.ncols & 1)
    assert np.array_equal(keys, ol.kdf_keys(s, dt, order))


@pytest.mark.parametrize("family", dl.PRESORTED_FAMILIES)
def test_every_descent_case_is_one_descent_and_its_expectation_the_oracles(family):
    for spec in dl.presorted_specs(family):
        _check_spec(spec)


def test_no_case_is_refused():
    """Walks every spec's positions again (cheap: descent_case is O(1)) so that the count does not depend on the test order."""
    cases = refused = 0
    for family in dl.PRESORTED_FAMILIES:
        for spec in dl.presorted_specs(family):
            s = dl.spec_base(spec)
            for off in spec.offsets:
                for p in dl.spec_positions(spec, off):
                    cases += 1
                    try:
                        dl.descent_case(s, spec.dtype, spec.order, p)
                    except dl.NoDescent:
                        refused += 1
    print("decide_lib: %d descent cases generated, %d refused" % (cases, refused))
    assert cases > 0 and refused == 0


def test_positions_names_every_boundary():
    for kb in (1, 2, 4, 8):
        vec = 16 // kb
        n = (1 << 21) + 12345
        for off in (0, 1, 3):
            head = dl.head_elems_of(off, kb)
            ps = dl.positions(n, kb, head, sampled=True)
            assert ps == sorted(set(ps)) and ps[0] >= 0 and ps[-1] == n - 2
            for r in (0, 1, vec - 2, vec - 1, vec, 64 * vec - 1, 64 * vec, 1024 * vec - 1, 1024 * vec, 2048 * vec - 1, 2048 * vec):
                assert head + r in ps and max(r, 0) in ps, (kb, off, r)
            m = 1
            while m * 2048 * vec < n:
                assert head + m * 2048 * vec - 1 in ps
                m *= 2
            assert m > 1
            if head:
                assert head - 1 in ps
            full = (n - head) // vec
            assert min(head + full * vec - 1, n - 2) in ps and head + full * vec - 2 in ps and n - 3 in ps
            step = (n - 128) // 63
            assert all(x in ps for x in (6, 7, 8, 127, 128, step - 1, step, step + 7, step + 8))
            assert len(dl.positions(n, kb, head, rand=0)) < len(dl.positions(n, kb, head)) <= len(dl.positions(n, kb, head, rand=0)) + 16
    # small arrays: everything out of range collapses onto the ends, nothing is lost in between
    assert dl.positions(2, 4) == [0] and dl.positions(3, 1) == [0, 1]
    assert dl.head_elems_of(1, 1) == 15 and dl.head_elems_of(3, 4) == 1 and dl.head_elems_of(3, 8) == 1 and dl.head_elems_of(0, 2) == 0


def test_one_descent_refuses_what_cannot_descend():
    flat = np.full(10, 7, dtype=np.uint32)
    with pytest.raises(dl.NoDescent):
        dl.one_descent(flat, ol.U32, ol.ASC, 3)
    half = np.array([1, 1, 1, 1, 1, 9, 9, 9, 9, 9], dtype=np.uint32)
    with pytest.raises(dl.NoDescent):      # raising an element whose right neighbour is the maximum already
        dl.one_descent(np.array([1, 1, 9, 9, 9, 9, 9, 9, 9, 9], dtype=np.uint32), ol.U32, ol.ASC, 3)
    with pytest.raises(dl.NoDescent):      # lowering the right neighbour of an element that is the minimum already
        dl.one_descent(np.array([1, 1, 1, 1, 1, 1, 1, 1, 9, 9], dtype=np.uint32), ol.U32, ol.ASC, 6)
    a, want = dl.one_descent(half, ol.U32, ol.ASC, 2)
    assert a.tolist() == [1, 1, 9, 1, 1, 9, 9, 9, 9, 9] and want.tolist() == sorted(a.tolist())


@pytest.mark.parametrize("dt", range(10), ids=ol.DTYPE_NAMES)
def test_kdf_inverse_round_trips(dt):
    a = ol.splitmix_fill(4099, dt, 77 + dt)
    if dt in dl._FLOAT_EDGES:
        a[:8] = np.array(dl._FLOAT_EDGES[dt], dtype=a.dtype)
    for order in (ol.ASC, ol.DESC):
        assert np.array_equal(dl.kdf_inverse(ol.kdf_keys(a, dt, order), dt, order), a)
        want, _, _ = ol.oracle_sort(a, dt, order)
        assert np.array_equal(dl.sort_by_kdf(a, dt, order), want)


def test_rank_pieces_are_the_oracles_ranks():
    """The O(n) ranks of a descent case (ties: the moved element in front of the equal maxima, behind the equal minima) against
    oracle_rank: every position of the arrays up to 70001 keys, four of each larger one."""
    for family in ("A-rank-pairs", "F", "E-rank-pairs"):
        for spec in dl.presorted_specs(family):
            s = dl.spec_base(spec)
            dt, order, n = spec.dtype, spec.order, spec.n
            ranks, half, info, _ = ol.oracle_rank(s, dt, 4, order)
            assert info.early_exit == 2 and np.array_equal(ranks, np.arange(n, dtype=np.uint32))
            ps = dl.spec_positions(spec)
            ps = ps if n <= 70001 else dl.spot_positions(ps, 4)
            iota = np.arange(n, dtype=np.uint32)
            for p in ps:
                case = dl.descent_case(s, dt, order, p)
                want, whalf, winfo, _ = ol.oracle_rank(dl.apply_patches(s, case), dt, 4, order)
                pieces = dl.rank_pieces(s, dt, order, case)
                got = dl.assemble(iota, dl.Case(p, case.kind, case.patches, pieces))
                assert winfo.early_exit == 0 and np.array_equal(got, want), (dl.spec_id(spec), p)
                assert whalf == (winfo.ncols & 1)
    # the tie rule is exercised: a base whose maximum and minimum occur more than once
    s = np.array([1, 1, 2, 3, 4, 5, 6, 7, 9, 9], dtype=np.uint32)
    for p in range(9):
        try:
            case = dl.descent_case(s, ol.U32, ol.ASC, p)
        except dl.NoDescent:
            continue
        want = ol.oracle_rank(dl.apply_patches(s, case), ol.U32, 4)[0]
        got = dl.assemble(np.arange(10, dtype=np.uint32), dl.Case(p, case.kind, case.patches, dl.rank_pieces(s, ol.U32, ol.ASC, case)))
        assert np.array_equal(got, want), p


def _check_stray(spec, base, positions, flips, what):
    """flips: (column, bit) pairs."""
    dt, order, n = spec.dtype, spec.order, spec.n
    base_kept = dl.kept_columns(base, dt, order)
    want, in_aux, info = _oracle(base, dt, order)
    assert list(info.cols[:info.ncols]) == (base_kept if info.early_exit == 0 else []), what
    sb = dl.sort_by_kdf(base, dt, order)
    assert np.array_equal(sb, want) or info.early_exit
    sk = ol.kdf_keys(sb, dt, order)
    cases = [(c, b, p) for c, b in flips for p in positions]
    spots = set(range(len(cases))) if n <= dl.SMALL else set(dl.spot_positions(list(range(len(cases))), 8))
    for j, (column, bit, p) in enumerate(cases):
        _counts["stray_cases"] += 1
        assert column not in base_kept, what
        case = dl.stray_case(base, sb, dt, order, column, p, bit, sorted_keys=sk)
        (i, v), = case.patches
        assert i == p and v == dl.one_stray(base, dt, column, p, bit)[p]
        x = int(ol.kdf_keys(np.array([v], dtype=base.dtype), dt, order)[0]) ^ int(ol.kdf_keys(base[p:p + 1], dt, order)[0])
        assert x == 1 << (8 * column + bit), (what, column, bit, p)
        if j not in spots:
            continue
        a = dl.apply_patches(base, case)
        want, in_aux, info = _oracle(a, dt, order)
        kept, want_aux, early = dl.stray_decision(base, base_kept, dt, order, column, case)
        assert info.early_exit == early and in_aux == want_aux and list(info.cols[:info.ncols]) == kept, (what, column, bit, p)
        if base_kept:
            assert kept == sorted(base_kept + [column]) and early == 0
        assert np.array_equal(dl.assemble(sb, case), want), (what, column, bit, p)


@pytest.mark.parametrize("size_class", ["A", "B", "C"])
def test_stray_cases_keep_the_bases_columns_plus_one(size_class):
    for spec in dl.stray_specs(size_class):
        base = dl.stray_base(spec)
        assert dl.kept_columns(base, spec.dtype, spec.order) == [c for c in range(ol.DTYPE_SIZE[spec.dtype]) if c not in spec.constant]
        ps = dl.stray_positions(spec.n, ol.DTYPE_SIZE[spec.dtype], spec.sampled)
        _check_stray(spec, base, ps, [(c, b) for c in spec.constant for b in dl.STRAY_BITS], dl.stray_id(spec))


def test_stray_cases_above_the_log_routes_window():
    for n in dl.N_D:
        base = dl.stray_base_d(n)
        assert int(base.max()) < 1 << 40 and dl.kept_columns(base, ol.U64, ol.ASC) == [0, 1, 2, 3, 4]
        spec = dl.StraySpec(ol.U64, ol.ASC, n, (5, 6, 7), True)
        _check_stray(spec, base, dl.stray_positions(n, 8, True), [(b // 8, b % 8) for b in dl.STRAY_BITS_D], "D n=%d" % n)


def test_counts_are_reported():
    print("decide_lib: %(descent_cases)d descent cases checked (%(refused)d refused), %(stray_cases)d stray cases, "
          "%(oracle_sorts)d oracle sorts" % _counts)
    assert _counts["refused"] == 0
