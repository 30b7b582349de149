"""The features on top of the plain sorts (reduce, join, lex, topk, nth, locate, partition, rankdata) at the sizes where the sort
INSIDE them leaves one pass per column, with the feature's route AND the inner sort's route asserted in every case, the result
compared with the existing oracles, and the inputs compared with their host copies afterwards.

The features hand the inner sort slices of their own workspace, cut side by side (reduce: v1 = v0 + npad; join: k1 = k0 + npad in
one allocation with start and count behind it; topk: pk | pk2 | pi | pi2; lex: three index buffers).  The inner routes put level-1
slots into the second buffers, decide from a sample, report result_in_aux by another rule, and after an overflow promise that the
first buffers are untouched -- so a wrong offset, a stale result_in_aux or a first buffer written by a called-off attempt is wrong
for every large input, and only these sizes show it.

  hybrid == 5   the sort without a histogram: 4-byte keys with a 4-byte payload or index from 2^22 pairs on, keys alone from
                7.5 Mi 4-byte / 4.5 Mi 8-byte keys on (tests 1 .. 6)
  called off    inner_lib.overflowing: a level-1 slot overflows after the slots below it were written; the sort goes by another
                route from the first buffers (test 7: hybrid != 5 and launches booked as called off)
  hybrid == 1   one MSB pass and leaves, 300001 pairs (test 8)
  sequences     a large call, a small one, the large one again on one context without emptying the cache (test 9)
  2^23 + 3      where a level-1 slot holds a tile of the pass and 204 of the 256 lie in the feature's SECOND buffers: reduce and join
                without a histogram, reduce called off after those buffers were written (test 10)

Where an info struct carries the inner sort it is asserted directly (.sort.hybrid of reduce, locate, partition, join's right side
and rankdata; group[i].hybrid of lex).  topk and nth expose nothing: their call is bracketed with profile_begin / profile_end and
must book the same hist_launches and leaf_launches as a plain radix_sort_rank of the same keys in the same test, whose info.hybrid
is asserted (only the sort without a histogram books no histogram; only one pass per column books no leaves).  The sort of join's
LEFT side is in no info either: what a MERGE join books beyond the SEARCH join of the same sides must be what a plain key + payload
sort of the left keys books.  Test 5 (top-k by selection, 2^22 + 1 survivors) meets the called-off attempt by itself: the
survivors share their top bits.  n = 2^22 + 3 unless a case says otherwise."""
import os

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
import rankdata_lib as rkl
import reduce_lib as rl
import topk_lib as tl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_SIGNED = {4: np.int32, 8: np.int64}
SWITCHES = ("RSX_JOIN_FORCE", "RSX_RANKDATA_NO_TABLES", "RSX_BLIND_MIN_LOG2", "RSX_LOCATE_FORCE")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()      # (no back-off from an earlier attempt that was called off: the routes are asserted)
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(bits):
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(_SIGNED[a.itemsize]).copy()).cuda()


def bits_of(t, dt):
    return t.cpu().numpy().view(ol.NP_BITS[dt])


def unwritten(tag, t, bits, dt):
    assert np.array_equal(bits_of(t, dt), np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])), (tag, "an input was written")


def junk_like(t, count=None):
    return torch.full((t.numel() if count is None else count,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")


def profiled(call):
    """call() between profile_begin and profile_end: (its result, (hist_launches, leaf_launches), called_off_launches)."""
    rsa.profile_begin()
    try:
        out = call()
        torch.cuda.synchronize()
    finally:
        p = rsa.profile_end()
    return out, (int(p.hist_launches), int(p.leaf_launches)), int(p.called_off_launches)


def plain_rank(src_t, dt, order=ol.ASC):
    """A plain radix_sort_rank of the keys, profiled: (info, launches, called off)."""
    rsa.reload_env()
    ib = junk_like(src_t, 2 * src_t.numel())
    (_, info), launches, off = profiled(lambda: rsa.radix_sort_rank(src_t, ib, dtype=dt, order=order))
    print("plain rank sort: route", info.hybrid, "hist and leaf launches", launches, "called off", off)
    return info, launches, off


def plain_pairs(keys_t, dt, order=ol.ASC):
    """A plain radix_sort_pairs of a copy of the keys with their positions as payloads, profiled: (info, launches, called off)."""
    rsa.reload_env()
    k, v = keys_t.clone(), torch.arange(keys_t.numel(), dtype=torch.int32, device="cuda")
    (_, _, info), launches, off = profiled(lambda: rsa.radix_sort_pairs(k, junk_like(k), v, junk_like(v), dtype=dt, order=order))
    print("plain key + payload sort: route", info.hybrid, "hist and leaf launches", launches, "called off", off)
    return info, launches, off


def assert_plain_route(info, launches, hybrid):
    """The plain sort took route `hybrid` (5 or 1), and its launches say so too: a histogram on every route but 5, leaves on both."""
    assert info.hybrid == hybrid, ("the plain sort", info.hybrid, launches, "wanted route", hybrid)
    assert (launches[0] == 0) == (hybrid == 5) and launches[1] >= 1, ("the plain sort", info.hybrid, launches)


# ---- reduce -----------------------------------------------------------------------------------------------------------------------
def reduce_case(tag, kbits, dt, vbits, vdt, order, hybrid, grp=None):
    """One radix_sort_reduce with every output against reduce_lib; the sort route, the inner route, the inputs unwritten."""
    n = kbits.size
    grp = rl.groups(kbits, dt, order) if grp is None else grp
    want = rl.want_reduce(grp, vbits, vdt)
    k, v = dev(kbits), dev(vbits)
    rsa.reload_env()
    out, _, off = profiled(lambda: rsa.radix_sort_reduce(k, v, dtype=dt, val_dtype=vdt, order=order, sum=True, min=True, max=True, counts=True))
    ok, cn, sm, mn, mx, info = out
    tag = "%s kdt=%d vdt=%d order=%d n=%d route=%d inner=%d called off=%d" % (tag, dt, vdt, order, n, info.route, info.sort.hybrid, off)
    print(tag)
    assert info.route == rsa.REDUCE_SORT and info.table_bytes == 0, tag
    if hybrid is None:
        assert info.sort.hybrid != 5 and off >= 1, (tag, "wanted an attempt without a histogram that was called off", off)
    else:
        assert info.sort.hybrid == hybrid, (tag, "wanted inner route", hybrid)
    unwritten(tag, k, kbits, dt)
    unwritten(tag, v, vbits, vdt)
    got = (bits_of(ok, dt), cn.cpu().numpy().view(np.uint32).astype(np.uint64), sm.cpu().numpy().view(np.uint64), bits_of(mn, vdt), bits_of(mx, vdt))
    il.compare_reduce(tag, got, want)
    assert info.sort.key_bytes == 4
    return info


@pytest.fixture(scope="module")
def keys22():
    """The 4-byte bit patterns most cases share (read as u32, i32 or f32 keys)."""
    return {"wide": il.wide(il.N22, ol.U32, 7101), "ties": il.wide_ties(il.N22, ol.U32, 7102)}


@pytest.mark.parametrize("keys,order", [("wide", ol.ASC), ("ties", ol.ASC), ("ties", ol.DESC)], ids=["wide", "ties", "ties-desc"])
@pytest.mark.parametrize("dt,vdt", [(ol.U32, ol.I32), (ol.F32, ol.F32), (ol.I32, ol.U32)], ids=["u32-i32", "f32-f32", "i32-u32"])
def test_1_reduce_without_histogram(keys22, keys, order, dt, vdt):
    """`wide` keys: nearly every group has one element, so a value beside the wrong key shows in sum, min and max at once;
    `ties`: the groups' sums, and min / max over ties, in both orders."""
    reduce_case("reduce " + keys, keys22[keys], dt, rl.small_ints(il.N22, vdt, 7110 + vdt), vdt, order, 5)


# ---- join -------------------------------------------------------------------------------------------------------------------------
def join_case(tag, want, how, lt, rt, route=rsa.JOIN_MERGE):
    """Phase 1 and phase 2 against join_lib (start, count, right_perm, the number of pairs, the expanded pairs; route; both inputs
    unwritten; left_sorted == 1 on the merge route).  Returns (info, launches, called off) of phase 1."""
    left_join = how == "left"
    (n_pairs, st, ct, pm, info), launches, off = profiled(
        lambda: rsa.radix_sort_join_ranges(lt, rt, dtype=want.dt, order=want.order, how=how))
    tag = (tag, how, "route", info.route, "right side's sort", info.sort.hybrid, "launches", launches, "called off", off)
    print(tag)
    jl.check(tag, want, st, ct, pm, n_pairs, info, left_join, route, lt, rt)
    li, ri, total = rsa.radix_sort_join_pairs(st, ct, pm, how, n_pairs=n_pairs)
    torch.cuda.synchronize()
    wl, wr = want.pairs(left_join)
    assert total == wl.size, tag
    il.same(tag, "left_idx", jl.signed(li), wl)
    il.same(tag, "right_idx", jl.signed(ri), wr)
    return info, launches, off


def left_sort_launches(monkeypatch, want, lt, rt, merged):
    """What the MERGE join booked (`merged`) beyond the SEARCH join of the same sides: the launches of its sort of the left side."""
    monkeypatch.setenv("RSX_JOIN_FORCE", "2")
    rsa.reload_env()
    (_, _, _, _, info), base, _ = profiled(lambda: rsa.radix_sort_join_ranges(lt, rt, dtype=want.dt, order=want.order))
    assert info.route == rsa.JOIN_SEARCH and info.left_sorted == 0
    monkeypatch.delenv("RSX_JOIN_FORCE")
    rsa.reload_env()
    return (merged[0] - base[0], merged[1] - base[1])


JOIN_CASES = {"u32": (ol.U32, ol.ASC, False, 7201), "f32-desc": (ol.F32, ol.DESC, True, 7202)}


@pytest.fixture(scope="module")
def join_sides():
    made = {}

    def get(name):
        if name not in made:
            dt, order, specials, seed = JOIN_CASES[name]
            left, right = il.join_sides(il.JOIN_LEFT, il.JOIN_RIGHT, dt, seed, specials)
            made[name] = jl.Want(left, right, dt, order)
        return made[name]
    return get


@pytest.mark.parametrize("name", list(JOIN_CASES))
def test_2_join_default_merge(join_sides, name, monkeypatch):
    """2^22 + 5 left rows against 2^20 + 3 right rows, nothing forced: the MERGE route, whose (key, iota) sort of the left side goes
    without a histogram; the right side's index sort is one MSB pass and leaves."""
    want = join_sides(name)
    assert "RSX_JOIN_FORCE" not in os.environ
    lt, rt = dev(want.left), dev(want.right)
    for how in ("inner", "left"):
        rsa.reload_env()
        info, merged, _ = join_case("join " + name, want, how, lt, rt)
        assert info.left_sorted == 1 and info.sort.hybrid == 1, (name, how, info.left_sorted, info.sort.hybrid)
    if want.dt == ol.F32:
        sp = il.float_specials(ol.F32)
        assert np.isin(sp, want.left).all() and np.isin(sp, want.right).all()
        assert (want.count[np.isin(want.left, sp)] >= 1).all() and want.count[want.left == sp[0]][0] == 2
    left_info, left_plain, _ = plain_pairs(lt, want.dt, want.order)
    assert_plain_route(left_info, left_plain, 5)
    assert left_sort_launches(monkeypatch, want, lt, rt, merged) == left_plain, "the left side's sort did not go without a histogram"


def test_2_join_right_side_without_histogram():
    """m = 2^22 + 7 right rows with right_perm wanted: the right side's index sort is on the route too."""
    left, right = il.join_sides(il.JOIN_LEFT, il.JOIN_RIGHT_BIG, ol.U32, 7203)
    want = jl.Want(left, right, ol.U32)
    info, _, _ = join_case("join, 2^22 + 7 right rows", want, "inner", dev(left), dev(right))
    assert info.left_sorted == 1 and info.sort.hybrid == 5, (info.left_sorted, info.sort.hybrid)


# ---- lex --------------------------------------------------------------------------------------------------------------------------
def lex_case(tag, cols, dtypes, orders, hybrids, called_off_groups=()):
    """radix_sort_lex against lex_lib.lexsort_perm; `hybrids`: the inner route of every group, group 0 (the last column) first --
    None: any route but 5, after an attempt that was called off."""
    tens = [dev(c) for c in cols]
    rsa.reload_env()
    (idx, info), _, off = profiled(lambda: rsa.radix_sort_lex(tens, orders=orders, dtypes=dtypes))
    got_routes = [int(g.hybrid) for g in info.group[:info.ngroups]]
    tag = (tag, "inner routes", got_routes, "called off", off)
    print(tag)
    assert info.ngroups == len(cols) and [int(g.key_bytes) for g in info.group[:info.ngroups]] == [4] * len(cols), tag
    for g, want_route in zip(got_routes, hybrids):
        assert (g != 5 and off >= 1) if want_route is None else g == want_route, (tag, "wanted", hybrids, "called off", off)
    for t, c, dt in zip(tens, cols, dtypes):
        unwritten(tag, t, c, dt)
    il.same(tag, "the permutation", idx.cpu().numpy().view(np.uint32).astype(np.int64), xl.lexsort_perm(cols, dtypes, orders))
    return info


def test_3_lex_three_columns(keys22):
    """Three u32 columns that tie everywhere, (ASC, DESC, ASC): group 0 through the rank sort, the others through the key + payload
    sort with the permutation as payload, each sorted as u32 without a histogram."""
    cols = [keys22["ties"], il.wide_ties(il.N22, ol.U32, 7301), il.wide_ties(il.N22, ol.U32, 7302)]
    info = lex_case("lex u32 x 3", cols, [ol.U32] * 3, [ol.ASC, ol.DESC, ol.ASC], [5, 5, 5])
    assert [int(g.sorted_as) for g in info.group[:3]] == [ol.U32] * 3


def test_3_lex_float_and_int_columns(keys22):
    cols = [il.with_specials(keys22["ties"], ol.F32, 7303), il.wide_ties(il.N22, ol.I32, 7304)]
    lex_case("lex (f32, i32)", cols, [ol.F32, ol.I32], [ol.DESC, ol.ASC], [5, 5])


# ---- topk and nth -----------------------------------------------------------------------------------------------------------------
def topk_case(tag, want, src_t, k, route, launches=None, seen=None):
    (keys, idx, info), got, off = profiled(lambda: rsa.radix_sort_topk(src_t, k, dtype=want.dt, order=want.order))
    if seen is not None:
        seen.append(got)
    print(tag, "route", info.route, "launches", got, "called off", off)
    tl.check((tag, "launches", got), want, k, keys, idx, info, route)
    unwritten(tag, src_t, want.bits, want.dt)
    if launches is not None:
        assert got == launches, (tag, "hist and leaf launches", got, "a plain rank sort of the same keys", launches)
    return off


def nth_case(tag, want, src_t, ranks, launches):
    (keys, idx, n_less, n_equal, info), got, off = profiled(lambda: rsa.radix_sort_nth(src_t, ranks, dtype=want.dt, order=want.order))
    print(tag, "route", info.route, "launches", got, "called off", off)
    nl.check((tag, "launches", got), want, ranks, keys, idx, n_less, n_equal, info, rsa.NTH_SORT)
    unwritten(tag, src_t, want.bits, want.dt)
    assert got == launches, (tag, "hist and leaf launches", got, "a plain rank sort of the same keys", launches)
    return off


@pytest.fixture(scope="module")
def ranked22(keys22):
    return {"u32": il.Ranked(keys22["ties"], ol.U32), "f32-desc": il.Ranked(il.with_specials(keys22["ties"], ol.F32, 7401), ol.F32, ol.DESC)}


@pytest.mark.parametrize("name", ["u32", "f32-desc"])
def test_4_topk_and_nth_sort_route(ranked22, name):
    """k = n / 2 and 65 distinct ranks (one more than the select route takes): both go by the rank sort of the whole input."""
    want = ranked22[name]
    n = want.bits.size
    src_t = dev(want.bits)
    info, launches, _ = plain_rank(src_t, want.dt, want.order)
    assert_plain_route(info, launches, 5)
    rsa.reload_env()
    topk_case("topk " + name, want, src_t, n // 2, rsa.TOPK_SORT, launches)
    ranks, (lo, hi) = il.nth_ranks(want.kd, rsa.NTH_MAX_SELECT_RANKS + 1)
    assert {0, n - 1, lo, hi} <= set(int(r) for r in ranks) and np.unique(ranks).size == 65
    nth_case("nth " + name, want, src_t, ranks, launches)


def test_5_topk_select_with_more_than_2_22_survivors():
    """n = 2^25 + 8, k = 2^22 + 1 = n / 8: the select route, whose k survivors go through the key + payload sort in pk | pk2 | pi | pi2.
    The survivors are the smallest eighth of evenly spread keys: 32 of the 256 top digits hold them all, eight shares each, so the
    attempt without a histogram that their number invites overflows its level-1 slots and is called off -- the sort behind it
    starts from pk and pi again."""
    n, k = (1 << 25) + 8, (1 << 22) + 1
    assert k == n // 8
    want = il.FirstK(il.wide(n, ol.U32, 7501), ol.U32, k)
    assert not il.slots_fit(want.first(k)[0], ol.U32) and int(want.first(k)[0].max()) >> 24 < 33
    launches = []
    off = topk_case("topk select", want, dev(want.bits), k, rsa.TOPK_SELECT, seen=launches)
    # (the selection's own kernels are not booked in the profile: every launch counted here is the survivors' sort's)
    assert off >= 1 and launches[0][0] >= 1, ("the survivors' sort: wanted an attempt that was called off, then a histogram", off, launches)


# ---- locate and partition ---------------------------------------------------------------------------------------------------------
def locate_values(bits, dt, count, seed):
    """`count` distinct values in no order, half of them keys, half of them none."""
    rng = np.random.default_rng(seed)
    u = np.unique(np.concatenate([bits[rng.integers(0, bits.size, count)], il.wide(count, dt, seed)]))
    assert u.size >= count
    return rng.permutation(u)[:count].copy()


def locate_case(tag, want, vals, src_t, hybrid=5):
    vals_t = dev(vals)
    info, le, eq, bi = rsa.radix_sort_locate(src_t, vals_t, dtype=want.dt, order=want.order, less=True, equal=True, bins=True)
    torch.cuda.synchronize()
    tag = (tag, "route", info.route, "inner", info.sort.hybrid)
    print(tag)
    ll.check(tag, want, vals, src_t, vals_t, le, eq, bi, False, info, rsa.LOCATE_SORT)
    assert (info.sort.hybrid != 5) if hybrid is None else (info.sort.hybrid == hybrid), (tag, "wanted inner route", hybrid)
    assert info.sort.key_bytes == ol.DTYPE_SIZE[want.dt], tag


def partition_case(tag, want, edges, src_t, locate_route, locate_hybrid):
    edges_t = dev(edges)
    info, keys, idx, off = rsa.radix_sort_partition(src_t, edges_t, dtype=want.dt, order=want.order, keys=True, idx=True, offsets=True)
    torch.cuda.synchronize()
    tag = (tag, "route", info.route, "locate", info.locate.route, "its sort", info.locate.sort.hybrid, "the bins' sort", info.sort.hybrid)
    print(tag)
    ptl.check(tag, want, edges, src_t, edges_t, keys, idx, off, False, info, rsa.PARTITION_SORT)
    assert info.locate.route == locate_route and info.locate.sort.hybrid == locate_hybrid, tag
    # the bins are below 2^13: two kept columns at the most, which no route but one pass per column takes
    assert info.sort.hybrid == 0 and info.sort.ncols <= 2, tag


@pytest.fixture(scope="module")
def keys23():
    return ptl.Want(il.wide(il.N23, ol.U32, 7601), ol.U32)


def test_6_locate_u32_keys_alone(keys23):
    """2^23 + 3 u32 keys (the floor of keys alone is 7.5 Mi) and 5000 distinct values, more than the search route holds in LDS."""
    locate_case("locate u32", keys23, locate_values(keys23.bits, ol.U32, 5000, 7602), dev(keys23.bits))


def test_6_locate_u64_keys_alone():
    want = ll.Want(il.wide(il.N64, ol.U64, 7603), ol.U64, ol.DESC)
    locate_case("locate u64", want, locate_values(want.bits, ol.U64, 5000, 7604), dev(want.bits))


def test_6_locate_with_the_floor_lowered(keys22, monkeypatch):
    """RSX_BLIND_MIN_LOG2=22: 2^22 + 3 keys alone go without a histogram; and by the histogram without the switch."""
    want = ll.Want(keys22["wide"], ol.U32)
    vals = locate_values(want.bits, ol.U32, 5000, 7605)
    src_t = dev(want.bits)
    locate_case("locate, default floor", want, vals, src_t, hybrid=1)      # (keys alone below the floor: one MSB pass and leaves)
    monkeypatch.setenv("RSX_BLIND_MIN_LOG2", "22")
    rsa.reload_env()
    locate_case("locate, RSX_BLIND_MIN_LOG2=22", want, vals, src_t, hybrid=5)


def test_6_partition_by_sort(keys23, monkeypatch):
    """The same 2^23 + 3 keys split by 300 edges (more than the scatter route's 255) and by 5000.  The sort route finds the bins
    with rsx_sort_locate_device's machinery: 5000 edges send it to ITS sort route, which sorts the keys alone without a histogram;
    300 edges fit its search route, which sorts no keys -- unless RSX_LOCATE_FORCE=2 closes it."""
    src_t = dev(keys23.bits)
    e300, e5000 = locate_values(keys23.bits, ol.U32, 300, 7606), locate_values(keys23.bits, ol.U32, 5000, 7607)
    partition_case("partition, 5000 edges", keys23, e5000, src_t, rsa.LOCATE_SORT, 5)
    partition_case("partition, 300 edges", keys23, e300, src_t, rsa.LOCATE_SEARCH, 0)
    monkeypatch.setenv("RSX_LOCATE_FORCE", "2")
    rsa.reload_env()
    partition_case("partition, 300 edges, RSX_LOCATE_FORCE=2", keys23, e300, src_t, rsa.LOCATE_SORT, 5)


# ---- an attempt called off after the level-1 slots were written -------------------------------------------------------------------
@pytest.fixture(scope="module")
def overflow_keys():
    return {d: il.overflowing(il.N22, 7700 + d, d) for d in (0x05, 0xF3)}


DIGITS = pytest.mark.parametrize("digit", [0x05, 0xF3], ids=["0x05", "0xF3"])


@DIGITS
def test_7_called_off_inside_reduce(overflow_keys, digit):
    """Random u32 values: a first value buffer the attempt damaged shows per element (nearly every group has one)."""
    a = overflow_keys[digit]
    reduce_case("reduce, called off", a, ol.U32, pl.payloads("random", a.size, 4, 7710 + digit), ol.U32, ol.ASC, None)


@DIGITS
def test_7_called_off_inside_join(overflow_keys, digit, monkeypatch):
    """The overflowing keys as the left side of a default MERGE join: start and count come back through the left permutation."""
    left = overflow_keys[digit]
    rng = np.random.default_rng(7720 + digit)
    right = np.concatenate([left[rng.choice(left.size, 1 << 19, replace=False)], il.wide((1 << 19) + 3, ol.U32, 7721 + digit)])
    want = jl.Want(left, right, ol.U32)
    assert want.n_pairs(True) <= il.JOIN_MAX_PAIRS
    lt, rt = dev(left), dev(right)
    rsa.reload_env()
    info, merged, off = join_case("join, called off", want, "left", lt, rt)
    assert off >= 1, "no launch of the join was booked as called off"
    left_info, left_plain, plain_off = plain_pairs(lt, ol.U32)
    assert left_info.hybrid != 5 and plain_off >= 1, (left_info.hybrid, plain_off)
    assert left_sort_launches(monkeypatch, want, lt, rt, merged) == left_plain


@DIGITS
def test_7_called_off_inside_lex(overflow_keys, digit, keys22):
    """The overflowing keys as column 0 of two: the last group's key + payload sort carries the permutation the first group made."""
    lex_case("lex, called off", [overflow_keys[digit], keys22["ties"]], [ol.U32, ol.U32], [ol.ASC, ol.ASC], [5, None])


@DIGITS
def test_7_called_off_inside_topk(overflow_keys, digit):
    want = il.Ranked(overflow_keys[digit], ol.U32)
    src_t = dev(want.bits)
    info, launches, plain_off = plain_rank(src_t, ol.U32)
    assert info.hybrid != 5 and plain_off >= 1, (info.hybrid, plain_off)
    rsa.reload_env()
    off = topk_case("topk, called off", want, src_t, want.bits.size // 2, rsa.TOPK_SORT, launches)
    assert off >= 1, "no launch of the top-k call was booked as called off"


# ---- one MSB pass and leaves ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys300k():
    return il.wide(il.N_ONE_LEVEL, ol.U32, 7801)


def test_8_one_level_inside_reduce_and_rankdata(keys300k, monkeypatch):
    reduce_case("reduce, one level", keys300k, ol.U32, rl.small_ints(keys300k.size, ol.I32, 7802), ol.I32, ol.ASC, 1)
    monkeypatch.setenv("RSX_RANKDATA_NO_TABLES", "1")
    rsa.reload_env()
    src_t = dev(keys300k)
    place, less, equal, info = rsa.radix_sort_rankdata(src_t, dtype=ol.U32, place=True, less=True, equal=True)
    torch.cuda.synchronize()
    print("rankdata: route", info.route, "inner", info.sort.hybrid)
    assert info.route == rsa.RANKDATA_SORT and info.sort.hybrid == 1, (info.route, info.sort.hybrid)
    unwritten("rankdata", src_t, keys300k, ol.U32)
    for name, t, w in zip(("place", "less", "equal"), (place, less, equal), rkl.want_rankdata(keys300k, ol.U32)):
        il.same("rankdata, one level", name, t.cpu().numpy().view(np.uint32).astype(np.uint64), w)


def test_8_one_level_inside_join(keys300k, monkeypatch):
    rng = np.random.default_rng(7803)
    right = np.concatenate([keys300k[rng.choice(keys300k.size, 50000, replace=False)], il.wide(50003, ol.U32, 7804)])
    want = jl.Want(keys300k, right, ol.U32)
    lt, rt = dev(want.left), dev(want.right)
    monkeypatch.setenv("RSX_JOIN_FORCE", "3")
    rsa.reload_env()
    info, merged, _ = join_case("join, one level", want, "inner", lt, rt)
    assert info.left_sorted == 1 and info.sort.hybrid == 1, (info.left_sorted, info.sort.hybrid)
    left_info, left_plain, _ = plain_pairs(lt, ol.U32)
    assert_plain_route(left_info, left_plain, 1)
    assert left_sort_launches(monkeypatch, want, lt, rt, merged) == left_plain


def test_8_one_level_inside_lex(keys300k):
    lex_case("lex, one level", [keys300k, il.wide(keys300k.size, ol.U32, 7805)], [ol.U32, ol.U32], [ol.ASC, ol.DESC], [1, 1])


def test_8_one_level_inside_topk_and_nth(keys300k):
    want = il.Ranked(np.concatenate([keys300k[:-9], keys300k[:9]]), ol.U32)     # (nine keys twice: a run of ties for the ranks)
    src_t = dev(want.bits)
    info, launches, _ = plain_rank(src_t, ol.U32)
    assert_plain_route(info, launches, 1)
    topk_case("topk, one level", want, src_t, want.bits.size // 2, rsa.TOPK_SORT, launches)
    ranks, _ = il.nth_ranks(want.kd, rsa.NTH_MAX_SELECT_RANKS + 1)
    nth_case("nth, one level", want, src_t, ranks, launches)


# ---- sequences on one context -----------------------------------------------------------------------------------------------------
def test_9_reduce_large_small_large(keys22):
    """Case 1, the same feature at n = 70001, case 1 again, nothing released in between: a pointer kept into a slack buffer that
    the large call allocated anew would show in the third call, one into a buffer the small call shrank in the second."""
    a, v = keys22["wide"], rl.small_ints(il.N22, ol.I32, 7901)
    grp = rl.groups(a, ol.U32)
    reduce_case("reduce, first", a, ol.U32, v, ol.I32, ol.ASC, 5, grp)
    reduce_case("reduce, 70001", a[:70001], ol.U32, v[:70001], ol.I32, ol.ASC, 1)
    reduce_case("reduce, again", a, ol.U32, v, ol.I32, ol.ASC, 5, grp)


def test_9_join_large_small_large(join_sides, monkeypatch):
    want = join_sides("u32")
    small = jl.Want(want.left[:70001], want.right[:70001], ol.U32)
    lt, rt = dev(want.left), dev(want.right)
    info, first, _ = join_case("join, first", want, "inner", lt, rt)
    assert info.sort.hybrid == 1
    info, _, _ = join_case("join, 70001", small, "inner", dev(small.left), dev(small.right), route=rsa.JOIN_SEARCH)
    assert info.sort.hybrid == 1 and info.left_sorted == 0
    info, again, _ = join_case("join, again", want, "left", lt, rt)
    assert info.sort.hybrid == 1
    # the left side's sort of the first and of the third call (measured above, compared once the sequence is over)
    left_info, left_plain, _ = plain_pairs(lt, ol.U32)
    assert_plain_route(left_info, left_plain, 5)
    assert first == again and left_sort_launches(monkeypatch, want, lt, rt, again) == left_plain


# ---- level-1 slots in the features' second buffers --------------------------------------------------------------------------------
# At 2^22 + 3 pairs a level-1 slot (20480 pairs) is smaller than a tile of the pass and all 256 slots lie in scratch memory.  From
# about 6.7 Mi pairs on a slot holds a tile, and the 204 slots that fit lie in the second key and payload buffers the feature hands
# over -- reduce's v1 = v0 + npad, join's k1 = k0 + npad with start and count behind it.
def test_10_reduce_with_slots_in_the_second_buffers(keys23):
    reduce_case("reduce, 2^23 + 3", keys23.bits, ol.U32, rl.small_ints(il.N23, ol.I32, 8001), ol.I32, ol.ASC, 5)


@DIGITS
def test_10_reduce_called_off_after_the_second_buffers_were_written(digit):
    """Digit 0x05's slot lies in the second buffers, 0xF3's in scratch memory; random values say per element whether v0 survived."""
    a = il.overflowing(il.N23, 8010 + digit, digit)
    assert il.level1_slot(a.size) >= 32768 and not il.slots_fit(a, ol.U32)
    reduce_case("reduce, 2^23 + 3, called off", a, ol.U32, pl.payloads("random", a.size, 4, 8011 + digit), ol.U32, ol.ASC, None)


def test_10_join_with_slots_in_the_second_buffers(monkeypatch):
    left, right = il.join_sides(il.N23 + 2, il.JOIN_RIGHT, ol.U32, 8020)
    want = jl.Want(left, right, ol.U32)
    assert want.n_pairs(True) <= 2 * il.JOIN_MAX_PAIRS
    lt, rt = dev(left), dev(right)
    info, merged, _ = join_case("join, 2^23 + 5 left rows", want, "left", lt, rt)
    assert info.left_sorted == 1 and info.sort.hybrid == 1, (info.left_sorted, info.sort.hybrid)
    left_info, left_plain, _ = plain_pairs(lt, ol.U32)
    assert_plain_route(left_info, left_plain, 5)
    assert left_sort_launches(monkeypatch, want, lt, rt, merged) == left_plain
