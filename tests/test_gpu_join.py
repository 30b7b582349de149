"""rsx_sort_join_device and rsx_join_pairs_device on the GPU against NumPy on the oracle's derived keys (tests/join_lib.py): phase 1
on the table route with the route asserted (every edge of the count table and of the test of the fixed bits), on the search and
the merge route forced, every subset of the outputs on every route, counting above 32 bits; phase 2 on ranges made by hand -- the
expansion reads nothing else -- for inner and left, 4- and 8-byte indices, at every edge of its row tiles and output tiles; and
the Python wrappers radix_sort_join and isin.  n, m <= 2^17 throughout."""
import itertools

import numpy as np
import pytest

import join_lib as jl
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_NP = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
ROW, EXP = rsa.JOIN_ROW_TILE, rsa.JOIN_EXPAND_TILE
SENTINEL = -7
ENVS = ("RSX_JOIN_FORCE", "RSX_JOIN_NO_TABLE")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()


def _route(monkeypatch, force=None, no_table=False):
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    if force:
        monkeypatch.setenv("RSX_JOIN_FORCE", str(force))
    if no_table:
        monkeypatch.setenv("RSX_JOIN_NO_TABLE", "1")
    rsa.reload_env()


def _dev(bits):
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(_NP[a.itemsize]).copy()).cuda()


def _idx(size, ib):
    """An index output of `size` entries and one sentinel behind them."""
    return torch.full((size + 1,), SENTINEL, dtype=torch.int32 if ib == 4 else torch.int64, device="cuda")


def _phase1(tag, left, right, dt, order=ol.ASC, ib=4, flags=0, outs=(True, True, True), route=None, want=None):
    want = want if want is not None else jl.Want(left, right, dt, order)
    n, m = want.left.size, want.right.size
    lt, rt = _dev(want.left), _dev(want.right)
    st, ct, pm = (_idx(size, ib) if on else None for on, size in zip(outs, (n, n, m)))
    rc, pairs, info = jl.call_device(lt, n, rt, m, dt, order, ib, st, ct, pm, flags)
    assert rc == 0, (tag, rsa.lib().rsx_last_error())
    torch.cuda.synchronize()
    for t in (st, ct, pm):
        assert t is None or int(t[-1]) == SENTINEL, (tag, "written past the end")
    cut = lambda t: None if t is None else t[:-1]
    jl.check(tag, want, cut(st), cut(ct), cut(pm), pairs, info, bool(flags & rsa.JOIN_LEFT), route, lt, rt)
    return want, info


def _masked(dt, mask, fixed, size, seed):
    """Bit patterns fixed | (random & mask)."""
    t = ol.NP_BITS[dt]
    return (ol.splitmix_fill(size, dt, seed).astype(t) & t(mask)) | t(fixed & ~mask & ((1 << (8 * ol.DTYPE_SIZE[dt])) - 1))


def _mixed_left(right, dt, size, seed, strangers):
    """Left keys: two thirds drawn from the right keys, the rest from `strangers`."""
    rng = np.random.default_rng(seed)
    a = right[rng.integers(0, right.size, size=size)].copy()
    k = size // 3
    a[:k] = strangers[rng.integers(0, strangers.size, size=k)]
    return rng.permutation(a).astype(ol.NP_BITS[dt])


# ---- phase 1, the table route ---------------------------------------------------------------------------------------------------

def test_table_u8_keys():
    right = ol.splitmix_fill(3001, ol.U8, 11) % np.uint8(200)
    left = ol.splitmix_fill(5003, ol.U8, 12)
    for flags in (0, rsa.JOIN_LEFT):
        _, info = _phase1("u8", left, right, ol.U8, flags=flags, route=rsa.JOIN_TABLE)
    _phase1("i8 desc", left, right, ol.I8, ol.DESC, ib=8, route=rsa.JOIN_TABLE)


def test_table_u32_one_byte_column():
    right = _masked(ol.U32, 0x0000FF00, 0xC0DE0042, 3000, 21)
    left = _mixed_left(right, ol.U32, 5000, 22, ol.splitmix_fill(700, ol.U32, 23))
    _, info = _phase1("u32 one column", left, right, ol.U32, route=rsa.JOIN_TABLE)
    assert info.varying_bits == 8


MASK16 = 0x00F0FF0F


def test_table_u32_three_runs_and_one_bit_more(monkeypatch):
    right = _masked(ol.U32, MASK16, 0x5A0A00A0, 4000, 31)
    strangers = np.concatenate([ol.splitmix_fill(500, ol.U32, 32), _masked(ol.U32, MASK16, 0x5A0A00A0, 500, 33)])
    left = _mixed_left(right, ol.U32, 6001, 34, strangers)
    want, info = _phase1("mask16", left, right, ol.U32, route=rsa.JOIN_TABLE)
    assert info.varying_bits == 16
    # the same inputs with the table route closed, and on both forced routes: the same answers
    _route(monkeypatch, no_table=True)
    _, info = _phase1("mask16 no table", left, right, ol.U32, want=want)
    assert info.route == rsa.JOIN_SEARCH and info.varying_bits == 16
    for force, route in ((2, rsa.JOIN_SEARCH), (3, rsa.JOIN_MERGE)):
        _route(monkeypatch, force=force)
        _phase1("mask16 forced %d" % force, left, right, ol.U32, route=route, want=want)
    # one varying bit more: V = 17 must not take the table
    _route(monkeypatch)
    right17 = _masked(ol.U32, MASK16 | 0x01000000, 0x5A0A00A0, 4000, 35)
    _, info = _phase1("mask17", left, right17, ol.U32)
    assert info.route == rsa.JOIN_SEARCH and info.varying_bits == 17


def test_table_u16_full_range():
    right = ol.splitmix_fill(70001, ol.U16, 41)
    left = ol.splitmix_fill(50003, ol.U16, 42)
    _, info = _phase1("u16", left, right, ol.U16, flags=rsa.JOIN_LEFT, route=rsa.JOIN_TABLE)
    assert info.varying_bits == 16


def test_table_right_keys_all_equal():
    right = np.full(777, 0xDEADBEEF, dtype=np.uint32)
    left = np.array([0xDEADBEEF, 0xDEADBEEE, 0xDEADBEEF, 0x5EADBEEF, 0, 0xFFFFFFFF, 0xDEADBEEF], dtype=np.uint32)
    want, info = _phase1("all equal", left, right, ol.U32, route=rsa.JOIN_TABLE)
    assert info.varying_bits == 0 and list(want.count) == [777, 0, 777, 0, 0, 0, 777]
    _phase1("all equal, none matches", left[[1, 3, 4, 5]], right, ol.U32, flags=rsa.JOIN_LEFT, route=rsa.JOIN_TABLE)
    _phase1("all equal, all match", left[[0, 2, 6]], right, ol.U32, route=rsa.JOIN_TABLE)


def test_table_fixed_bits_and_table_ends():
    mask, fixed = 0x0FF0FF00, 0x50050055     # two runs of eight bits: bits 8 .. 15 and 20 .. 27
    ends = np.array([fixed & ~mask, (fixed & ~mask) | mask], dtype=np.uint32)
    right = _masked(ol.U32, mask, fixed, 5000, 51)
    right = right[~np.isin(right, ends)]
    inside = right[:64]
    # one bit off the fixed bits -- above the mask, between its runs, below it: no match, whatever the varying bits say
    off = np.concatenate([inside ^ np.uint32(1 << 30), inside ^ np.uint32(1 << 17), inside ^ np.uint32(1 << 3)])
    # the packed values 0 and 2^V - 1 (the read of offs[2^V]), present among the right keys and absent
    left = np.concatenate([inside, off, ends, inside])
    for tag, r in (("ends present", np.concatenate([right, ends, ends[1:]])), ("ends absent", right)):
        want, info = _phase1("fixed bits, " + tag, left, r, ol.U32, route=rsa.JOIN_TABLE)
        assert info.varying_bits == 16
        assert (want.count[:64] >= 1).all() and not want.count[64:64 + 192].any()
        assert list(want.count[256:258]) == ([1, 2] if tag == "ends present" else [0, 0])


def test_table_one_row_on_either_side():
    right = _masked(ol.U32, 0x00000FF0, 0x12340000, 2000, 61)
    _phase1("n = 1, match", right[5:6], right, ol.U32, route=rsa.JOIN_TABLE)
    _phase1("n = 1, none", right[5:6] ^ np.uint32(1 << 20), right, ol.U32, flags=rsa.JOIN_LEFT, route=rsa.JOIN_TABLE)
    left = _mixed_left(right, ol.U32, 3000, 62, ol.splitmix_fill(100, ol.U32, 63))
    want, info = _phase1("m = 1", left, right[7:8], ol.U32, route=rsa.JOIN_TABLE)
    assert info.varying_bits == 0 and info.sort.early_exit == 1 and want.count.max() == 1
    _phase1("n = m = 1, match", right[:1], right[:1], ol.U32, ib=8, route=rsa.JOIN_TABLE)
    _phase1("n = m = 1, none", right[:1], right[1:2] ^ np.uint32(1), ol.U32, route=rsa.JOIN_TABLE)
    _phase1("u8 n = m = 1", np.array([7], dtype=np.uint8), np.array([7], dtype=np.uint8), ol.U8, route=rsa.JOIN_TABLE)


@pytest.mark.parametrize("dt", [ol.U32, ol.U8, ol.U64])
def test_table_vector_tails(dt):
    kb = ol.DTYPE_SIZE[dt]
    right = _masked(dt, 0xFF if kb == 1 else 0x0000F0F0, 0 if kb == 1 else 0x77000001, 1500, 71)
    for n in (4097, 4098, 4099, 4096 + 15):
        left = _mixed_left(right, dt, n, 72 + n, ol.splitmix_fill(300, dt, 73))
        for off in (0, 1, 3):     # the left keys' distance from a 16-byte boundary, in elements
            lt = _dev(np.concatenate([np.zeros(off, dtype=left.dtype), left]))[off:]
            want = jl.Want(left, right, dt)
            rt = _dev(want.right)
            for ib in (4, 8):
                st, ct = _idx(n + 1, ib)[1:], _idx(n + 3, ib)[3:]     # outputs that are element-aligned only
                rc, pairs, info = jl.call_device(lt, n, rt, right.size, dt, ol.ASC, ib, st, ct, None)
                assert rc == 0, rsa.lib().rsx_last_error()
                torch.cuda.synchronize()
                assert int(st[-1]) == SENTINEL and int(ct[-1]) == SENTINEL
                jl.check("tails n=%d off=%d ib=%d" % (n, off, ib), want, st[:-1], ct[:-1], None, pairs, info, False, rsa.JOIN_TABLE, lt, rt)


F32_POS_ZERO, F32_NEG_ZERO = 0x00000000, 0x80000000


def test_table_floats_zeros_and_nan_payloads():
    # right: +0.0 and 1.0 + k 2^-15 (15 varying bits); left also holds -0.0 and NaNs, which differ in fixed bits
    ones = (np.uint32(0x3F800000) | (ol.splitmix_fill(3000, ol.U32, 81) & np.uint32(0xFF)) << np.uint32(8)).astype(np.uint32)
    right = np.concatenate([ones, np.full(5, F32_POS_ZERO, dtype=np.uint32)])
    odd = np.array([F32_POS_ZERO, F32_NEG_ZERO, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x3F800000, 0xBF800000], dtype=np.uint32)
    left = _mixed_left(right, ol.F32, 4001, 82, odd)
    for order in (ol.ASC, ol.DESC):
        want, info = _phase1("f32 zeros order=%d" % order, left, right, ol.F32, order, route=rsa.JOIN_TABLE)
        assert info.varying_bits <= 16
        assert (want.count[want.left == F32_NEG_ZERO] == 0).all() and (want.count[want.left == F32_POS_ZERO] == 5).all()
    # right: NaNs that differ in their payloads alone
    nans = (np.uint32(0x7FC00000) | (ol.splitmix_fill(2000, ol.U32, 83) & np.uint32(0x3FF))).astype(np.uint32)
    left = _mixed_left(nans, ol.F32, 3000, 84, np.concatenate([odd, nans[:50] | np.uint32(0x80000000)]))
    want, info = _phase1("f32 NaN payloads", left, nans, ol.F32, route=rsa.JOIN_TABLE)
    assert info.varying_bits == 10 and (want.count[(want.left & 0x80000000) != 0] == 0).all()


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt,mask,fixed", [(ol.I32, 0x8000FF0F, 0x12340000), (ol.I64, 0x000FF000000000FF, 0x8123000000004500),
                                           (ol.F64, 0x0000FFFF00000000, 0x3FF0000000000123), (ol.F64, 0x000000000FF00FF0, 0xBFF0000000000000)])
def test_table_signed_and_float_keys(dt, mask, fixed, order):
    right = _masked(dt, mask, fixed, 3500, 91)
    left = _mixed_left(right, dt, 5001, 92, np.concatenate([ol.splitmix_fill(400, dt, 93), _masked(dt, mask, fixed, 400, 94)]))
    _, info = _phase1("%s mask=%x order=%d" % (ol.DTYPE_NAMES[dt], mask, order), left, right, dt, order, ib=8 if order else 4,
                      flags=rsa.JOIN_LEFT if order else 0, route=rsa.JOIN_TABLE)
    assert info.varying_bits == bin(mask).count("1")


# ---- phase 1, the search and the merge route --------------------------------------------------------------------------------------

def _pooled(dt, n, m, seed):
    """Keys drawn from a pool a quarter the size of m: many rows match many."""
    pool = ol.splitmix_fill(max(m // 4, 1), dt, seed)
    rng = np.random.default_rng(seed)
    right = pool[rng.integers(0, pool.size, size=m)]
    left = _mixed_left(right, dt, n, seed + 1, ol.splitmix_fill(500, dt, seed + 2))
    return left, right


@pytest.mark.parametrize("force,route", [(2, rsa.JOIN_SEARCH), (3, rsa.JOIN_MERGE)])
@pytest.mark.parametrize("dt", [ol.U32, ol.U64])
def test_forced_routes_many_to_many(dt, force, route, monkeypatch):
    _route(monkeypatch, force=force)
    for n, m in ((5000, 3000), (3000, 5000)):
        left, right = _pooled(dt, n, m, 100 + dt)
        want = jl.Want(left, right, dt)
        assert want.count.max() > 1
        for ib, flags in ((4, 0), (8, rsa.JOIN_LEFT)):
            _, info = _phase1("pool %s n=%d m=%d" % (ol.DTYPE_NAMES[dt], n, m), left, right, dt, ib=ib, flags=flags, route=route, want=want)
            assert info.sort.early_exit == 0
    left, right = _pooled(dt, 2000, 3000, 110)
    _phase1("pool desc", left, right, dt, ol.DESC, route=route)
    _phase1("one left row", left[:1], right, dt, route=route)
    _phase1("one right row", left, right[:1], dt, route=route)


@pytest.mark.parametrize("force,route", [(None, rsa.JOIN_SEARCH), (2, rsa.JOIN_SEARCH), (3, rsa.JOIN_MERGE)])
def test_right_side_in_order_is_not_sorted(force, route, monkeypatch):
    _route(monkeypatch, force=force)
    left, right = _pooled(ol.U32, 4000, 3000, 120)
    right = np.sort(right)
    for outs in ((True, True, True), (True, True, False)):
        want, info = _phase1("sorted right", left, right, ol.U32, outs=outs, route=route)
        assert info.sort.early_exit == 2 and np.array_equal(want.perm, np.arange(right.size, dtype=np.uint64))


@pytest.mark.parametrize("force,route", [(None, rsa.JOIN_TABLE), (2, rsa.JOIN_SEARCH), (3, rsa.JOIN_MERGE)])
def test_every_subset_of_the_outputs(force, route, monkeypatch):
    _route(monkeypatch, force=force)
    right = _masked(ol.U32, 0x000FFF00, 0x40000007, 3000, 131)
    left = _mixed_left(right, ol.U32, 4001, 132, ol.splitmix_fill(300, ol.U32, 133))
    want = jl.Want(left, right, ol.U32)
    rot = itertools.cycle([(4, 0), (8, rsa.JOIN_LEFT)])
    for outs in itertools.product((False, True), repeat=3):
        ib, flags = next(rot)
        _phase1("subset %s" % (outs,), left, right, ol.U32, ib=ib, flags=flags, outs=outs, route=route, want=want)
    left8, right8 = ol.splitmix_fill(4001, ol.U8, 134), ol.splitmix_fill(1000, ol.U8, 135)
    want8 = jl.Want(left8, right8, ol.U8)
    for outs in itertools.product((False, True), repeat=3):
        _phase1("u8 subset %s" % (outs,), left8, right8, ol.U8, outs=outs, route=route, want=want8)


@pytest.mark.parametrize("force", [None, 2, 3])
def test_counting_above_32_bits(force, monkeypatch):
    _route(monkeypatch, force=force)
    n, m = 1 << 17, 1 << 16
    lt = torch.full((n,), 0x1234567, dtype=torch.int32, device="cuda")
    rt = torch.full((m,), 0x1234567, dtype=torch.int32, device="cuda")
    for flags in (0, rsa.JOIN_LEFT):
        rc, pairs, info = jl.call_device(lt, n, rt, m, ol.U32, ol.ASC, 4, None, None, None, flags)
        assert rc == 0, rsa.lib().rsx_last_error()
        assert pairs == 1 << 33 and info.route == (force or rsa.JOIN_TABLE)


# ---- phase 2: the expansion, on ranges made by hand ------------------------------------------------------------------------------

def _ranges(count, m, seed):
    """start / right_perm that go with `count`: a random permutation of m right rows, every row's range inside it."""
    rng = np.random.default_rng(seed)
    count = np.asarray(count, dtype=np.int64)
    assert count.max(initial=0) <= m
    start = (rng.random(count.size) * (m - count + 1)).astype(np.int64)
    return start, count, rng.permutation(m).astype(np.int64)


def _expand(tag, count, m, seed=1):
    start, count, perm = _ranges(count, m, seed)
    n = count.size
    for ib, left_join in itertools.product((4, 8), (False, True)):
        npi = np.int32 if ib == 4 else np.int64
        st, ct, pm = (torch.from_numpy(a.astype(npi)).cuda() for a in (start, count, perm))
        wl, wr = jl.pairs_of(start, count, perm, left_join)
        total = wl.size
        flags = rsa.JOIN_LEFT if left_join else 0
        what = (tag, ib, left_join)
        for want_l, want_r in ((True, True), (True, False), (False, True)):
            ol_t, or_t = (_idx(total, ib) if on else None for on in (want_l, want_r))
            rc, pairs = jl.call_pairs(st, ct, pm, n, m, ib, flags, ol_t, or_t, total)     # capacity == n_pairs
            assert rc == 0 and pairs == total, (what, rc, pairs, total, rsa.lib().rsx_last_error())
            torch.cuda.synchronize()
            if ol_t is not None:
                got = jl.signed(ol_t)
                assert np.array_equal(got[:-1], wl) and got[-1] == SENTINEL, (what, "out_left", np.flatnonzero(got[:-1] != wl)[:8])
            if or_t is not None:
                got = jl.signed(or_t)
                assert np.array_equal(got[:-1], wr) and got[-1] == SENTINEL, (what, "out_right", np.flatnonzero(got[:-1] != wr)[:8])
        if total:
            ol_t, or_t = _idx(total, ib), _idx(total, ib)
            rc, pairs = jl.call_pairs(st, ct, pm, n, m, ib, flags, ol_t, or_t, total - 1)     # one entry short
            assert rc == -1 and b"does not fit" in rsa.lib().rsx_last_error() and pairs == total, what
            torch.cuda.synchronize()
            assert bool((ol_t == SENTINEL).all()) and bool((or_t == SENTINEL).all()), (what, "written although it does not fit")
        for a, t in ((start, st), (count, ct), (perm, pm)):
            assert np.array_equal(t.cpu().numpy().astype(np.int64), a), (what, "an input was written")
    return total


def test_expand_counts_all_one():
    assert _expand("ones", np.ones(5000, dtype=np.int64), 5000) == 5000
    assert _expand("one row", np.ones(1, dtype=np.int64), 1) == 1


def test_expand_counts_all_zero():
    # (inner: no pairs, nothing written -- _expand's sentinels; left: n pairs of -1)
    _expand("zeros", np.zeros(3 * ROW + 5, dtype=np.int64), 10)
    _expand("zeros, no right rows", np.zeros(100, dtype=np.int64), 0)


def test_expand_zero_run_over_whole_row_tiles():
    count = np.zeros(5 * ROW + 10, dtype=np.int64)
    count[5], count[ROW - 1], count[4 * ROW], count[4 * ROW + 7], count[-2] = 3, 1, 2, 5, 4     # row tiles 1 .. 3 hold nothing
    _expand("zero run", count, 64)
    count = np.zeros(2 * ROW, dtype=np.int64)     # the first and the last row without a match, one row tile boundary between the others
    count[1:-1] = np.random.default_rng(5).integers(0, 4, size=count.size - 2)
    _expand("first and last row zero", count, 200)


def test_expand_one_row_larger_than_three_output_tiles():
    count = np.concatenate([np.ones(EXP // 2 - 3, dtype=np.int64), [3 * EXP + 1], np.zeros(7, dtype=np.int64), np.full(40, 2, dtype=np.int64)])
    _expand("big row in the middle of an output tile", count, 3 * EXP + 50)
    _expand("big row alone", np.array([3 * EXP + 1], dtype=np.int64), 3 * EXP + 1)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_expand_totals_at_the_output_tile(delta):
    assert _expand("ones", np.ones(2 * EXP + delta, dtype=np.int64), 3000) == 2 * EXP + delta
    count = np.full(ROW + 1, 7, dtype=np.int64)     # the same totals from rows of seven: a row tile of them and what is missing in one more row
    count[-1] = 2 * EXP + delta - 7 * ROW
    assert _expand("sevens", count, 3000) == 2 * EXP + delta


def test_expand_skewed_counts():
    rng = np.random.default_rng(9)
    count = (np.minimum(1.0 / rng.random(3 * ROW + 77) ** 1.3, 20001.0) - 1.0).astype(np.int64)     # Zipf-like, many zeros
    _expand("zipf", count, 20000)


# ---- the Python wrappers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["inner", "left"])
def test_radix_sort_join_wrapper(how, monkeypatch):
    left, right = _pooled(ol.U32, 5000, 3000, 140)
    want = jl.Want(left, right, ol.U32)
    wl, wr = want.pairs(how == "left")
    for force in (None, 3):
        _route(monkeypatch, force=force)
        li, ri, info, st, ct, pm = rsa.radix_sort_join(_dev(left), _dev(right), how=how, dtype=rsa.U32, return_ranges=True)
        assert li.dtype == torch.int32 and li.numel() == wl.size and ri.numel() == wl.size
        assert np.array_equal(jl.signed(li), wl) and np.array_equal(jl.signed(ri), wr)
        assert info.route == (rsa.JOIN_MERGE if force else rsa.JOIN_SEARCH)
        li2, ri2, none = rsa.radix_sort_join(None, None, how=how, ranges=(st, ct, pm))     # phase 2 alone, from the ranges
        assert none is None and torch.equal(li2, li) and torch.equal(ri2, ri)
    li, ri, info = rsa.radix_sort_join(_dev(left.astype(np.uint64)), _dev(right.astype(np.uint64)), how=how, dtype=rsa.U64, idx_dtype=torch.int64)
    assert li.dtype == torch.int64 and np.array_equal(jl.signed(li), wl) and np.array_equal(jl.signed(ri), wr)
    li, ri, info = rsa.radix_sort_join(_dev(left[:10] | np.uint32(1 << 31)), _dev(right & np.uint32(0x7FFFFFFF)), how=how, dtype=rsa.U32)
    assert li.numel() == (10 if how == "left" else 0) and (how == "inner" or bool((ri == -1).all()))
    _route(monkeypatch)
    hl, hr, hinfo, _, _, _ = rsa.radix_sort_join_host(left, right, rsa.U32, how=how)
    assert np.array_equal(jl.signed(hl), wl) and np.array_equal(jl.signed(hr), wr) and hinfo.route == rsa.JOIN_SEARCH


def test_isin_wrapper(monkeypatch):
    for dt, test, route in ((ol.U32, _masked(ol.U32, 0x0000FFF0, 0x10000001, 2000, 151), rsa.JOIN_TABLE),
                            (ol.F32, ol.splitmix_fill(2000, ol.F32, 152), rsa.JOIN_SEARCH), (ol.U8, ol.splitmix_fill(100, ol.U8, 153) % np.uint8(50), rsa.JOIN_TABLE)):
        src = _mixed_left(test, dt, 6001, 154, ol.splitmix_fill(900, dt, 155))
        mask, info = rsa.isin(_dev(src), _dev(test), dtype=dt)
        want = np.isin(ol.kdf_keys(src, dt), ol.kdf_keys(test, dt))
        assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want) and want.any() and not want.all()
        assert info.route == route
