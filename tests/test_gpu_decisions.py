"""One key from the edge: the library's two decisions with the reference's meaning (radix_sort.hpp:60-70) -- is the input sorted
already (then `src` comes back and `aux` stays untouched), and which byte columns vary (which also says where the result lies,
:92) -- at every place where one of its deciders has boundary code of its own.

Pre-sorted family: a base sorted in KDF order (with duplicates) takes the early exit; the same base with ONE descent, put at
every seam tests/decide_lib.py names (vector, wave, sweep, unaligned head, last vector and tail, the sample's places), does not,
and comes back sorted, bit for bit, with the oracle's result_in_aux and kept columns.  Kept-columns family: unsorted keys with
byte columns of the derived keys constant, and one bit of one key flipped in such a column.

    A  rsx_small_sort_kernel and its pair / rank siblings (n x size <= 64 KiB)
    B  rsx_hist_kernel: aligned and unaligned pointers, fused with the plan and not (RSX_NO_FUSED_HIST=1)
    C  rsx_blind_precheck_kernel and the level-1 pass's cmask / key0 check (RSX_BLIND_MIN_LOG2=22 brings them down to 4 Mi keys)
    D  rsx_log_hist_kernel / rsx_log_plan_kernel (RSX_LOG_MIN_LOG2=20)
    E  the device-scheduled entries (*_inplace_async)
    F  blocking rank and key + payload sorts

tests/test_decide_lib_cpu.py proves, with the reference restatement alone, that every input made here is what it is taken for
and that the expected results (the sorted base with one element moved: slices put together on the device) are the oracle's.
Routes are asserted only where a comment says why.  The oracle is asked per case for arrays up to 65536 keys, per base and
construction beyond (the decision depends on the position only through the moved element).
"""
import numpy as np
import pytest

import decide_lib as dl
import oracle_lib as ol
import pairs_lib as pl
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_CARRIER = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
_FILL = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
BLIND_ROUTE, LOG_ROUTE = 5, 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()
    yield
    torch.cuda.empty_cache()


def to_dev(bits):
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(_CARRIER[a.itemsize]).copy()).cuda()


def _scalar(v, ut):
    """A bit pattern as the Python integer of the same-width signed carrier."""
    return int(np.array([v], dtype=ut).view(_CARRIER[np.dtype(ut).itemsize])[0])


class Dev:
    """A base on the device: the pristine copy, what the pieces of an expected result are cut from, and the buffers that are
    sorted -- `offset` elements behind a 16-byte-aligned address."""

    def __init__(self, base, cut_from=None, offset=0):
        self.ut = base.dtype
        self.n = base.size
        self.pristine = to_dev(base)
        self.cut = self.pristine if cut_from is None else to_dev(cut_from)
        self.fill = _FILL[base.itemsize]
        self.src_full = torch.zeros(self.n + offset, dtype=self.pristine.dtype, device="cuda")
        self.aux_full = torch.full_like(self.src_full, self.fill)
        self.src, self.aux = self.src_full[offset:], self.aux_full[offset:]
        assert self.src.data_ptr() % 16 == (offset * base.itemsize) % 16

    def load(self, case=None):
        self.src.copy_(self.pristine)
        for i, v in (case.patches if case is not None else ()):
            self.src[i] = _scalar(v, self.ut)

    def put_together(self, pieces, cut=None):
        cut = self.cut if cut is None else cut
        ut = self.ut if cut is self.cut else np.uint32
        parts = [cut[pc[1]:pc[2]] if pc[0] == "s" else torch.tensor([_scalar(pc[1], ut)], dtype=cut.dtype, device="cuda")
                 for pc in pieces]
        return torch.cat(parts)

    def aux_untouched(self):
        return bool((self.aux_full == self.fill).all().item())


def _oracle_decision(a, dt, order):
    want, in_aux, info = ol.oracle_sort(a, dt, order)
    return want, in_aux, list(info.cols[:info.ncols]), int(info.early_exit)


_decisions = {}


def _decision(spec, s, case):
    """(result_in_aux, kept columns) of a perturbed array: the oracle's, per case for the small arrays, once per base and
    construction for the others."""
    if spec.n <= dl.SMALL:
        _, in_aux, cols, early = _oracle_decision(dl.apply_patches(s, case), spec.dtype, spec.order)
        assert early == 0
        return in_aux, cols
    key = (spec.base, spec.dtype, spec.order, spec.n, case.kind)
    if key not in _decisions:
        _, in_aux, cols, early = _oracle_decision(dl.apply_patches(s, case), spec.dtype, spec.order)
        assert early == 0
        _decisions[key] = (in_aux, cols)
    return _decisions[key]


def _sorted_exit(dev, spec, what):
    """radix_sort.hpp:60-62 on the unperturbed base: src returned, nothing kept, aux byte for byte untouched."""
    dev.load()
    dev.aux_full.fill_(dev.fill)
    res, info = rsa.radix_sort(dev.src, dev.aux, dtype=spec.dtype, order=spec.order)
    torch.cuda.synchronize()
    assert info.early_exit == 2 and info.ncols == 0 and info.result_in_aux == 0 and res is dev.src, (what, info.early_exit, info.ncols)
    assert torch.equal(dev.src, dev.pristine), what
    assert dev.aux_untouched(), what
    return info


def _one_descent(dev, spec, s, p, what, before=None):
    case = dl.descent_case(s, spec.dtype, spec.order, p)
    want_aux, want_cols = _decision(spec, s, case)
    dev.load(case)
    if before is not None:
        before()
    res, info = rsa.radix_sort(dev.src, dev.aux, dtype=spec.dtype, order=spec.order)
    what = (what, "p", p, case.kind, "route", info.hybrid)
    assert info.early_exit == 0, what
    assert info.result_in_aux == want_aux and info.kept_columns() == want_cols, (what, info.result_in_aux, info.kept_columns())
    assert torch.equal(res, dev.put_together(case.pieces)), what
    return info


def _presorted_keys_only(spec, offsets=None, before=None, route_of=None):
    s = dl.spec_base(spec)
    for off in (spec.offsets if offsets is None else offsets):
        dev = Dev(s, offset=off)
        what = (dl.spec_id(spec), "offset", off)
        _sorted_exit(dev, spec, what)
        for p in dl.spec_positions(spec, off):
            info = _one_descent(dev, spec, s, p, what, before)
            if route_of is not None:
                route_of[p] = int(info.hybrid)
        del dev


# ---- A: the one-workgroup kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", range(10), ids=ol.DTYPE_NAMES)
def test_a_small_sort_presorted_or_one_descent(dt):
    specs = [s for s in dl.presorted_specs("A") if s.dtype == dt]
    assert len(specs) == 10
    for spec in specs:
        _presorted_keys_only(spec)


def _rank(dev, spec, case=None):
    dev.load(case)
    ib = torch.full((2 * dev.n,), _FILL[4], dtype=torch.int32, device="cuda")
    half, info = rsa.radix_sort_rank(dev.src, ib, dtype=spec.dtype, order=spec.order)
    torch.cuda.synchronize()
    return half, info, ib


def _pairs(dev, spec, vals, case=None):
    dev.load(case)
    dev.aux_full.fill_(dev.fill)
    v = vals.clone()
    vaux = torch.full_like(v, _FILL[4])
    kr, vr, info = rsa.radix_sort_pairs(dev.src, dev.aux, v, vaux, dtype=spec.dtype, order=spec.order)
    torch.cuda.synchronize()
    return kr, vr, info, v, vaux


def _rank_and_pairs(spec, spots=None):
    """Blocking rank and key + payload sorts of a base and of every one-descent case of it.  Ranks against oracle_rank itself up
    to 70001 keys; beyond, against decide_lib.rank_pieces (pinned to oracle_rank in tests/test_decide_lib_cpu.py) and against
    oracle_rank at `spots` positions.  Payloads are not the input position (pairs_lib's random family)."""
    s = dl.spec_base(spec)
    n, dt, order = spec.n, spec.dtype, spec.order
    what = dl.spec_id(spec)
    dev = Dev(s)
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    vals_host = pl.payloads("random", n, 4, seed=n % 1000)
    vals = to_dev(vals_host)
    # sorted input: identity ranks in the half the oracle names, the other half untouched; keys and payloads where they were
    _, whalf, winfo, _ = ol.oracle_rank(s, dt, 4, order)
    half, info, ib = _rank(dev, spec)
    assert winfo.early_exit == 2 and info.early_exit == 2 and info.result_in_aux == whalf, what
    assert torch.equal(half, iota), what
    other = ib[:n] if whalf else ib[n:]
    assert bool((other == _FILL[4]).all().item()), what
    kr, vr, info, v, vaux = _pairs(dev, spec, vals)
    assert info.early_exit == 2 and info.result_in_aux == 0 and kr is dev.src and vr is v, what
    assert torch.equal(kr, dev.pristine) and torch.equal(vr, vals), what
    assert dev.aux_untouched() and bool((vaux == _FILL[4]).all().item()), what
    ps = dl.spec_positions(spec)
    ask = set(ps) if n <= 70001 else set(dl.spot_positions(ps, spots))
    for p in ps:
        case = dl.descent_case(s, dt, order, p)
        want_aux, want_cols = _decision(spec, s, case)
        perm = dev.put_together(dl.rank_pieces(s, dt, order, case), cut=iota)
        if p in ask:
            wr, wh, wi, _ = ol.oracle_rank(dl.apply_patches(s, case), dt, 4, order)
            assert wh == want_aux and wi.early_exit == 0
            assert np.array_equal(perm.cpu().numpy().view(np.uint32), wr), (what, p)
        half, info, _ = _rank(dev, spec, case)
        assert info.early_exit == 0 and info.result_in_aux == want_aux and info.kept_columns() == want_cols, (what, p, info.hybrid)
        assert torch.equal(half, perm), (what, "ranks", p, case.kind, info.hybrid)
        kr, vr, info, _, _ = _pairs(dev, spec, vals, case)
        assert info.early_exit == 0 and info.result_in_aux == want_aux and info.kept_columns() == want_cols, (what, p, info.hybrid)
        assert torch.equal(kr, dev.put_together(case.pieces)), (what, "keys", p, case.kind, info.hybrid)
        assert torch.equal(vr, vals[perm.long()]), (what, "payloads", p, case.kind, info.hybrid)


@pytest.mark.parametrize("spec", dl.presorted_specs("A-rank-pairs"), ids=dl.spec_id)
def test_a_small_rank_and_pairs(spec):
    _rank_and_pairs(spec)


# ---- B: the histogram kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "RSX_NO_FUSED_HIST"])
@pytest.mark.parametrize("spec", dl.presorted_specs("B"), ids=dl.spec_id)
def test_b_histogram_presorted_or_one_descent(spec, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("RSX_NO_FUSED_HIST", "1")
    _presorted_keys_only(spec)


# ---- C: the sample of the sorts without a histogram ---------------------------------------------------------------------------
@pytest.mark.parametrize("spec", dl.presorted_specs("C"), ids=dl.spec_id)
def test_c_sampled_presorted_or_one_descent(spec, monkeypatch):
    """Every case starts from a context that has forgotten its lost attempts (rsx_reload_env), so every case is an attempt; the
    route is recorded per position and printed.  It is NOT asserted, not even at p == 0, where thread 0 of the sample (keys
    0 .. 7) proves the descent itself: the sample reads 64 places of 128 CONSECUTIVE keys, and in a sorted array of 4 Mi keys
    that spread evenly the 128 keys of a place share their level-1 digit -- 128 of the 8192 samples in one digit, where
    rsx_blind_precheck_kernel allows twice the share, 64 (`s_maxs[0] <= 2 * NS / 256`: a slot holds 1.25 times the mean).  The
    sample takes a nearly sorted array for clustered keys and calls the attempt off; the histogram then decides.  What has to
    hold at every position is the decision and the result.  (The attempt that goes through, with a column the sample takes
    for constant, is test_kept_columns_one_stray_key_sampled's.)"""
    monkeypatch.setenv("RSX_BLIND_MIN_LOG2", "22")
    routes = {}
    _presorted_keys_only(spec, before=rsa.reload_env, route_of=routes)
    print("%s: routes by position %s" % (dl.spec_id(spec), sorted(routes.items())))


# ---- D: the (bit length, mantissa) route's own histogram --------------------------------------------------------------------
@pytest.mark.parametrize("spec", dl.presorted_specs("D"), ids=dl.spec_id)
def test_d_log_route_presorted_or_one_descent(spec, monkeypatch):
    monkeypatch.setenv("RSX_LOG_MIN_LOG2", "20")
    s = dl.spec_base(spec)
    dev = Dev(s)
    what = dl.spec_id(spec)
    _sorted_exit(dev, spec, what)
    monkeypatch.setenv("RSX_NO_BLIND", "1")        # (straight to this route's own histogram)
    _sorted_exit(dev, spec, (what, "RSX_NO_BLIND"))
    monkeypatch.delenv("RSX_NO_BLIND")
    for p in dl.spec_positions(spec):
        info = _one_descent(dev, spec, s, p, what, before=rsa.reload_env)
        if p != 0:          # (at p == 0 the first key changes, and with it the window the sample finds)
            assert info.hybrid == LOG_ROUTE, (what, p, info.hybrid)


# ---- E: the device-scheduled entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", dl.presorted_specs("E"), ids=dl.spec_id)
def test_e_inplace_async_presorted_or_one_descent(spec, monkeypatch):
    if spec.n == dl.N_C:
        monkeypatch.setenv("RSX_BLIND_MIN_LOG2", "22")
    s = dl.spec_base(spec)
    dev = Dev(s)
    what = dl.spec_id(spec)
    dev.load()
    rsa.radix_sort_inplace_async(dev.src, dev.aux, dtype=spec.dtype, order=spec.order)
    assert torch.equal(dev.src, dev.pristine), what           # sorted input: the keys are where they were
    for p in dl.spec_positions(spec):
        case = dl.descent_case(s, spec.dtype, spec.order, p)
        dev.load(case)
        rsa.reload_env()
        rsa.radix_sort_inplace_async(dev.src, dev.aux, dtype=spec.dtype, order=spec.order)
        assert torch.equal(dev.src, dev.put_together(case.pieces)), (what, p, case.kind, rsa.async_route())   # always in `buf`


@pytest.mark.parametrize("spec", dl.presorted_specs("E-rank-pairs"), ids=dl.spec_id)
def test_e_rank_and_pairs_inplace_async(spec):
    s = dl.spec_base(spec)
    n, dt, order = spec.n, spec.dtype, spec.order
    dev = Dev(s)
    what = dl.spec_id(spec)
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    vals = to_dev(pl.payloads("random", n, 4, seed=n % 1000))
    ib = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    v, vscratch = torch.empty_like(vals), torch.empty_like(vals)

    def run(case):
        dev.load(case)
        ib.fill_(_FILL[4])
        given = dev.src.clone()
        ranks = rsa.radix_sort_rank_inplace_async(dev.src, ib, dtype=dt, order=order)
        assert torch.equal(dev.src, given), what                 # (a rank sort only reads its keys)
        v.copy_(vals)
        rsa.radix_sort_pairs_inplace_async(dev.src, dev.aux, v, vscratch, dtype=dt, order=order)
        return ranks

    ranks = run(None)
    assert torch.equal(ranks, iota), what                                          # sorted input: ranks 0 .. n-1,
    assert torch.equal(dev.src, dev.pristine) and torch.equal(v, vals), what       # keys and payloads unchanged
    for p in dl.spec_positions(spec):
        case = dl.descent_case(s, dt, order, p)
        perm = dev.put_together(dl.rank_pieces(s, dt, order, case), cut=iota)
        ranks = run(case)
        assert torch.equal(ranks, perm), (what, "ranks", p, case.kind)
        assert torch.equal(dev.src, dev.put_together(case.pieces)), (what, "keys", p, case.kind)
        assert torch.equal(v, vals[perm.long()]), (what, "payloads", p, case.kind)


# ---- F: blocking rank and key + payload sorts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", dl.presorted_specs("F"), ids=dl.spec_id)
def test_f_rank_and_pairs_presorted_or_one_descent(spec):
    _rank_and_pairs(spec, spots=2)


# ---- kept columns: one stray key in a constant column ---------------------------------------------------------------------------
def _stray_cases(spec, base, positions, flips, what, before=None, after=None):
    dt, order, n = spec.dtype, spec.order, spec.n
    routes = set()
    base_kept = dl.kept_columns(base, dt, order)
    sb = dl.sort_by_kdf(base, dt, order)
    sk = ol.kdf_keys(sb, dt, order)
    dev = Dev(base, cut_from=sb)
    # the base itself: exactly its own columns (a base of equal keys is sorted: the early exit)
    flat = not base_kept
    dev.load()
    if before is not None:
        before()
    res, info = rsa.radix_sort(dev.src, dev.aux, dtype=dt, order=order)
    assert info.early_exit == (2 if flat else 0) and info.kept_columns() == base_kept, (what, info.early_exit, info.kept_columns())
    assert info.result_in_aux == (0 if flat else len(base_kept) & 1) and torch.equal(res, dev.cut), what
    base_route = int(info.hybrid)
    for column, bit in flips:
        for p in positions:
            case = dl.stray_case(base, sb, dt, order, column, p, bit, sorted_keys=sk)
            if n <= dl.SMALL:
                _, want_aux, want_cols, early = _oracle_decision(dl.apply_patches(base, case), dt, order)
            else:
                want_cols, want_aux, early = dl.stray_decision(base, base_kept, dt, order, column, case)
            if base_kept:
                assert want_cols == sorted(base_kept + [column]) and early == 0
            dev.load(case)
            if before is not None:
                before()
            res, info = rsa.radix_sort(dev.src, dev.aux, dtype=dt, order=order)
            w = (what, "column", column, "bit", bit, "p", p, "route", info.hybrid)
            assert info.early_exit == early, w
            assert info.kept_columns() == want_cols and info.result_in_aux == want_aux, (w, info.kept_columns(), info.result_in_aux)
            assert torch.equal(res, dev.put_together(case.pieces)), w
            routes.add(int(info.hybrid))
            if after is not None:
                after(p, info)
    print("%s: route of the base %d, with a stray key %s" % (what, base_route, sorted(routes)))


def _stray_spec(spec, before=None):
    base = dl.stray_base(spec)
    ps = dl.stray_positions(spec.n, ol.DTYPE_SIZE[spec.dtype], spec.sampled)
    _stray_cases(spec, base, ps, [(c, b) for c in spec.constant for b in dl.STRAY_BITS], dl.stray_id(spec), before=before)


@pytest.mark.parametrize("spec", dl.stray_specs("A"), ids=dl.stray_id)
def test_kept_columns_one_stray_key_small(spec):
    _stray_spec(spec)


@pytest.mark.parametrize("spec", dl.stray_specs("B"), ids=dl.stray_id)
def test_kept_columns_one_stray_key_histogram(spec):
    _stray_spec(spec)


@pytest.mark.parametrize("atoms", [False, True], ids=["chained", "RSX_PASS32_MIN_MI"])
@pytest.mark.parametrize("spec", dl.stray_specs("C"), ids=dl.stray_id)
def test_kept_columns_one_stray_key_sampled(spec, atoms, monkeypatch):
    """A column that is constant in the sample has to be checked on every key (SegCtl::cmask / key0) by the level-1 pass: the
    chained one (rsx_scatter2_kernel) and, with its floor lowered to 4 Mi keys, the one that writes whole atoms
    (rsx_pass32a_kernel).  Only the decision and the result are asserted: whether the attempt is called off or never made is
    the library's business (the routes are printed)."""
    monkeypatch.setenv("RSX_BLIND_MIN_LOG2", "22")
    if atoms:
        monkeypatch.setenv("RSX_PASS32_MIN_MI", "4")
    _stray_spec(spec, before=rsa.reload_env)


@pytest.mark.parametrize("n", dl.N_D)
def test_kept_columns_one_key_above_the_log_routes_window(n, monkeypatch):
    """Zipf-like keys below 2^40 with one key carrying bit 45, 50 or 63: if the sample does not read that key the histogram's OR
    against the first key has to find it (rsx_log_plan_kernel's `inside`), and the route must not be taken either way."""
    monkeypatch.setenv("RSX_LOG_MIN_LOG2", "20")
    base = dl.stray_base_d(n)
    spec = dl.StraySpec(ol.U64, ol.ASC, n, (5, 6, 7), True)

    def after(p, info):
        if p != 0:
            assert info.hybrid != LOG_ROUTE, (n, p, info.hybrid)

    _stray_cases(spec, base, dl.stray_positions(n, 8, True), [(b // 8, b % 8) for b in dl.STRAY_BITS_D], "D n=%d" % n,
                 before=rsa.reload_env, after=after)
