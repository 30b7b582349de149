"""feature_fuzz_lib without a GPU: the generator is deterministic, the default run (default seed, default chunks) covers what the
fuzz is for -- every feature with every dtype in both orders, every switch value, every output subset, both index widths, stream
kinds and forms, every reachable route as the one route the rule allows --, the comparison the GPU test uses accepts the reference
and refuses every wrong answer, and the references of a chunk stay within their CPU time."""
import collections
import time

import numpy as np
import pytest

import feature_fuzz_lib as fz
import oracle_lib as ol



class Walk:
    """One pass over the default run, so that every input and every reference is made once: the cases, their expected routes, the
    CPU time of each chunk's references, and what the comparison said to the reference's own answer and to every wrong one."""

    def __init__(self):
        self.run, self.routes, self.seconds = [], [], []
        self.applied, self.failures = collections.Counter(), []
        for chunk in range(fz.DEFAULT_CHUNKS):
            spent = 0.0
            for i, c in enumerate(fz.cases(fz.DEFAULT_SEED, chunk)):
                inp = fz.inputs(c)
                self.run.append((chunk, i, c))
                self.routes.append(fz.expected_routes(c, inp))
                t0 = time.process_time()
                want = fz.reference(c, inp)
                spent += time.process_time() - t0
                where = fz.tag(c, fz.DEFAULT_SEED, chunk, i)
                bad = fz.mismatches(c, fz.clean_answer(c, want), want)
                if bad:
                    self.failures.append(("the reference's own answer is refused", bad, where))
                for wrong in fz.WRONG:
                    got = wrong(c, inp, want)
                    if got is None:
                        continue
                    self.applied[(c.feature, wrong.__name__)] += 1
                    if not fz.mismatches(c, got, want):
                        self.failures.append((wrong.__name__ + " is accepted", where))
            self.seconds.append(spent)


@pytest.fixture(scope="module")
def walk():
    return Walk()


@pytest.fixture(scope="module")
def default_run(walk):
    return walk.run, walk.routes


def test_cases_are_deterministic():
    for chunk in (0, 3):
        a, b = fz.cases(fz.DEFAULT_SEED, chunk), fz.cases(fz.DEFAULT_SEED, chunk)
        assert a == b and len(a) == fz.CASES_PER_CHUNK
        for x, y in list(zip(a, b))[:22]:
            ix, iy = fz.inputs(x), fz.inputs(y)
            assert sorted(ix) == sorted(iy)
            for name in ix:
                vx, vy = ix[name], iy[name]
                if isinstance(vx, list):
                    assert len(vx) == len(vy) and all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(vx, vy)), fz.describe(x)
                elif isinstance(vx, np.ndarray):
                    assert vx.dtype == vy.dtype and vx.tobytes() == vy.tobytes(), (name, fz.describe(x))
                else:
                    assert vx == vy, (name, fz.describe(x))
    assert fz.cases(fz.DEFAULT_SEED, 0) != fz.cases(fz.DEFAULT_SEED, 1)
    assert fz.cases(fz.DEFAULT_SEED, 0) != fz.cases(fz.DEFAULT_SEED + 1, 0)


def test_describe_names_every_field():
    c = fz.cases(fz.DEFAULT_SEED, 0)[5]
    text = fz.describe(c)
    for part in (c.feature, ol.DTYPE_NAMES[c.dt], "n=%d" % c.n, "style=%d" % c.style, "seed=%d" % c.seed, "idx=%d" % c.idx_bytes,
                 "stream=" + c.stream, "form=" + c.form, "params=", "outputs=", "switches=", "asc" if c.order == 0 else "desc"):
        assert part in text, (part, text)
    assert "\n" not in text
    assert "RSX_FUZZ_SEED=7 RSX_FUZZ_CASE=2:5" in fz.tag(c, 7, 2, 5)


def test_sizes_and_forms_follow_the_rules(default_run):
    run, _ = default_run
    cases = [c for _, _, c in run]
    assert all(0 <= c.n <= fz.max_n() for c in cases)
    assert all(c.n <= fz.HOST_MAXN and c.stream == "default" for c in cases if c.form == "host")
    tiny = [c for c in cases if c.n < 2]
    assert len(cases) // 40 <= len(tiny) <= len(cases) // 12, len(tiny)        # "one case in about thirty"
    assert {c.n for c in tiny} == {0, 1}
    hosts = sum(c.form == "host" for c in cases)
    assert len(cases) // 16 <= hosts <= len(cases) // 5, hosts                   # "about one case in eight"
    small = sum(2 <= c.n <= 3000 for c in cases)
    assert small >= len(cases) // 5, small


def test_every_feature_meets_every_dtype_in_both_orders(default_run):
    run, _ = default_run
    seen = {(c.feature, c.dt, c.order) for _, _, c in run}
    missing = [(f, ol.DTYPE_NAMES[dt], order) for f in fz.FEATURES for dt in range(10) for order in (0, 1) if (f, dt, order) not in seen]
    assert not missing, missing
    # reduce: each of the six value types, integer values of full range and both kinds of float values
    vals = {(c.params["val_dt"], c.params["vals"]) for _, _, c in run if c.feature == "reduce"}
    assert {v for v, _ in vals} == set(range(10)) & {ol.U32, ol.I32, ol.F32, ol.U64, ol.I64, ol.F64}
    assert {k for v, k in vals if v in (ol.F32, ol.F64)} == {"small_ints", "general"}
    # lex: 1 to 5 columns, a repeated column, every packing
    lex = [c for _, _, c in run if c.feature == "lex"]
    assert {len(c.params["cols"]) for c in lex} == {1, 2, 3, 4, 5}
    assert any(len({s for _, _, s in c.params["cols"]}) < len(c.params["cols"]) for c in lex)


def test_every_switch_value_and_every_output_subset_occurs(default_run):
    run, _ = default_run
    for f in fz.FEATURES:
        mine = [c for _, _, c in run if c.feature == f]
        for name, values in fz.SWITCHES[f].items():
            seen = {c.switches.get(name, "") for c in mine}
            for v in values:
                if v == "small":
                    assert any(s not in ("", "0") for s in seen), (f, name)
                else:
                    assert v in seen, (f, name, v, seen)
        assert {tuple(c.outputs) for c in mine} == set(fz.SUBSETS[f]), (f, set(fz.SUBSETS[f]) - {tuple(c.outputs) for c in mine})
        assert {c.idx_bytes for c in mine} == {4, 8}, f
        assert {c.stream for c in mine} == {"default", "side"}, f
        assert {c.form for c in mine} == {"device", "host"}, f
        assert all(set(c.switches) <= set(fz.ENV_NAMES) for c in mine)
    # the flags and parameter values the issue lists
    by = lambda f: [c for _, _, c in run if c.feature == f]
    assert {c.params["below"] for c in by("locate")} == {0, 1} and {c.params["below"] for c in by("partition")} == {0, 1}
    assert {c.params["how"] for c in by("join")} == {"inner", "left"}
    assert {c.params["local"] for c in by("segments")} == {0, 1} and {bool(c.params["rows"]) for c in by("segments")} == {False, True}
    assert {c.params["k_kind"] for c in by("topk")} >= {"one", "two", "draw", "tie", "n-1", "n"}
    assert min(c.params["m"] for c in by("nth")) == 1 and max(c.params["m"] for c in by("nth")) == 70
    assert min(c.params["m"] for c in by("locate")) == 0 and max(c.params["m"] for c in by("locate")) > 4096
    assert min(c.params["m"] for c in by("partition")) == 0 and max(c.params["m"] for c in by("partition")) > 255
    # the subsets as the issue words them
    assert len(fz.SUBSETS["rankdata"]) == 7 and len(fz.SUBSETS["locate"]) == 7 and len(fz.SUBSETS["join"]) == 7
    assert len(set(fz.SUBSETS["group"])) == 15 and len(set(fz.SUBSETS["partition"])) == 6
    ops = {tuple(n for n in s if n in ("sum", "min", "max")) for s in fz.SUBSETS["reduce"]}
    assert len(ops) == 8
    for name in ("keys", "counts"):
        assert {name in s for s in fz.SUBSETS["reduce"]} == {False, True}
    # every key style occurs, the few-bits classes and the specials with every feature they can tell something about
    assert {c.style for _, _, c in run} == set(range(len(fz.STYLE_NAMES)))


def test_every_route_is_the_only_one_allowed_for_two_cases(default_run):
    run, routes = default_run
    single = collections.Counter()
    for (_, _, c), r in zip(run, routes):
        if r is not None:
            assert r and r <= set(fz.ROUTES[c.feature]), (r, fz.describe(c))
            if len(r) == 1:
                single[(c.feature, next(iter(r)))] += 1
    thin = {(f, r): single[(f, r)] for f in fz.FEATURES for r in fz.ROUTES[f] if (f, r) not in fz.EXEMPT and single[(f, r)] < 2}
    assert not thin, thin
    for (f, r), reason in fz.EXEMPT.items():
        assert r in fz.ROUTES[f] and reason
    none = sum(r is None for r in routes)
    print("cases without an expected route: %d of %d" % (none, len(routes)))
    assert 3 * none <= len(routes), (none, len(routes))


def test_the_comparison_accepts_the_reference_and_refuses_every_wrong_answer(walk):
    """Over the default run: the reference's own answer passes, every wrong answer built from it is refused (by mismatches, which
    is all check() asserts), every generator applies to some case and every feature has at least two of its own that apply."""
    assert not walk.failures, walk.failures[:5]
    for wrong in fz.WRONG:
        assert any(walk.applied[(f, wrong.__name__)] for f in fz.FEATURES), wrong.__name__
    for f in fz.FEATURES:
        mine = [w.__name__ for w in fz.WRONG if walk.applied[(f, w.__name__)] and w not in (fz.wrong_tail_written, fz.wrong_input_written)]
        assert len(mine) >= 2, (f, mine)
    c = walk.run[0][2]
    inp = fz.inputs(c)
    want = fz.reference(c, inp)
    fz.check(c, fz.clean_answer(c, want), want)
    with pytest.raises(AssertionError, match="tails"):
        fz.check(c, fz.wrong_tail_written(c, inp, want), want, "somewhere")


def test_general_float_sums_are_compared_within_the_derived_bound_only():
    """reduce's one exception: a sum inside reduce_lib.fsum_bound of math.fsum passes, one outside it does not, and with
    rl.small_ints values a single bit off is refused."""
    found = set()
    for chunk in range(fz.DEFAULT_CHUNKS):
        for c in fz.cases(fz.DEFAULT_SEED, chunk):
            if c.feature != "reduce" or "sum" not in c.outputs or c.params["val_dt"] not in (ol.F32, ol.F64) or c.n < 100:
                continue
            if c.params["vals"] in found:
                continue
            found.add(c.params["vals"])
            inp = fz.inputs(c)
            want = fz.reference(c, inp)
            got = fz.clean_answer(c, want)
            s = want["sum"].view(np.float64)
            if c.params["vals"] == "general":
                j = int(np.argmax(want["sum_bound"]))
                assert want["sum_bound"][j] > 0
                inside, outside = s.copy(), s.copy()
                inside[j] += 0.5 * want["sum_bound"][j]
                outside[j] += 4.0 * want["sum_bound"][j] + abs(s[j]) * 2.0 ** -40
                assert not fz.mismatches(c, dict(got, sum=inside.view(np.uint64)), want)
                assert fz.mismatches(c, dict(got, sum=outside.view(np.uint64)), want)
            else:
                assert "sum_bound" not in want
                off = want["sum"].copy()
                off[0] ^= np.uint64(1)
                assert fz.mismatches(c, dict(got, sum=off), want) == ["sum"]
        if len(found) == 2:
            break
    assert found == {"general", "small_ints"}


def test_reference_cost(walk):
    """The references of every chunk of the default run, timed on this core (process time): printed, not asserted -- the number
    beside feature_fuzz_lib.CASES_PER_CHUNK is the largest of them."""
    print("references of the most expensive default chunk: %.2f s for %d cases (all chunks: %s)" % (
        max(walk.seconds), fz.CASES_PER_CHUNK, " ".join("%.2f" % t for t in walk.seconds)))
