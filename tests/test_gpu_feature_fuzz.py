"""Seeded differential fuzz of the eleven feature entry points (feature_fuzz_lib): every dimension of a call drawn jointly --
feature, dtype, order, n, key style, parameters, wanted outputs, index width, route switches, stream, device or host form -- and
every wanted output compared bit for bit with the oracle-derived reference (reduce's general float sums within reduce_lib.fsum_bound);
inputs unchanged, guards and tails untouched, the route one of those include/rsx.h's rule allows.

The cases of a chunk run back to back on one context (and one side stream), so the fuzz also walks random pairs of features.
RSX_FUZZ_CHUNKS / RSX_FUZZ_SEED (test_gpu_fuzz.py's): a longer or a different run; RSX_FUZZ_CASE=chunk:case: that case alone, as a
failure names it."""
import collections
import os

import numpy as np
import pytest

import feature_fuzz_lib as fz
import join_lib as jl
import lex_lib
import locate_lib as ll
import nth_lib as nl
import oracle_lib as ol
import partition_lib as pl
import radix_sorting_amd as rsa
import segments_lib as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_CHUNKS = int(os.environ.get("RSX_FUZZ_CHUNKS", str(fz.DEFAULT_CHUNKS)))
_SEED = int(os.environ.get("RSX_FUZZ_SEED", str(fz.DEFAULT_SEED)))
_ONLY = tuple(int(x) for x in os.environ["RSX_FUZZ_CASE"].split(":")) if os.environ.get("RSX_FUZZ_CASE") else None

CENSUS = collections.Counter()      # (feature, switches, observed route) -> cases; printed, asserted only through expected_routes


def _clear(monkeypatch):
    for name in fz.ENV_NAMES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    _clear(monkeypatch)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    _clear(monkeypatch)
    rsa.reload_env()


def _info_checks(case, inp, want, got, info, where):
    """What the features' own libs assert of the info beside the outputs (their check() functions on what the call delivered)."""
    f, o = case.feature, (lambda name: got.get(name) if name in case.outputs else None)
    if f == "topk" and inp["k"]:
        kb = ol.DTYPE_SIZE[case.dt]
        assert info.key_bytes == kb and info.n_less < inp["k"] <= info.n_less + info.n_equal, where
        if info.route == rsa.TOPK_SELECT:
            assert 1 <= info.input_reads <= kb + 1 and info.digit_passes == kb, (where, info.input_reads, info.digit_passes)
        else:
            assert info.input_reads == 0 and info.digit_passes == 0, where
    elif f == "nth" and inp["ranks"].size and case.n >= 2:
        nl.check(where, want["_want"], inp["ranks"], o("keys"), o("idx"), got["n_less"], got["n_equal"], info)
    elif f == "locate" and info.route != rsa.LOCATE_TRIVIAL:
        ll.check(where, want["_want"], inp["vals"], None, None, o("less"), o("equal"), o("bins"), bool(case.params["below"]), info)
    elif f == "partition" and info.route != rsa.PARTITION_TRIVIAL:
        seam = int(case.switches.get("RSX_PARTITION_BALLOT_PARTS", pl.BALLOT_PARTS))
        pl.check(where, want["_want"], inp["edges"], None, None, o("keys"), o("idx"), o("offsets"), bool(case.params["below"]), info, seam=seam)
    elif f == "segments":
        sg.check(where, want["_want"], None, None, o("keys"), o("idx"), bool(case.params["local"]), info)
    elif f == "join":
        jl.check(where, want["_want"], o("start"), o("count"), o("right_perm"), got["n_pairs"], info, case.params["how"] == "left")
    elif f == "lex" and case.n >= 2:
        limit = int(case.switches.get("RSX_LEX_PACK_BYTES", 4))
        dtypes = [c[0] for c in case.params["cols"]]
        assert info.pack_bytes == limit and info.ncols == len(dtypes), where
        assert info.groups() == lex_lib.want_groups(dtypes, limit), (where, info.groups())


def _one(case, where, session, monkeypatch):
    torch.cuda.synchronize()
    _clear(monkeypatch)
    for name, value in case.switches.items():
        monkeypatch.setenv(name, value)
    rsa.reload_env()
    inp = fz.inputs(case)
    want = fz.reference(case, inp)
    try:
        got, mem, info = fz.run(case, inp, session)
    except (rsa.RsxError, AssertionError) as e:       # (every case is a valid call: anything but RSX_OK is a finding)
        raise AssertionError("%s: %s" % (where, e)) from e
    fz.check(case, got, want, where)
    try:
        mem.check_guards()
    except AssertionError as e:
        raise AssertionError("%s: %s" % (where, e)) from e
    routes = fz.expected_routes(case, inp)
    drawn = ("RSX_LOCATE_MAX_VALUES",)      # (a small draw: one line for all of them)
    CENSUS[(case.feature, tuple(sorted((k, "k" if k in drawn else v) for k, v in case.switches.items())), got["route"])] += 1
    if routes is not None:
        assert got["route"] in routes, "%s: route %s, the rule allows %s" % (where, got["route"], sorted(routes))
    _info_checks(case, inp, want, got, info, where)


@pytest.mark.parametrize("chunk", range(_CHUNKS))
def test_fuzz_features(chunk, monkeypatch):
    rsa.require_gpu()
    session = fz.Session()
    try:
        for number, case in enumerate(fz.cases(_SEED, chunk)):
            if _ONLY is not None and _ONLY != (chunk, number):
                continue
            _one(case, fz.tag(case, _SEED, chunk, number), session, monkeypatch)
    finally:
        session.close()
    if chunk == _CHUNKS - 1:
        print("\nroute census (feature, switches, observed route): cases")
        for (feature, switches, route), count in sorted(CENSUS.items(), key=lambda kv: (kv[0][0], kv[0][1], str(kv[0][2]))):
            print("  %-9s %-70s route %s: %d" % (feature, " ".join("%s=%s" % kv for kv in switches) or "-", route, count))
