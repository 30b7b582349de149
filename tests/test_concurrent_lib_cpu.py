"""concurrent_lib without a GPU: run_threads really surfaces what a worker raises (with the worker's name) and tells a hung
worker from a failed one and from one that passed, overlaps() counts hand-made intervals, the work lists are what the GPU test
needs them to be, and the checks made after the join refuse another worker's answer."""
import threading
import time

import pytest

import concurrent_lib as cl
import inner_lib as il
import seq_lib as sq


# ---- run_threads --------------------------------------------------------------------------------------------------------------
def test_return_values_come_back_in_order():
    got = cl.run_threads([("w%d" % i, (lambda i=i: (time.sleep(0.01 * (3 - i)), i * i)[1])) for i in range(4)], 5.0)
    assert got == [0, 1, 4, 9]


def test_workers_start_together_and_carry_their_names():
    seen, lock = {}, threading.Lock()

    def worker():
        with lock:
            seen[threading.current_thread().name] = time.perf_counter()
        time.sleep(0.02)

    cl.run_threads([(name, worker) for name in ("a", "b", "c")], 5.0)
    assert sorted(seen) == ["a", "b", "c"]
    assert max(seen.values()) - min(seen.values()) < 0.5, "the barrier did not release the workers together"


def _raises():
    raise ValueError("sorted wrongly at 17")


def test_an_exception_surfaces_with_the_workers_name_and_traceback():
    with pytest.raises(cl.WorkerFailed) as e:
        cl.run_threads([("good", lambda: time.sleep(0.01)), ("bad one", _raises), ("other", lambda: 3)], 5.0)
    text = str(e.value)
    assert "worker bad one raised ValueError: sorted wrongly at 17" in text
    assert "_raises" in text, "the worker's traceback is part of the message"
    assert isinstance(e.value.__cause__, ValueError)
    by_name = {o.name: o for o in e.value.outcomes}
    assert by_name["other"].value == 3 and by_name["good"].error is None and not by_name["bad one"].hung


def test_the_first_exception_is_the_one_raised():
    def late():
        time.sleep(0.05)
        raise KeyError("second")

    with pytest.raises(cl.WorkerFailed) as e:
        cl.run_threads([("w0", lambda: None), ("w1", _raises), ("w2", late)], 5.0)
    assert "worker w1 raised ValueError" in str(e.value)
    assert sum(o.error is not None for o in e.value.outcomes) == 2


def test_an_assertion_in_a_worker_is_not_swallowed():
    def worker():
        assert 1 + 1 == 3, "checked in the thread"

    with pytest.raises(AssertionError, match="worker w raised AssertionError: checked in the thread"):
        cl.run_threads([("w", worker)], 5.0)


def test_a_hung_worker_is_reported_as_hung_not_as_passed_or_failed():
    release = threading.Event()
    try:
        t0 = time.monotonic()
        with pytest.raises(cl.Hung) as e:
            cl.run_threads([("quick", lambda: 1), ("stuck", lambda: release.wait(30.0))], 0.2)
        assert time.monotonic() - t0 < 5.0, "the join did not give up at the limit"
        assert e.value.names == ["stuck"] and "stuck" in str(e.value) and "hung" in str(e.value)
        assert not isinstance(e.value, cl.WorkerFailed)
        by_name = {o.name: o for o in e.value.outcomes}
        assert by_name["stuck"].hung and by_name["quick"].value == 1 and not by_name["quick"].hung
    finally:
        release.set()


def test_hung_wins_over_a_failure_and_still_names_it():
    release = threading.Event()
    try:
        with pytest.raises(cl.Hung) as e:
            cl.run_threads([("bad", _raises), ("stuck", lambda: release.wait(30.0))], 0.2)
        assert e.value.names == ["stuck"] and "worker bad failed" in str(e.value)
    finally:
        release.set()


def test_the_limit_runs_from_the_release_for_all_workers_at_once():
    """Three stuck workers cost one limit, not three: the joins share one deadline."""
    release = threading.Event()
    try:
        t0 = time.monotonic()
        with pytest.raises(cl.Hung) as e:
            cl.run_threads([("s%d" % i, lambda: release.wait(30.0)) for i in range(3)], 0.3)
        assert time.monotonic() - t0 < 0.8 and e.value.names == ["s0", "s1", "s2"]
    finally:
        release.set()


# ---- Timeline and overlaps ------------------------------------------------------------------------------------------------------
def _timeline(**calls):
    t = cl.Timeline()
    for worker, ivs in calls.items():
        for a, b in ivs:
            t.add(worker, a, b)
    return t


def test_overlaps_of_hand_made_intervals():
    assert cl.overlaps(_timeline(a=[(0, 10)], b=[(20, 30)])) == {"a": 0, "b": 0}                       # disjoint
    assert cl.overlaps(_timeline(a=[(0, 100)], b=[(20, 30), (40, 50)])) == {"a": 1, "b": 2}             # nested
    assert cl.overlaps(_timeline(a=[(0, 10)], b=[(10, 20)])) == {"a": 0, "b": 0}                        # touching end to start
    assert cl.overlaps(_timeline(a=[(0, 10), (5, 20), (30, 40)])) == {"a": 0}                           # a single worker
    assert cl.overlaps(_timeline(a=[(0, 10), (30, 40)], b=[(9, 11)], c=[(35, 36), (50, 60)])) == {"a": 2, "b": 1, "c": 1}
    assert cl.overlaps(_timeline(a=[(5, 5)], b=[(0, 10)])) == {"a": 1, "b": 1}                          # an instant inside a call
    assert cl.overlaps(cl.Timeline()) == {}


def test_timeline_stamps_calls_per_thread():
    t = cl.Timeline()

    def worker():
        for _ in range(2):
            t.call(time.sleep, 0.05, label="sleep")
        return t.call(lambda x, y=0: x + y, 2, y=3)

    assert cl.run_threads([("a", worker), ("b", worker)], 5.0) == [5, 5]
    assert sorted(t.calls) == ["a", "b"] and all(len(v) == 3 for v in t.calls.values())
    for ivs in t.calls.values():
        assert all(b1 >= b0 for b0, b1, _ in ivs) and ivs[0][1] - ivs[0][0] >= 40e6 and ivs[0][2] == "sleep"
    assert all(c >= 2 for c in cl.overlaps(t).values()), "two workers that sleep at the same time overlap"


def test_timeline_stamps_a_call_that_raises():
    t = cl.Timeline()
    with pytest.raises(ValueError):
        t.call(_raises, worker="w")
    assert len(t.calls["w"]) == 1


# ---- the work lists ---------------------------------------------------------------------------------------------------------------
def test_work_lists_cover_the_kinds_and_differ():
    lists = cl.sort_lists()
    assert lists == cl.sort_lists() and len(lists) == 4 and all(len(steps) == 10 for steps in lists)
    kinds = {s.kind for steps in lists for s in steps}
    assert kinds == set(sq.KINDS) - {"host"}
    assert [s.kind for s in lists[0]].count("replay") == 3 and all(s.kind != "replay" for steps in lists[1:] for s in steps)
    assert [s.n for steps in lists for s in steps if s.kind == "keys_nohist"] == [il.N23]
    assert {s.seed % 2 for steps in lists for s in steps if s.kind == "sub_async"} == {0, 1}
    assert len({tuple(steps) for steps in lists}) == 4
    assert len({s.seed for steps in lists for s in steps}) == 40, "no two steps share their input"
    for steps in lists:
        assert any(a.n < b.n and a.kind != "replay" != b.kind for a, b in zip(steps, steps[1:])), "a pair of sizes that grows"
    for steps in lists:
        for s in steps:
            lo, _, dts = sq.SPEC[s.kind]
            assert s.dt in dts and s.n >= lo, s


def test_the_checks_after_the_join_refuse_another_workers_answer():
    """Had concurrency mixed up two contexts' outputs, worker v's step would hold worker w's result.  For every position of the
    lists: the reference's own answer to worker w's step (in the form run() reports) is accepted for that step and refused for
    the step at the same position of the next worker.  (Steps above 100 001 keys are left out to keep this quick; a refused call
    has no data, so where both steps are refusals there is nothing to tell apart.)"""
    lists = cl.sort_lists()
    told = 0
    for w, steps in enumerate(lists):
        for mine, theirs in zip(steps, lists[(w + 1) % 4]):
            if max(mine.n, theirs.n) > 100001 or mine.kind == theirs.kind == "refused":
                continue
            got = sq.clean_answer(mine, sq.expect(mine))
            assert sq.mismatches(mine, got) == []
            assert sq.mismatches(theirs, got), (sq.describe(mine), "passes for", sq.describe(theirs))
            with pytest.raises(AssertionError, match="wrong after"):
                sq.check(theirs, got)
            told += 1
    assert told >= 24


def test_a_stale_answer_is_refused_as_in_the_sequences():
    """... and a worker's own previous result presented as its next one is refused as seq_lib.WRONG has it."""
    steps = [s for s in cl.sort_lists()[3] if s.n <= 100001]
    wrongs = 0
    for prev, step in zip(steps, steps[1:]):
        want, prev_want = sq.expect(step), sq.expect(prev)
        for make in sq.WRONG:
            got = make(step, want, prev, prev_want)
            if got is not None:
                assert sq.mismatches(step, got, want), (make.__name__, sq.describe(step))
                wrongs += 1
    assert wrongs >= 8
