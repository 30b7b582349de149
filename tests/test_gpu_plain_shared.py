"""What the drivers of the three plain sorts share (csrc/rsx_sort_plain.hpp, rsx_sort_async.hpp), where a slip would stay silent.

A. The RSX_VERIFY=2 bracket, one function under sort_keys_device, sort_pairs_device and sort_rank_device: with
   RSX_VERIFY_INJECT=1 every kind must fail with RSX_EVERIFY in its OWN words (key mix / pair mix / rank mix -- whole sentences
   are matched), and pass with the switch off on the same input, on the one-launch sort and on the first size past it
   (SMALL_SORT_BYTES / SMALL_PAIR_BYTES are read from csrc/rsx_small.hpp).  Ranks of one key are not bracketed at all.
B. The gate of a device-scheduled sort (Ctx::pass_gate) is cleared when the launches behind an attempt return an error: the
   next blocking sort of the context must not look at a verdict.
"""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


def _small_bytes(name):
    src = open(os.path.join(ROOT, "radix_sorting_amd", "csrc", "rsx_small.hpp")).read()
    return int(re.search(r"constexpr u32 %s = (\d+);" % name, src).group(1))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


# ---- A. RSX_VERIFY=2 with RSX_VERIFY_INJECT=1 ----------------------------------------------------------------------------------
def _keys(a):
    res, _ = rsa.radix_sort(_dev(a), torch.zeros(a.size, dtype=torch.int32, device="cuda"), dtype=rsa.U32)
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy().view(np.uint32), ol.oracle_sort(a, ol.U32)[0])


def _pairs(a):
    vals = (np.arange(a.size, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x80000001)     # (every bit used, not the position)
    kr, vr, _ = rsa.radix_sort_pairs(_dev(a), torch.zeros(a.size, dtype=torch.int32, device="cuda"), _dev(vals),
                                     torch.zeros(a.size, dtype=torch.int32, device="cuda"), dtype=rsa.U32)
    torch.cuda.synchronize()
    order = np.argsort(a, kind="stable")
    assert np.array_equal(kr.cpu().numpy().view(np.uint32), a[order]) and np.array_equal(vr.cpu().numpy().view(np.uint32), vals[order])


def _ranks(a):
    ranks, info = rsa.radix_sort_rank(_dev(a), torch.zeros(2 * a.size, dtype=torch.int32, device="cuda"), dtype=rsa.U32)
    torch.cuda.synchronize()
    want, half, _, _ = ol.oracle_rank(a, ol.U32, 4)
    assert info.result_in_aux == half and np.array_equal(ranks.cpu().numpy().view(np.uint32), want)


_KINDS = {
    # kind: (the call, SMALL_* that bounds its one-launch sort, bytes per element in that bound, the report with inject on)
    "keys": (_keys, "SMALL_SORT_BYTES", 4,
             r"rsx error -5: RSX_VERIFY=2: the result of a sort of %d keys \(route \d+\) is not a permutation of the input: "
             r"0 descents, key sum kept, key mix changed$"),
    "pairs": (_pairs, "SMALL_PAIR_BYTES", 2 * (4 + 4),
              r"rsx error -5: RSX_VERIFY=2: the result of a key \+ payload sort of %d pairs \(route \d+\) is not a permutation of the "
              r"input's pairs: 0 descents, key sum kept, pair mix changed$"),
    "ranks": (_ranks, "SMALL_PAIR_BYTES", 2 * (4 + 4),
              r"rsx error -5: RSX_VERIFY=2: the ranks of a sort of %d keys \(route \d+\) are not a permutation of 0 \.\. n-1: "
              r"0 places out of order, rank sum right, rank mix wrong$"),
}


@pytest.mark.parametrize("size", ["one-launch", "past-one-launch"])
@pytest.mark.parametrize("kind", ["keys", "pairs", "ranks"])
def test_whole_sort_check_reports_in_its_kinds_words(kind, size, monkeypatch):
    call, bound, per_elem, report = _KINDS[kind]
    n = 300 if size == "one-launch" else _small_bytes(bound) // per_elem + 1
    a = ol.splitmix_fill(n, ol.U32, 9100 + n, 0xFFFFFFFF)
    monkeypatch.setenv("RSX_VERIFY", "2")
    call(a)                                              # inject off: the bracket runs and finds nothing
    monkeypatch.setenv("RSX_VERIFY_INJECT", "1")
    with pytest.raises(rsa.RsxError, match=report % n) as err:
        call(a)
    assert "%s mix" % {"keys": "key", "pairs": "pair", "ranks": "rank"}[kind] in str(err.value)
    monkeypatch.delenv("RSX_VERIFY_INJECT")
    call(a)                                              # ... and off again, on the same input


def test_ranks_of_one_key_are_not_bracketed(monkeypatch):
    monkeypatch.setenv("RSX_VERIFY", "2")
    monkeypatch.setenv("RSX_VERIFY_INJECT", "1")
    ib = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    ranks, info = rsa.radix_sort_rank(_dev(np.array([5], dtype=np.uint32)), ib, dtype=rsa.U32)
    torch.cuda.synchronize()
    assert info.early_exit == 1 and ranks.cpu().numpy().tolist() == [0]


# ---- B. the gate after a failing gated body -------------------------------------------------------------------------------------
def test_gate_is_cleared_when_the_gated_launches_fail():
    """A context of its own (a new stream) whose only sort so far went without a histogram: it has the slots of an attempt but no
    status words.  A device-scheduled sort of the same keys under a stream capture then enqueues its attempt and is refused behind
    it, where the status words would have to grow (DevBuf::ensure: nothing grows under a capture) -- inside the gated launches.
    The capture is never replayed.  rsx_async_route says 5 exactly if the attempt was enqueued (the control block still holds the
    blocking sort's verdict); a gate left standing would make the next blocking sort's passes read that verdict and do nothing."""
    rsa.reload_env()
    n = 10 * MI + 3     # (past the floor of a device-scheduled attempt on 4-byte keys, 9 Mi: async_blind_ok)
    a = ol.splitmix_fill(n, ol.U32, 9200, 0xFFFFFFFF)
    s = torch.cuda.Stream()
    src, aux = _dev(a), torch.zeros(n, dtype=torch.int32, device="cuda")
    buf, scratch = _dev(a), torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res, info = rsa.radix_sort(src, aux, dtype=rsa.U32, stream=s)
    s.synchronize()
    assert info.hybrid == 5, info.hybrid
    assert np.array_equal(res.cpu().numpy().view(np.uint32), ol.oracle_sort(a, ol.U32)[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with pytest.raises(rsa.RsxError, match="would have to grow"):
            rsa.radix_sort_inplace_async(buf, scratch, dtype=rsa.U32, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert rsa.async_route(s) == 5     # the attempt was enqueued: the refusal came from behind it
    b = ol.splitmix_fill(300001, ol.U32, 9201, 0xFF00FFFF)
    bsrc, baux = _dev(b), torch.zeros(b.size, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res, info = rsa.radix_sort(bsrc, baux, dtype=rsa.U32, stream=s)
    s.synchronize()
    want, want_aux, _ = ol.oracle_sort(b, ol.U32)
    assert info.result_in_aux == want_aux and np.array_equal(res.cpu().numpy().view(np.uint32), want)
    rsa.release_stream(s)
