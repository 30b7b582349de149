"""The sample in front of rsx_sort_unique_device, rsx_sort_group_device and rsx_sort_rankdata_device, on both sides of each
feature's limit.

At the sizes where the ordinary sort would go without a histogram, the three drivers look at a sample of the keys first: it can
only prove that many bits vary, and where that is more than the largest bitmap or table of the call takes, the keys go to the
sort before any plan.  The limit is the one thing the three set differently (the outputs asked for and the feature's switch decide
it), so every row below is one side of one limit.  What shows is the info struct: varying_bits == 0 together with the SORT route
says the sample sent the keys away; else the plan ran and varying_bits is the popcount of the mask.

2^22 keys with RSX_BLIND_MIN_LOG2=22: the smallest size at which the sample is taken.  A sample of 4096 evenly spread keys misses
one of k varying bits with a probability of about 2^-4095, and the seeds are fixed.  Two-byte keys are never sampled: their
varying_bits are 16 whatever the limit.  Results are checked with what each feature's own test file uses.
"""
import functools

import numpy as np
import pytest

import group_lib as gr
import oracle_lib as ol
import radix_sorting_amd as rsa
import rankdata_lib as rl
import test_gpu_group as tg
import test_gpu_rankdata as tr
import test_gpu_unique as tu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 1 << 22
PLACE, LESS = (True, False, False), (False, True, False)
M24, M25 = 0x00FFFFFF, 0x01FFFFFF


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _sample_from_4mi_keys(monkeypatch):
    monkeypatch.setenv("RSX_BLIND_MIN_LOG2", "22")
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def keys(dt, mask):
    a = ol.splitmix_fill(N, dt, 9100 + bin(mask).count("1"), mask)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_group(dt, mask):
    return gr.want_group(keys(dt, mask), dt, ol.ASC)


@functools.lru_cache(maxsize=None)
def want_rankdata(dt, mask):
    return rl.want_rankdata(keys(dt, mask), dt, ol.ASC)


def seen(info, route, vbits, names):
    return "route %s (expected %s), varying_bits %d (expected %d)" % (names.get(info.route), names[route], info.varying_bits, vbits)


# (name, dtype, mask, count_bytes, switch or None, route, varying bits)
UNIQUE = [
    ("v24", ol.U32, M24, 0, None, rsa.UNIQUE_BITMAP_GLOBAL, 24),
    ("v25", ol.U32, M25, 0, None, rsa.UNIQUE_SORT, 0),
    ("counts-v8", ol.U32, 0x00FF0000, 4, None, rsa.UNIQUE_TABLE, 8),
    ("counts-v9", ol.U32, 0x01FF0000, 4, None, rsa.UNIQUE_SORT, 0),
    ("max-bits-0-v8", ol.U32, 0x00FF0000, 0, ("RSX_UNIQUE_MAX_BITS", "0"), rsa.UNIQUE_SORT, 0),
    ("u64-v24", ol.U64, M24 << 20, 0, None, rsa.UNIQUE_BITMAP_GLOBAL, 24),
    ("u64-v25", ol.U64, M25 << 20, 0, None, rsa.UNIQUE_SORT, 0),
    ("u16-full", ol.U16, 0xFFFF, 0, None, rsa.UNIQUE_BITMAP_LDS, 16),
    ("u16-full-counts", ol.U16, 0xFFFF, 4, None, rsa.UNIQUE_TABLE, 16),
]


@pytest.mark.parametrize("case", UNIQUE, ids=[c[0] for c in UNIQUE])
def test_unique(case, monkeypatch):
    name, dt, mask, cb, switch, route, vbits = case
    if switch:
        monkeypatch.setenv(*switch)
    _, _, info = tu.check(keys(dt, mask), dt, count_bytes=cb, what=name)
    print(name, seen(info, route, vbits, tu.ROUTE))
    assert info.route == route and info.varying_bits == vbits, seen(info, route, vbits, tu.ROUTE)


# (name, dtype, mask, counts, first, route, varying bits): the inverse is always asked for, the keys never
GROUP = [
    ("v24", ol.U32, M24, False, False, rsa.GROUP_RANK_GLOBAL, 24),
    ("v25", ol.U32, M25, False, False, rsa.GROUP_SORT, 0),
    ("counts-v8", ol.U32, 0x00FF0000, True, False, rsa.GROUP_TABLE, 8),
    ("first-v8", ol.U32, 0x00FF0000, False, True, rsa.GROUP_SORT, 8),     # the sample lets them through, no table takes `first`
    ("counts-v9", ol.U32, 0x01FF0000, True, False, rsa.GROUP_SORT, 0),
    ("u64-v24", ol.U64, M24 << 20, False, False, rsa.GROUP_RANK_GLOBAL, 24),
    ("u64-v25", ol.U64, M25 << 20, False, False, rsa.GROUP_SORT, 0),
    ("u16-full", ol.U16, 0xFFFF, False, False, rsa.GROUP_RANK_LDS, 16),
    ("u16-full-counts", ol.U16, 0xFFFF, True, False, rsa.GROUP_SORT, 16),
]


@pytest.mark.parametrize("case", GROUP, ids=[c[0] for c in GROUP])
def test_group(case):
    name, dt, mask, counts, first, route, vbits = case
    got = tg.run(keys(dt, mask), dt, keys=False, counts=counts, first=first)
    info = got[4]
    print(name, seen(info, route, vbits, tg.ROUTE))
    tg.compare(got[:4], want_group(dt, mask), "%s route=%s" % (name, tg.ROUTE.get(info.route)))
    assert (got[2] is not None) == counts and (got[3] is not None) == first and got[1] is None
    assert info.route == route and info.varying_bits == vbits, seen(info, route, vbits, tg.ROUTE)


# (name, dtype, mask, outputs, switch or None, route, varying bits)
RANKDATA = [
    ("place-v8", ol.U32, 0x00FF0000, PLACE, None, rsa.RANKDATA_TABLE, 8),
    ("place-v9", ol.U32, 0x01FF0000, PLACE, None, rsa.RANKDATA_SORT, 0),
    ("less-v16", ol.U32, 0x0000FFFF, LESS, None, rsa.RANKDATA_COUNT16, 16),
    ("less-v17", ol.U32, 0x0001FFFF, LESS, None, rsa.RANKDATA_SORT, 0),
    ("no-tables-v8", ol.U32, 0x00FF0000, PLACE, ("RSX_RANKDATA_NO_TABLES", "1"), rsa.RANKDATA_SORT, 0),
    ("u64-less-v16", ol.U64, 0xFFFF << 20, LESS, None, rsa.RANKDATA_COUNT16, 16),
    ("u64-v24", ol.U64, M24 << 20, LESS, None, rsa.RANKDATA_SORT, 0),
    ("u64-v25", ol.U64, M25 << 20, PLACE, None, rsa.RANKDATA_SORT, 0),
    ("u16-full-less", ol.U16, 0xFFFF, LESS, None, rsa.RANKDATA_COUNT16, 16),
    ("u16-full-place", ol.U16, 0xFFFF, PLACE, None, rsa.RANKDATA_SORT, 16),
]


@pytest.mark.parametrize("case", RANKDATA, ids=[c[0] for c in RANKDATA])
def test_rankdata(case, monkeypatch):
    name, dt, mask, what, switch, route, vbits = case
    if switch:
        monkeypatch.setenv(*switch)
    info, _ = tr.check(keys(dt, mask), dt, what=what, tag=name, want=want_rankdata(dt, mask))
    print(name, seen(info, route, vbits, tr.ROUTE))
    assert info.route == route and info.varying_bits == vbits, seen(info, route, vbits, tr.ROUTE)
