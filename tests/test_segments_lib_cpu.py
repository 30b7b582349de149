"""tests/segments_lib.py on the CPU: the model of rsx_sort_segments -- per segment, np.argsort of the oracle's derived keys -- against
oracle_lib's rank sort segment by segment on a few dozen segments of every dtype and both orders, and the model's class / cap
arithmetic against the values tests/cpp/segments_shape_check prints from radix_sorting_amd/csrc/rsx_segments_shape.hpp."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa
import segments_lib as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offsets(rng, m, most):
    lens = rng.integers(0, most + 1, size=m)
    lens[rng.integers(0, m, size=m // 4)] = 0          # empty segments among them
    lens[rng.integers(0, m, size=m // 8)] = 1
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


@pytest.mark.parametrize("dt", list(range(10)))
def test_model_is_the_oracles_rank_sort_per_segment(dt):
    rng = np.random.default_rng(4100 + dt)
    off = _offsets(rng, 40, 300)
    n = int(off[-1])
    bits = ol.splitmix_fill(n, dt, 4200 + dt, 0xFFFF if ol.DTYPE_SIZE[dt] > 1 else 0x1F)     # many ties: stability shows
    for order in (ol.ASC, ol.DESC):
        want = sg.Want(bits, dt, off, order)
        assert sorted(want.idx.tolist()) == list(range(n))
        for s in range(40):
            a, b = int(off[s]), int(off[s + 1])
            ranks, _, _, _ = ol.oracle_rank(bits[a:b], dt, 4, order)
            assert np.array_equal(want.local[a:b], ranks.astype(np.uint64)), (dt, order, s)
            assert np.array_equal(want.idx[a:b], ranks.astype(np.uint64) + np.uint64(a))
            assert np.array_equal(want.keys[a:b], bits[a:b][ranks.astype(np.int64)])
        assert np.array_equal(want.bits, bits)


def test_uniform_offsets_and_routes():
    assert list(sg.uniform_offsets(12, 3)) == [0, 4, 8, 12]
    bits = ol.splitmix_fill(22137, ol.U64, 5)
    want = sg.Want(bits, ol.U64, [0, 0, 1, 13, 13, 300, 300 + 7168, 300 + 7168 + 7169, 22137])
    counts, max_len, n_long, c = want.classes(True)
    assert c == 7168 and counts == [3, 1, 1, 1, 2] and n_long == 2 and max_len == 7500
    assert want.classes(False)[0] == [3, 1, 1, 3, 0]
    assert want.natural_route(True, "2") == rsa.SEGMENTS_LEX and want.natural_route(True, "1", 2) == rsa.SEGMENTS_MIXED
    assert want.natural_route(True, "1", 1) == rsa.SEGMENTS_LEX and want.natural_route(False, "1") == rsa.SEGMENTS_LDS


def test_class_and_cap_arithmetic_is_the_headers():
    exe = os.path.join(ROOT, "tests", "cpp", "segments_shape_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/segments_shape_check"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [tuple(int(x) for x in line.split()[1:]) for line in out.stdout.splitlines() if line.startswith("cap ")]
    assert len(rows) == 8
    for kb, with_idx, cap, lds in rows:
        assert sg.cap(kb, bool(with_idx)) == cap, (kb, with_idx)
        assert sg.lds_bytes(sg.BLOCK, kb, bool(with_idx), cap) == lds <= sg.LDS_BYTES
        dt = {1: rsa.U8, 2: rsa.U16, 4: rsa.U32, 8: rsa.U64}[kb]
        assert rsa.SEGMENTS_CAP(dt, bool(with_idx)) == cap
        for length in sg.seam_lengths(cap):
            cls = sg.class_of(length, cap)
            assert sg.lds_bytes(cls, kb, bool(with_idx), length) <= sg.LDS_BYTES
            if cls in sg.TEAM_WAVES:
                assert sg.stride(cls, length, cap) >= length
        assert [sg.class_of(x, cap) for x in (0, 1, 2, 256, 257, 2048, 2049, cap, cap + 1)] == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    assert (sg.COPY_MAX, sg.WAVE_MAX, sg.GROUP_MAX) == (rsa.SEGMENTS_COPY_MAX, rsa.SEGMENTS_WAVE_MAX, rsa.SEGMENTS_GROUP_MAX)
    assert sg.grid(sg.WAVE, 5) == 2 and sg.grid(sg.BLOCK, 5) == 5 and sg.grid(sg.COPY, 257) == 2
