"""rsx_sort_segments / rsx_sort_segments_device without a GPU: the symbols, the argument checks, the trivial sizes on host pointers,
the Python wrappers' own checks, and the refusal to do anything else on the CPU (there is no CPU path) with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xA5A5A5A5


def _call(src, n, offsets, m, dtype, order, keys, idx, idx_bytes, flags=0, device=False, null_src=False, keys_is_src=False, keys_ptr=None):
    lib = rsa.lib()
    info = rsa.SegmentsInfo()
    p = lambda a: None if a is None else a.ctypes.data
    sp = None if null_src else p(src)
    kp = sp if keys_is_src else keys_ptr if keys_ptr is not None else p(keys)
    if device:
        rc = lib.rsx_sort_segments_device(sp, n, p(offsets), m, idx_bytes, dtype, order, kp, p(idx), flags, None, C.byref(info))
    else:
        rc = lib.rsx_sort_segments(sp, n, p(offsets), m, idx_bytes, dtype, order, kp, p(idx), flags, C.byref(info))
    return rc, info


def _outs(n):
    return np.full(n, FILL, dtype=np.uint32), np.full(n, FILL, dtype=np.uint32)


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_segments" in names and "rsx_sort_segments_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_segments.argtypes) == 11
    assert len(lib.rsx_sort_segments_device.argtypes) == 12
    assert C.sizeof(rsa.SegmentsInfo) == 16 + 16 + 8 * rsa.SEGMENTS_CLASSES + C.sizeof(rsa.LexInfo) + C.sizeof(rsa.Info) + 4     # (+ 4: the tail's alignment to 8)
    assert (rsa.SEGMENTS_TRIVIAL, rsa.SEGMENTS_LDS, rsa.SEGMENTS_MIXED, rsa.SEGMENTS_LEX) == (0, 1, 2, 3)
    assert rsa.SEGMENTS_LOCAL_IDX == 1 and rsa.SEGMENTS_CLASSES == 5
    header = open(rsa.__file__.replace("radix_sorting_amd/__init__.py", "include/rsx.h")).read()
    assert "RSX_SEGMENTS_CLASSES = %d" % rsa.SEGMENTS_CLASSES in header and "RSX_SEGMENTS_LOCAL_IDX = 1" in header
    env = open(rsa.__file__.replace("__init__.py", "csrc/rsx_env.hpp")).read()
    assert "SEGMENTS_MAX_LONG_COMPILED = %d, SEGMENTS_MAX_LONG_DEFAULT = %d, SEGMENTS_DEFAULT_CLASSES = %d }" % (
        rsa.SEGMENTS_MAX_LONG, rsa.SEGMENTS_DEFAULT_MAX_LONG, rsa.SEGMENTS_DEFAULT_CLASSES) in env
    shape = open(rsa.__file__.replace("__init__.py", "csrc/rsx_segments_shape.hpp")).read()
    assert "SEGMENTS_COPY_MAX = %d, SEGMENTS_WAVE_MAX = %d, SEGMENTS_GROUP_MAX = %d" % (
        rsa.SEGMENTS_COPY_MAX, rsa.SEGMENTS_WAVE_MAX, rsa.SEGMENTS_GROUP_MAX) in shape
    assert "SEGMENTS_LDS_BYTES = %d, SEGMENTS_TEAM_FIXED = %d" % (rsa.SEGMENTS_LDS_BYTES, rsa.SEGMENTS_TEAM_FIXED) in shape
    assert "SEGMENTS_MAX_LONG_LISTED = %d" % rsa.SEGMENTS_MAX_LONG in shape


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(6, dtype=np.uint32)
    off = np.array([0, 2, 6], dtype=np.uint32)
    keys, idx = _outs(6)
    for device in (False, True):
        rc, _ = _call(a, 6, off, 2, rsa.U32, 0, None, None, 4, device=device)
        assert rc == -1 and b"both of out_keys and out_idx" in lib.rsx_last_error()
        rc, _ = _call(a, 6, off, 2, rsa.U32, 0, keys, idx, 3, device=device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _ = _call(a, 6, off, 2, 99, 0, keys, idx, 4, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 6, off, 2, rsa.U32, 2, keys, idx, 4, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 6, off, 2, rsa.U32, 0, keys, idx, 4, flags=2, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 6, off, 2, rsa.U32, 0, keys, idx, 4, device=device, null_src=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 6, off, 2, rsa.U32, 0, keys, idx, 4, device=device, keys_is_src=True)
        assert rc == -1 and b"out_keys is src" in lib.rsx_last_error()
        rc, _ = _call(a, 4, off, 2, rsa.U32, 0, keys, idx, 4, device=device, keys_ptr=a.ctypes.data + 8)     # the last two of four keys
        assert rc == -1 and b"overlaps" in lib.rsx_last_error()
        rc, _ = _call(a, 6, None, 4, rsa.U32, 0, keys, idx, 4, device=device)
        assert rc == -1 and b"whole number" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            rc, _ = _call(a, (1 << 32) + 1, off, 2, rsa.U8, 0, keys, idx, 4, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
            rc, _ = _call(a, 6, off, (1 << 32) + 1, rsa.U8, 0, keys, idx, 8, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and list(off) == [0, 2, 6]
    assert (keys == FILL).all() and (idx == FILL).all()


def test_trivial_sizes_need_no_device():
    """n == 0 or m == 0: RSX_OK, route TRIVIAL, nothing written -- in either form, before any device call"""
    a = np.array([7, 3], dtype=np.uint64)
    off = np.array([0, 0, 0], dtype=np.uint64)
    keys, idx = np.full(2, FILL, dtype=np.uint64), np.full(2, FILL, dtype=np.uint64)
    for device in (False, True):
        for n, o, m in ((0, off, 2), (0, None, 3), (2, off, 0), (2, None, 0), (0, None, 0)):
            rc, info = _call(a, n, o, m, rsa.F64, 1, keys, idx, 8, device=device)
            assert rc == 0 and info.route == rsa.SEGMENTS_TRIVIAL and info.key_bytes == 8, (device, n, m)
            assert info.classes() == [0] * 5 and info.n_long == 0 and info.max_len == 0
    assert (keys == FILL).all() and (idx == FILL).all()
    info, k, i = rsa.radix_sort_segments_host(a[:0], rsa.U64, offsets=off, idx=True)
    assert info.route == rsa.SEGMENTS_TRIVIAL and k.size == 0 and i.size == 0


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    off = np.array([0, 1, 4], dtype=np.uint32)
    keys, idx = _outs(4)
    for device in (False, True):
        for o, m, ke, ix in ((off, 2, keys, idx), (None, 2, keys, None), (None, 4, None, idx), (off, 2, None, idx)):
            rc, _ = _call(src, 4, o, m, rsa.U32, 0, ke, ix, 4, device=device)
            assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_segments_host(src, rsa.U32, offsets=off, idx=True)
    assert list(src) == [3, 1, 3, 2] and list(off) == [0, 1, 4]
    assert (keys == FILL).all() and (idx == FILL).all()


def test_python_wrappers_check_their_arguments():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    off = np.array([0, 1, 4], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_segments_host(src, rsa.U64, offsets=off)
    with pytest.raises(rsa.RsxError, match="either offsets or rows"):
        rsa.radix_sort_segments_host(src, rsa.U32)
    with pytest.raises(rsa.RsxError, match="either offsets or rows"):
        rsa.radix_sort_segments_host(src, rsa.U32, offsets=off, rows=2)
    with pytest.raises(rsa.RsxError, match="4 or 8 bytes"):
        rsa.radix_sort_segments_host(src, rsa.U32, offsets=off.astype(np.uint16))
    with pytest.raises(rsa.RsxError, match="same size"):
        rsa.radix_sort_segments_host(src, rsa.U32, offsets=off, idx_dtype=np.uint64)
    with pytest.raises(rsa.RsxError, match="room"):
        rsa.radix_sort_segments_host(src, rsa.U32, offsets=off, keys=np.zeros(3, dtype=np.uint32))
    with pytest.raises(rsa.RsxError, match="both of out_keys and out_idx"):
        rsa.radix_sort_segments_host(src, rsa.U32, offsets=off, keys=False)
    with pytest.raises(rsa.RsxError, match="whole number"):
        rsa.radix_sort_segments_host(src, rsa.U32, rows=3)
    assert rsa.SEGMENTS_CAP(rsa.U32, True) == 12032 and rsa.SEGMENTS_CAP(rsa.F64, False) == 8960 and rsa.SEGMENTS_CAP(rsa.U8, False) == 65536
