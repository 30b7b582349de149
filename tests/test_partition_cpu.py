"""rsx_sort_partition / rsx_sort_partition_device without a GPU: the symbols, the argument checks, n == 0 on host pointers, the Python
wrappers' own checks, and the refusal to do anything else on the CPU (there is no CPU path) with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xA5A5A5A5


def _call(src, n, edges, m, dtype, order, keys, idx, offsets, idx_bytes, flags=0, device=False, null_src=False, null_edges=False, keys_is_src=False):
    lib = rsa.lib()
    info = rsa.PartitionInfo()
    p = lambda a: None if a is None else a.ctypes.data
    sp = None if null_src else p(src)
    ep = None if null_edges else p(edges)
    kp = sp if keys_is_src else p(keys)
    if device:
        rc = lib.rsx_sort_partition_device(sp, n, ep, m, dtype, order, kp, p(idx), p(offsets), idx_bytes, flags, None, C.byref(info))
    else:
        rc = lib.rsx_sort_partition(sp, n, ep, m, dtype, order, kp, p(idx), p(offsets), idx_bytes, flags, C.byref(info))
    return rc, info


def _outs(n, m):
    return np.full(n, FILL, dtype=np.uint32), np.full(n, FILL, dtype=np.uint32), np.full(m + 2, FILL, dtype=np.uint32)


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_partition" in names and "rsx_sort_partition_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_partition.argtypes) == 12
    assert len(lib.rsx_sort_partition_device.argtypes) == 13
    assert C.sizeof(rsa.PartitionInfo) == 28 + C.sizeof(rsa.LocateInfo) + C.sizeof(rsa.Info)     # 7 x u32 + rsx_locate_info + rsx_info
    assert (rsa.PARTITION_TRIVIAL, rsa.PARTITION_SCATTER, rsa.PARTITION_SORT) == (0, 1, 2)
    assert rsa.PARTITION_MAX_EDGES == 255 and rsa.PARTITION_BELOW == 1
    header = open(rsa.__file__.replace("radix_sorting_amd/__init__.py", "include/rsx.h")).read()
    assert "RSX_PARTITION_DEFAULT_MAX_EDGES = %d" % rsa.PARTITION_DEFAULT_MAX_EDGES in header and 1 <= rsa.PARTITION_DEFAULT_MAX_EDGES <= 255
    assert "PARTITION_MAX_EDGES_DEFAULT = %d," % rsa.PARTITION_DEFAULT_MAX_EDGES in open(rsa.__file__.replace("__init__.py", "csrc/rsx_env.hpp")).read()
    assert rsa.PARTITION_TILE == 8192 and rsa.PARTITION_SHARE_TILES >= 1
    text = open(rsa.__file__.replace("__init__.py", "csrc/rsx_partition_shape.hpp")).read()
    assert "PARTITION_TILE = %d" % rsa.PARTITION_TILE in text and "PARTITION_SHARE_TILES = %d" % rsa.PARTITION_SHARE_TILES in text
    assert "PARTITION_BALLOT_PARTS_DEFAULT = %d" % rsa.PARTITION_BALLOT_PARTS in text


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    e = np.zeros(2, dtype=np.uint32)
    keys, idx, off = _outs(4, 2)
    for device in (False, True):
        rc, _ = _call(a, 4, e, 2, rsa.U32, 0, None, None, off, 4, device=device)
        assert rc == -1 and b"both of out_keys and out_idx" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, rsa.U32, 0, keys, idx, off, 3, device=device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, 99, 0, keys, idx, off, 4, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, rsa.U32, 2, keys, idx, off, 4, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, rsa.U32, 0, keys, idx, off, 4, flags=2, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, rsa.U32, 0, keys, idx, off, 4, device=device, null_src=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, rsa.U32, 0, keys, idx, off, 4, device=device, null_edges=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, e, 2, rsa.U32, 0, keys, idx, off, 4, device=device, keys_is_src=True)
        assert rc == -1 and b"out_keys is src" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            rc, _ = _call(a, (1 << 32) + 1, e, 2, rsa.U8, 0, keys, idx, off, 4, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
            rc, _ = _call(a, 4, e, (1 << 32) + 1, rsa.U8, 0, keys, idx, off, 4, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and not e.any()
    assert (keys == FILL).all() and (idx == FILL).all() and (off == FILL).all()


def test_no_keys_on_host_pointers_need_no_device():
    """n == 0: the offsets all zero and nothing else written -- on host pointers without a device call"""
    a = np.array([7], dtype=np.uint64)
    e = np.array([3, 1, 2], dtype=np.uint64)
    keys, idx = np.full(1, FILL, dtype=np.uint64), np.full(1, FILL, dtype=np.uint64)
    off = np.full(6, FILL, dtype=np.uint64)
    rc, info = _call(a, 0, e, 3, rsa.U64, 1, keys, idx, off, 8)
    assert rc == 0 and info.route == rsa.PARTITION_TRIVIAL and info.key_bytes == 8
    assert list(off) == [0, 0, 0, 0, 0, FILL] and keys[0] == FILL and idx[0] == FILL
    assert (info.input_reads, info.distinct_edges, info.search_steps, info.rank_form, info.shares) == (0, 0, 0, 0, 0)
    off32 = np.full(3, FILL, dtype=np.uint32)
    rc, info = _call(a, 0, e, 0, rsa.I8, 0, keys, None, off32, 4, null_src=True, null_edges=True)     # no edges either: offsets = {0, 0}
    assert rc == 0 and list(off32) == [0, 0, FILL]
    for device in (False, True):     # no offsets wanted: nothing to do at all
        rc, info = _call(a, 0, e, 3, rsa.U64, 0, keys, idx, None, 8, device=device)
        assert rc == 0 and info.route == rsa.PARTITION_TRIVIAL and keys[0] == FILL and idx[0] == FILL
    info, k, i, o = rsa.radix_sort_partition_host(a[:0], e, rsa.U64, idx=True)
    assert info.route == rsa.PARTITION_TRIVIAL and k.size == 0 and i.size == 0 and list(o) == [0] * 5


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    edges = np.array([2, 9], dtype=np.uint32)
    keys, idx, off = _outs(4, 2)
    for device in (False, True):
        for args in ((src, 4, edges, 2, keys, idx, off), (src, 4, edges, 0, keys, None, off), (src, 1, edges, 1, None, idx, None)):
            s, n, e, m, ke, ix, of = args
            rc, _ = _call(s, n, e, m, rsa.U32, 0, ke, ix, of, 4, device=device)
            assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    rc, _ = _call(src, 0, edges, 2, rsa.U32, 0, keys, idx, off, 4, device=True)     # the device entry point's offsets are device memory
    assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_partition_host(src, edges, rsa.U32, idx=True)
    assert list(src) == [3, 1, 3, 2] and list(edges) == [2, 9]
    assert (keys == FILL).all() and (idx == FILL).all() and (off == FILL).all()


def test_python_wrappers_check_their_arguments():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_partition_host(src, np.array([1], dtype=np.uint32), rsa.U64)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_partition_host(src, np.array([1], dtype=np.uint64), rsa.U32)
    with pytest.raises(rsa.RsxError, match="room"):
        rsa.radix_sort_partition_host(src, np.array([1, 2], dtype=np.uint32), rsa.U32, offsets=np.zeros(3, dtype=np.uint32))
    with pytest.raises(rsa.RsxError, match="room"):
        rsa.radix_sort_partition_host(src, np.array([1, 2], dtype=np.uint32), rsa.U32, keys=np.zeros(4, dtype=np.uint64))
    with pytest.raises(rsa.RsxError, match="both of out_keys and out_idx"):
        rsa.radix_sort_partition_host(src, np.array([1], dtype=np.uint32), rsa.U32, keys=False)
    with pytest.raises(rsa.RsxError, match="not in 1"):
        rsa.partition_even(None, 0)
    with pytest.raises(rsa.RsxError, match="not in 1"):
        rsa.partition_even(None, 66)
