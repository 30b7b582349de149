"""rsx_sort_topk / rsx_sort_topk_device without a GPU: the symbols, k == 0, the argument checks, and the refusal to do anything
on the CPU (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa


def _call(src, n, k, dtype, order, keys, idx, idx_bytes, device=False):
    lib = rsa.lib()
    info = rsa.TopkInfo()
    kp = None if keys is None else keys.ctypes.data
    ip = None if idx is None else idx.ctypes.data
    if device:
        rc = lib.rsx_sort_topk_device(src.ctypes.data, n, k, dtype, order, kp, ip, idx_bytes, None, C.byref(info))
    else:
        rc = lib.rsx_sort_topk(src.ctypes.data, n, k, dtype, order, kp, ip, idx_bytes, C.byref(info))
    return rc, info


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_topk" in names and "rsx_sort_topk_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_topk.argtypes) == 9
    assert len(lib.rsx_sort_topk_device.argtypes) == 10
    assert C.sizeof(rsa.TopkInfo) == 40     # 4 x u32 + 3 x u64
    assert (rsa.TOPK_TRIVIAL, rsa.TOPK_SELECT, rsa.TOPK_SORT) == (0, 1, 2)


@pytest.mark.parametrize("device", [False, True])
def test_k_zero_needs_no_device(device):
    src = np.array([5, 3, 9], dtype=np.uint32)
    keys = np.array([0xA5], dtype=np.uint32)
    idx = np.array([0xC3], dtype=np.uint32)
    rc, info = _call(src, 3, 0, rsa.U32, 0, keys, idx, 4, device)
    assert rc == 0 and info.route == rsa.TOPK_TRIVIAL and info.key_bytes == 4
    assert (info.input_reads, info.digit_passes, info.n_less, info.n_equal) == (0, 0, 0, 0)
    assert list(src) == [5, 3, 9] and keys[0] == 0xA5 and idx[0] == 0xC3
    rc, info = _call(src, 0, 0, rsa.F64, 1, keys, None, 8, device)     # no keys at all
    assert rc == 0 and info.route == rsa.TOPK_TRIVIAL and info.key_bytes == 8


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    keys = np.zeros(4, dtype=np.uint32)
    idx = np.zeros(4, dtype=np.uint32)
    for device in (False, True):
        rc, _ = _call(a, 4, 5, rsa.U32, 0, keys, idx, 4, device)
        assert rc == -1 and b"k exceeds n" in lib.rsx_last_error()
        rc, _ = _call(a, 4, 2, rsa.U32, 0, None, None, 4, device)
        assert rc == -1 and b"both outputs" in lib.rsx_last_error()
        rc, _ = _call(a, 4, 2, rsa.U32, 0, keys, idx, 3, device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _ = _call(a, 4, 2, 99, 0, keys, idx, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, 2, rsa.U32, 2, keys, idx, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            rc, _ = _call(a, (1 << 32) + 1, 2, rsa.U8, 0, keys, idx, 4, device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and not keys.any() and not idx.any()


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    keys = np.full(2, 0xA5, dtype=np.uint32)
    idx = np.full(2, 0xC3, dtype=np.uint64)
    for device in (False, True):
        rc, info = _call(src, 4, 2, rsa.U32, 0, keys, idx, 8, device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_topk_host(src, 2, rsa.U32)
    assert list(src) == [3, 1, 3, 2] and list(keys) == [0xA5] * 2 and list(idx) == [0xC3] * 2
