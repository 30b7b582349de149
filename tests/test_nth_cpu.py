"""rsx_sort_nth / rsx_sort_nth_device without a GPU: the symbols, m == 0, the argument checks, n == 1 on host pointers, the
Python wrappers' own checks, and the refusal to do anything else on the CPU (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

P64 = C.POINTER(C.c_uint64)
FILL = 0xA5A5A5A5A5A5A5A5


def _call(src, n, ranks, dtype, order, keys, idx, idx_bytes, device=False, m=None, null_ranks=False):
    """One raw call; returns (rc, info, n_less, n_equal) with the host arrays prefilled."""
    lib = rsa.lib()
    info = rsa.NthInfo()
    r = np.ascontiguousarray(ranks, dtype=np.uint64)
    m = r.size if m is None else m
    n_less = np.full(max(m, 1), FILL, dtype=np.uint64)
    n_equal = np.full(max(m, 1), FILL, dtype=np.uint64)
    kp = None if keys is None else keys.ctypes.data
    ip = None if idx is None else idx.ctypes.data
    rp = None if null_ranks else r.ctypes.data_as(P64)
    if device:
        rc = lib.rsx_sort_nth_device(src.ctypes.data, n, rp, m, dtype, order, kp, ip, idx_bytes, n_less.ctypes.data_as(P64),
                                     n_equal.ctypes.data_as(P64), None, C.byref(info))
    else:
        rc = lib.rsx_sort_nth(src.ctypes.data, n, rp, m, dtype, order, kp, ip, idx_bytes, n_less.ctypes.data_as(P64),
                              n_equal.ctypes.data_as(P64), C.byref(info))
    return rc, info, n_less, n_equal


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_nth" in names and "rsx_sort_nth_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_nth.argtypes) == 12
    assert len(lib.rsx_sort_nth_device.argtypes) == 13
    assert C.sizeof(rsa.NthInfo) == 32     # 6 x u32 + 1 x u64
    assert (rsa.NTH_TRIVIAL, rsa.NTH_SELECT, rsa.NTH_SORT) == (0, 1, 2)
    assert rsa.NTH_MAX_SELECT_RANKS == 64


@pytest.mark.parametrize("device", [False, True])
def test_m_zero_needs_no_device(device):
    src = np.array([5, 3, 9], dtype=np.uint32)
    keys = np.array([0xA5], dtype=np.uint32)
    idx = np.array([0xC3], dtype=np.uint32)
    rc, info, n_less, n_equal = _call(src, 3, [], rsa.U32, 0, keys, idx, 4, device)
    assert rc == 0 and info.route == rsa.NTH_TRIVIAL and info.key_bytes == 4
    assert (info.input_reads, info.digit_passes, info.active_buckets, info.from_prefix, info.candidates) == (0, 0, 0, 0, 0)
    assert list(src) == [5, 3, 9] and keys[0] == 0xA5 and idx[0] == 0xC3 and n_less[0] == FILL and n_equal[0] == FILL
    rc, info, _, _ = _call(src, 3, [], rsa.F64, 1, keys, None, 8, device, null_ranks=True)     # ranks == NULL is fine with m == 0
    assert rc == 0 and info.route == rsa.NTH_TRIVIAL and info.key_bytes == 8
    rc, info, _, _ = _call(src, 0, [], rsa.U8, 0, keys, None, 4, device)     # no keys at all
    assert rc == 0 and info.route == rsa.NTH_TRIVIAL


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    keys = np.zeros(4, dtype=np.uint32)
    idx = np.zeros(4, dtype=np.uint32)
    for device in (False, True):
        for ranks in ([4], [0, 1, 7], [2 ** 63]):
            rc, _, n_less, n_equal = _call(a, 4, ranks, rsa.U32, 0, keys, idx, 4, device)
            assert rc == -1 and b"rank exceeds n" in lib.rsx_last_error()
            assert (n_less == FILL).all() and (n_equal == FILL).all()
        rc, _, _, _ = _call(a, 0, [0], rsa.U32, 0, keys, idx, 4, device)          # no keys: every rank is out of range
        assert rc == -1 and b"rank exceeds n" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, 4, [1, 2], rsa.U32, 0, None, None, 4, device)
        assert rc == -1 and b"both outputs" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, 4, [1, 2], rsa.U32, 0, keys, idx, 3, device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, 4, [1, 2], 99, 0, keys, idx, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, 4, [1, 2], rsa.U32, 2, keys, idx, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, 4, [], rsa.U32, 0, keys, idx, 4, device, m=2, null_ranks=True)
        assert rc == -1 and b"ranks is NULL" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            rc, _, _, _ = _call(a, (1 << 32) + 1, [1], rsa.U8, 0, keys, idx, 4, device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and not keys.any() and not idx.any()


@pytest.mark.parametrize("dt,npdt", [(rsa.U32, np.uint32), (rsa.F64, np.uint64), (rsa.I8, np.uint8)])
def test_one_key_on_host_pointers(dt, npdt):
    """n == 1: every rank is 0, the key is itself; rsx_sort_nth on host pointers does it without a device."""
    src = np.array([0x7B], dtype=npdt)
    for ib, idt in ((4, np.uint32), (8, np.uint64)):
        keys = np.full(4, 0x11, dtype=npdt)
        idx = np.full(4, 0x22, dtype=idt)
        rc, info, n_less, n_equal = _call(src, 1, [0, 0, 0], dt, 1, keys, idx, ib)
        assert rc == 0, rsa.lib().rsx_last_error()
        assert info.route == rsa.NTH_TRIVIAL and info.key_bytes == src.itemsize
        assert list(keys) == [0x7B] * 3 + [0x11] and list(idx) == [0, 0, 0, 0x22]
        assert list(n_less) == [0, 0, 0] and list(n_equal) == [1, 1, 1]
    keys = np.full(2, 0x11, dtype=npdt)
    rc, _, _, _ = _call(src, 1, [0], dt, 0, keys, None, 4)                    # keys only
    assert rc == 0 and list(keys) == [0x7B, 0x11]
    k, i, n_less, n_equal, info = rsa.radix_sort_nth_host(src, [0, 0], dt)
    assert list(k) == [0x7B, 0x7B] and list(i) == [0, 0] and list(n_less) == [0, 0] and list(n_equal) == [1, 1]


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    keys = np.full(2, 0xA5, dtype=np.uint32)
    idx = np.full(2, 0xC3, dtype=np.uint64)
    for device in (False, True):
        rc, info, n_less, n_equal = _call(src, 4, [1, 3], rsa.U32, 0, keys, idx, 8, device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
        assert (n_less == FILL).all() and (n_equal == FILL).all()
    one = np.array([3], dtype=np.uint32)
    rc, _, n_less, _ = _call(one, 1, [0], rsa.U32, 0, keys, idx, 8, True)      # the device form needs a device for its stores
    assert rc == -2 and n_less[0] == FILL
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_nth_host(src, [2], rsa.U32)
    assert list(src) == [3, 1, 3, 2] and list(keys) == [0xA5] * 2 and list(idx) == [0xC3] * 2


def test_python_wrappers_check_their_arguments():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="rank exceeds n"):
        rsa.radix_sort_nth_host(src, [4], rsa.U32)
    with pytest.raises(rsa.RsxError, match="negative"):
        rsa.radix_sort_nth_host(src, [-1], rsa.U32)
    with pytest.raises(rsa.RsxError, match="integers"):
        rsa.radix_sort_nth_host(src, [0.5], rsa.U32)
    with pytest.raises(rsa.RsxError, match="one-dimensional"):
        rsa.radix_sort_nth_host(src, [[0, 1]], rsa.U32)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_nth_host(src, [0], rsa.U64)
    k, i, n_less, n_equal, info = rsa.radix_sort_nth_host(src, [], rsa.U32)       # nothing asked: nothing needed
    assert k.size == 0 and i.size == 0 and n_less.size == 0 and info.route == rsa.NTH_TRIVIAL
