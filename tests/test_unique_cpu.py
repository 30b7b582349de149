"""rsx_sort_unique / rsx_sort_unique_device without a GPU: the symbols, the small sizes, the argument checks, and the
refusal to do anything on the CPU (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa


def _call(src, aux, n, dtype, order, counts, count_bytes, device=False):
    lib = rsa.lib()
    res, nu, info = C.c_void_p(), C.c_size_t(77), rsa.UniqueInfo()
    cp = None if counts is None else counts.ctypes.data
    if device:
        rc = lib.rsx_sort_unique_device(src.ctypes.data, aux.ctypes.data, n, dtype, order, cp, count_bytes, None, C.byref(res),
                                        C.byref(nu), C.byref(info))
    else:
        rc = lib.rsx_sort_unique(src.ctypes.data, aux.ctypes.data, n, dtype, order, cp, count_bytes, C.byref(res), C.byref(nu),
                                 C.byref(info))
    return rc, res.value, nu.value, info


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_unique" in names and "rsx_sort_unique_device" in names
    lib = rsa.lib()
    assert lib.rsx_sort_unique.argtypes is not None and len(lib.rsx_sort_unique.argtypes) == 10
    assert len(lib.rsx_sort_unique_device.argtypes) == 11
    assert C.sizeof(rsa.Info) == 52 and C.sizeof(rsa.UniqueInfo) == 72    # 52 + 4 + 4, padded to 8, + 8
    assert (rsa.UNIQUE_TRIVIAL, rsa.UNIQUE_BITMAP_LDS, rsa.UNIQUE_BITMAP_GLOBAL, rsa.UNIQUE_TABLE, rsa.UNIQUE_SORT) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("device", [False, True])
def test_no_keys_need_no_device(device):
    src = np.array([5], dtype=np.uint32)
    aux = np.array([0xA5], dtype=np.uint32)
    counts = np.array([0xC3], dtype=np.uint32)
    rc, res, nu, info = _call(src, aux, 0, rsa.U32, 0, counts, 4, device)
    assert rc == 0 and res == src.ctypes.data and nu == 0
    assert info.route == rsa.UNIQUE_TRIVIAL and info.sort.early_exit == 1 and info.sort.key_bytes == 4
    assert src[0] == 5 and aux[0] == 0xA5 and counts[0] == 0xC3


@pytest.mark.parametrize("device", [False, True])
def test_one_key_without_counts_needs_no_device(device):
    src = np.array([5], dtype=np.uint64)
    aux = np.array([0xA5], dtype=np.uint64)
    rc, res, nu, info = _call(src, aux, 1, rsa.U64, 1, None, 0, device)
    assert rc == 0 and res == src.ctypes.data and nu == 1
    assert info.route == rsa.UNIQUE_TRIVIAL and info.sort.early_exit == 1
    assert src[0] == 5 and aux[0] == 0xA5


@pytest.mark.parametrize("cb,cdt", [(4, np.uint32), (8, np.uint64)])
def test_one_key_with_host_counts(cb, cdt):
    """n == 1 through rsx_sort_unique on host buffers: src is returned, aux untouched, counts[0] = 1."""
    src = np.array([-3.5], dtype=np.float32)
    aux = np.array([7.0], dtype=np.float32)
    counts = np.array([0xC3, 0xC3], dtype=cdt)
    out, cnt, info = rsa.radix_sort_unique_host(src, aux, rsa.F32, counts=counts)
    assert out.base is src or out is src
    assert out.size == 1 and out[0] == np.float32(-3.5) and aux[0] == np.float32(7.0)
    assert list(cnt) == [1] and counts[1] == 0xC3 and info.sort.early_exit == 1


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    b = np.zeros(4, dtype=np.uint32)
    c = np.zeros(4, dtype=np.uint32)
    for device in (False, True):
        rc, _, _, _ = _call(a, b, 4, rsa.U32, 0, c, 3, device)
        assert rc == -1 and b"count_bytes" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, b, 4, 99, 0, None, 0, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _, _, _ = _call(a, b, 4, rsa.U32, 2, None, 0, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
    if C.sizeof(C.c_size_t) == 8:
        rc, _, _, _ = _call(a, b, (1 << 32) + 1, rsa.U8, 0, c, 4, True)
        assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and not b.any() and not c.any()


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    aux = np.full(4, 0xA5, dtype=np.uint32)
    counts = np.full(4, 0xC3, dtype=np.uint64)
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_unique_host(src, aux, rsa.U32, counts=counts)
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_unique_host(src, aux, rsa.U32)
    rc, _, _, _ = _call(src, aux, 4, rsa.U32, 0, counts, 8, device=True)
    assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    assert list(src) == [3, 1, 3, 2] and list(aux) == [0xA5] * 4 and list(counts) == [0xC3] * 4
