"""rsx_sort_locate / rsx_sort_locate_device without a GPU: the symbols, the argument checks, m == 0 with no bins wanted, the Python
wrappers' own checks, and the refusal to do anything else on the CPU (there is no CPU path) with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xA5A5A5A5


def _call(src, n, vals, m, dtype, order, less, equal, bins, idx_bytes, flags=0, device=False, null_src=False, null_vals=False):
    lib = rsa.lib()
    info = rsa.LocateInfo()
    p = lambda a: None if a is None else a.ctypes.data
    sp = None if null_src else p(src)
    vp = None if null_vals else p(vals)
    if device:
        rc = lib.rsx_sort_locate_device(sp, n, vp, m, dtype, order, p(less), p(equal), p(bins), idx_bytes, flags, None, C.byref(info))
    else:
        rc = lib.rsx_sort_locate(sp, n, vp, m, dtype, order, p(less), p(equal), p(bins), idx_bytes, flags, C.byref(info))
    return rc, info


def _outs(m, n):
    return np.full(m, FILL, dtype=np.uint32), np.full(m, FILL, dtype=np.uint32), np.full(n, FILL, dtype=np.uint32)


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_locate" in names and "rsx_sort_locate_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_locate.argtypes) == 12
    assert len(lib.rsx_sort_locate_device.argtypes) == 13
    assert C.sizeof(rsa.LocateInfo) == 24 + C.sizeof(rsa.Info)     # 6 x u32 + rsx_info
    assert (rsa.LOCATE_TRIVIAL, rsa.LOCATE_TABLE, rsa.LOCATE_SEARCH, rsa.LOCATE_SORT) == (0, 1, 2, 3)
    assert rsa.LOCATE_MAX_SEARCH_VALUES == 4096 and rsa.LOCATE_BINS_BELOW == 1


@pytest.mark.parametrize("device", [False, True])
def test_no_values_and_no_bins_need_no_device(device):
    src = np.array([5, 3, 9], dtype=np.uint32)
    vals = np.array([4], dtype=np.uint32)
    less, equal, bins = _outs(1, 3)
    rc, info = _call(src, 3, vals, 0, rsa.U32, 0, less, equal, None, 4, device=device)
    assert rc == 0 and info.route == rsa.LOCATE_TRIVIAL and info.key_bytes == 4
    assert (info.input_reads, info.distinct_values, info.search_steps, info.counter_sets) == (0, 0, 0, 0)
    assert list(src) == [5, 3, 9] and less[0] == FILL and equal[0] == FILL
    rc, info = _call(src, 3, vals, 0, rsa.F64, 1, less, None, None, 8, device=device, null_vals=True)     # vals == NULL is fine with m == 0
    assert rc == 0 and info.route == rsa.LOCATE_TRIVIAL and info.key_bytes == 8
    rc, info = _call(src, 0, vals, 0, rsa.U8, 0, less, equal, bins, 4, device=device, null_src=True)     # no keys either: no bin to write
    assert rc == 0 and info.route == rsa.LOCATE_TRIVIAL and bins[0] == FILL


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    v = np.zeros(2, dtype=np.uint32)
    less, equal, bins = _outs(2, 4)
    for device in (False, True):
        rc, _ = _call(a, 4, v, 2, rsa.U32, 0, None, None, None, 4, device=device)
        assert rc == -1 and b"all three outputs" in lib.rsx_last_error()
        rc, _ = _call(a, 4, v, 2, rsa.U32, 0, less, equal, bins, 3, device=device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _ = _call(a, 4, v, 2, 99, 0, less, equal, bins, 4, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, v, 2, rsa.U32, 2, less, equal, bins, 4, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, v, 2, rsa.U32, 0, less, equal, bins, 4, flags=2, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, v, 2, rsa.U32, 0, less, equal, bins, 4, device=device, null_src=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, v, 2, rsa.U32, 0, less, equal, bins, 4, device=device, null_vals=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            rc, _ = _call(a, (1 << 32) + 1, v, 2, rsa.U8, 0, less, None, None, 4, device=device)     # less may be n itself
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
            rc, _ = _call(a, 4, v, (1 << 32) + 1, rsa.U8, 0, None, None, bins, 4, device=device)     # a bin may be m itself
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and not v.any()
    assert (less == FILL).all() and (equal == FILL).all() and (bins == FILL).all()


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    vals = np.array([2, 9], dtype=np.uint32)
    less, equal, bins = _outs(2, 4)
    for device in (False, True):
        for args in ((src, 4, vals, 2, less, equal, bins), (src, 4, vals, 0, None, None, bins), (src, 0, vals, 2, less, equal, None),
                     (src, 1, vals, 1, less, None, None)):
            s, n, v, m, le, eq, bi = args
            rc, _ = _call(s, n, v, m, rsa.U32, 0, le, eq, bi, 4, device=device)
            assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_locate_host(src, vals, rsa.U32, bins=True)
    assert list(src) == [3, 1, 3, 2] and list(vals) == [2, 9]
    assert (less == FILL).all() and (equal == FILL).all() and (bins == FILL).all()


def test_python_wrappers_check_their_arguments():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_locate_host(src, np.array([1], dtype=np.uint32), rsa.U64)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_locate_host(src, np.array([1], dtype=np.uint64), rsa.U32)
    with pytest.raises(rsa.RsxError, match="room"):
        rsa.radix_sort_locate_host(src, np.array([1, 2], dtype=np.uint32), rsa.U32, less=np.zeros(1, dtype=np.uint32))
    with pytest.raises(rsa.RsxError, match="all three outputs"):
        rsa.radix_sort_locate_host(src, np.array([1], dtype=np.uint32), rsa.U32, less=False)
    info, le, eq, bi = rsa.radix_sort_locate_host(src, np.zeros(0, dtype=np.uint32), rsa.U32, equal=True)     # nothing asked: nothing needed
    assert le.size == 0 and eq.size == 0 and bi is None and info.route == rsa.LOCATE_TRIVIAL
    with pytest.raises(rsa.RsxError, match="neither"):
        rsa.searchsorted(None, None, side="middle")
