"""rsx_sort_rankdata / rsx_sort_rankdata_device without a GPU: the symbols, the small sizes, the argument checks, and the refusal to
do anything on the CPU (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xC3


def _outs(n, idt=np.uint32):
    return [np.full(n, FILL, dtype=idt), np.full(n, FILL, dtype=idt), np.full(n, FILL, dtype=idt)]


def _call(src, n, dtype, order, outs, idx_bytes, device=False, src_null=False):
    lib = rsa.lib()
    info = rsa.RankdataInfo()
    p = [None if o is None else o.ctypes.data for o in outs]
    sp = None if src_null else src.ctypes.data
    if device:
        rc = lib.rsx_sort_rankdata_device(sp, n, dtype, order, p[0], p[1], p[2], idx_bytes, None, C.byref(info))
    else:
        rc = lib.rsx_sort_rankdata(sp, n, dtype, order, p[0], p[1], p[2], idx_bytes, C.byref(info))
    return rc, info


def _untouched(outs):
    return all(o is None or bool(np.all(o == FILL)) for o in outs)


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_rankdata" in names and "rsx_sort_rankdata_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_rankdata.argtypes) == 9 and len(lib.rsx_sort_rankdata_device.argtypes) == 10
    assert C.sizeof(rsa.RankdataInfo) == 72    # rsx_info's 52 + 4 + 4, padded to 8, + 8
    assert (rsa.RANKDATA_TRIVIAL, rsa.RANKDATA_TABLE, rsa.RANKDATA_COUNT16, rsa.RANKDATA_SORT) == (0, 1, 2, 3)
    assert callable(rsa.radix_sort_rankdata) and callable(rsa.radix_sort_rankdata_host) and callable(rsa.rankdata)


@pytest.mark.parametrize("device", [False, True])
def test_no_keys_need_no_device(device):
    src = np.array([5], dtype=np.uint32)
    outs = _outs(1)
    rc, info = _call(src, 0, rsa.U32, 0, outs, 4, device)
    assert rc == 0 and _untouched(outs) and src[0] == 5
    assert info.route == rsa.RANKDATA_TRIVIAL and info.sort.early_exit == 1 and info.sort.key_bytes == 4
    rc, _ = _call(src, 0, rsa.U32, 0, [None, outs[1], None], 8, device, src_null=True)
    assert rc == 0 and _untouched(outs)


@pytest.mark.parametrize("ib,idt", [(4, np.uint32), (8, np.uint64)])
def test_one_key_on_the_host(ib, idt):
    src = np.array([-3.5], dtype=np.float32)
    outs = _outs(2, idt)
    rc, info = _call(src, 1, rsa.F32, 1, outs, ib)
    assert rc == 0 and info.route == rsa.RANKDATA_TRIVIAL and info.sort.early_exit == 1
    place, less, equal = outs
    assert place[0] == 0 and less[0] == 0 and equal[0] == 1
    assert all(o[1] == FILL for o in outs)   # nothing past element 0
    one = _outs(2, idt)
    rc, _ = _call(src, 1, rsa.F32, 0, [None, None, one[2]], ib)
    assert rc == 0 and one[2][0] == 1 and _untouched(one[:2])
    place, less, equal, _ = rsa.radix_sort_rankdata_host(src, rsa.F32, less=True, equal=True, idx_dtype=idt)
    assert list(place) == [0] and list(less) == [0] and list(equal) == [1]
    place, less, equal, _ = rsa.radix_sort_rankdata_host(src, rsa.F32)
    assert list(place) == [0] and less is None and equal is None


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    outs = _outs(4)
    for device in (False, True):
        rc, _ = _call(a, 4, rsa.U32, 0, outs, 3, device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _ = _call(a, 4, 99, 0, outs, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, rsa.U32, 2, outs, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, rsa.U32, 0, outs, 4, device, src_null=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _call(a, 4, rsa.U32, 0, [None] * 3, 4, device)
        assert rc == -1 and b"all three outputs are NULL" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            # (a dummy pointer: the call must fail before any device work)
            rc, _ = _call(a, 1 << 32, rsa.U8, 0, outs, 4, device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and _untouched(outs)
    with pytest.raises(rsa.RsxError, match="none of"):
        rsa.rankdata(None, method="first")


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_rankdata_host(src, rsa.U32, less=True, equal=True)
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_rankdata_host(src, rsa.U32, place=False, less=True)
    for device in (False, True):
        outs = _outs(4)
        rc, _ = _call(src, 4, rsa.U32, 0, outs, 4, device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
        assert list(src) == [3, 1, 3, 2] and _untouched(outs)
    one = _outs(1)
    rc, _ = _call(src, 1, rsa.U32, 0, one, 4, device=True)     # the device form needs the device for its stores
    assert rc == -2 and _untouched(one)
