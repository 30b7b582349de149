"""rsx_sort_group / rsx_sort_group_device without a GPU: the symbols, the small sizes, the argument checks, and the refusal to do
anything on the CPU (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xC3


def _outs(n, kdt=np.uint32, idt=np.uint32):
    return [np.full(n, FILL, dtype=idt), np.full(n, FILL, dtype=kdt), np.full(n, FILL, dtype=idt), np.full(n, FILL, dtype=idt)]


def _call(src, n, dtype, order, outs, idx_bytes, device=False, ng_null=False, src_null=False):
    lib = rsa.lib()
    ng, info = C.c_size_t(77), rsa.GroupInfo()
    p = [None if o is None else o.ctypes.data for o in outs]
    sp = None if src_null else src.ctypes.data
    ngp = None if ng_null else C.byref(ng)
    if device:
        rc = lib.rsx_sort_group_device(sp, n, dtype, order, p[0], p[1], p[2], p[3], idx_bytes, None, ngp, C.byref(info))
    else:
        rc = lib.rsx_sort_group(sp, n, dtype, order, p[0], p[1], p[2], p[3], idx_bytes, ngp, C.byref(info))
    return rc, ng.value, info


def _untouched(outs):
    return all(o is None or bool(np.all(o == FILL)) for o in outs)


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_group" in names and "rsx_sort_group_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_group.argtypes) == 11 and len(lib.rsx_sort_group_device.argtypes) == 12
    assert C.sizeof(rsa.GroupInfo) == 72    # rsx_info's 52 + 4 + 4, padded to 8, + 8
    assert (rsa.GROUP_TRIVIAL, rsa.GROUP_RANK_LDS, rsa.GROUP_RANK_GLOBAL, rsa.GROUP_TABLE, rsa.GROUP_SORT) == (0, 1, 2, 3, 4)
    assert callable(rsa.radix_sort_group) and callable(rsa.radix_sort_group_host)


@pytest.mark.parametrize("device", [False, True])
def test_no_keys_need_no_device(device):
    src = np.array([5], dtype=np.uint32)
    outs = _outs(1)
    rc, ng, info = _call(src, 0, rsa.U32, 0, outs, 4, device)
    assert rc == 0 and ng == 0 and _untouched(outs) and src[0] == 5
    assert info.route == rsa.GROUP_TRIVIAL and info.sort.early_exit == 1 and info.sort.key_bytes == 4
    rc, ng, _ = _call(src, 0, rsa.U32, 0, [None] * 4, 8, device, src_null=True)
    assert rc == 0 and ng == 0


@pytest.mark.parametrize("ib,idt", [(4, np.uint32), (8, np.uint64)])
def test_one_key_on_the_host(ib, idt):
    src = np.array([-3.5], dtype=np.float32)
    outs = _outs(2, np.float32, idt)
    rc, ng, info = _call(src, 1, rsa.F32, 1, outs, ib)
    assert rc == 0 and ng == 1 and info.route == rsa.GROUP_TRIVIAL and info.sort.early_exit == 1
    inv, keys, counts, first = outs
    assert inv[0] == 0 and keys[0] == np.float32(-3.5) and counts[0] == 1 and first[0] == 0
    assert all(o[1] == FILL for o in outs)   # nothing past element 0
    inv, keys, counts, first, _ = rsa.radix_sort_group_host(src, rsa.F32, keys=True, counts=True, first=True, idx_dtype=idt)
    assert list(inv) == [0] and list(keys) == [np.float32(-3.5)] and list(counts) == [1] and list(first) == [0]
    inv, keys, counts, first, _ = rsa.radix_sort_group_host(src, rsa.F32)
    assert list(inv) == [0] and keys is None and counts is None and first is None


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.zeros(4, dtype=np.uint32)
    outs = _outs(4)
    for device in (False, True):
        rc, _, _ = _call(a, 4, rsa.U32, 0, outs, 3, device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _, _ = _call(a, 4, 99, 0, outs, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _, _ = _call(a, 4, rsa.U32, 2, outs, 4, device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _, _ = _call(a, 4, rsa.U32, 0, outs, 4, device, ng_null=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _, _ = _call(a, 4, rsa.U32, 0, outs, 4, device, src_null=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            # (a dummy pointer: the call must fail before any device work)
            rc, _, _ = _call(a, 1 << 32, rsa.U8, 0, outs, 4, device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and _untouched(outs)


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    src = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_group_host(src, rsa.U32, keys=True, counts=True, first=True)
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_group_host(src, rsa.U32)
    for device in (False, True):
        outs = _outs(4)
        rc, _, _ = _call(src, 4, rsa.U32, 0, outs, 4, device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
        assert list(src) == [3, 1, 3, 2] and _untouched(outs)
    one = _outs(1)
    rc, _, _ = _call(src, 1, rsa.U32, 0, one, 4, device=True)     # the device form needs the device for its stores
    assert rc == -2 and _untouched(one)
