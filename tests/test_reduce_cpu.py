"""rsx_sort_reduce / rsx_sort_reduce_device without a GPU: the symbols, every RSX_EINVAL case of the header, n == 0, n == 1 on host
pointers without a device, the Python wrappers' own checks, and the refusal to do anything else on the CPU (there is no CPU path)
with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xA5


def _outs(n, kdt=np.uint32, vdt=np.uint32, ib=4):
    return [np.full(n, FILL, dtype=kdt), np.full(n, FILL, dtype=np.uint32 if ib == 4 else np.uint64), np.full(n, FILL, dtype=np.uint64),
            np.full(n, FILL, dtype=vdt), np.full(n, FILL, dtype=vdt)]


def _call(keys, vals, n, dtype, order, vdtype, ops, outs, idx_bytes=4, device=False, ng=True):
    lib = rsa.lib()
    info = rsa.ReduceInfo()
    p = lambda a: None if a is None else a.ctypes.data
    groups = C.c_size_t(77)
    ngp = C.byref(groups) if ng else None
    k, c, s, mn, mx = outs
    if device:
        rc = lib.rsx_sort_reduce_device(p(keys), p(vals), n, dtype, order, vdtype, ops, p(k), p(c), idx_bytes, p(s), p(mn), p(mx), None, ngp,
                                        C.byref(info))
    else:
        rc = lib.rsx_sort_reduce(p(keys), p(vals), n, dtype, order, vdtype, ops, p(k), p(c), idx_bytes, p(s), p(mn), p(mx), ngp, C.byref(info))
    return rc, groups.value, info


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_reduce" in names and "rsx_sort_reduce_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_reduce.argtypes) == 15 and len(lib.rsx_sort_reduce_device.argtypes) == 16
    assert C.sizeof(rsa.ReduceInfo) == C.sizeof(rsa.GroupInfo) == 72     # rsx_info (52), 2 x u32, padding to 8, u64
    assert (rsa.REDUCE_TRIVIAL, rsa.REDUCE_CELLS_LDS, rsa.REDUCE_CELLS_GLOBAL, rsa.REDUCE_SORT) == (0, 1, 2, 3)
    assert (rsa.REDUCE_SUM, rsa.REDUCE_MIN, rsa.REDUCE_MAX) == (1, 2, 4)


def test_bad_arguments_are_rejected():
    lib = rsa.lib()
    a = np.array([3, 1, 3, 2], dtype=np.uint32)
    v = np.array([1, 2, 3, 4], dtype=np.uint32)
    outs = _outs(4)
    k, c, s, mn, mx = outs
    err = lambda: lib.rsx_last_error()
    for device in (False, True):
        rc, _, _ = _call(a, v, 4, 99, 0, rsa.U32, 7, outs, device=device)
        assert rc == -1 and b"bad argument" in err()
        rc, _, _ = _call(a, v, 4, rsa.U32, 2, rsa.U32, 7, outs, device=device)
        assert rc == -1 and b"bad argument" in err()
        rc, _, _ = _call(None, v, 4, rsa.U32, 0, rsa.U32, 7, outs, device=device)
        assert rc == -1 and b"bad argument" in err()
        rc, _, _ = _call(a, None, 4, rsa.U32, 0, rsa.U32, 7, outs, device=device)
        assert rc == -1 and b"bad argument" in err()
        rc, _, _ = _call(a, v, 4, rsa.U32, 0, rsa.U32, 7, outs, device=device, ng=False)
        assert rc == -1 and b"bad argument" in err()
        for narrow in (rsa.U8, rsa.I8, rsa.U16, rsa.I16, 99):
            rc, _, _ = _call(a, v, 4, rsa.U32, 0, narrow, 7, outs, device=device)
            assert rc == -1 and b"val_dtype" in err()
        rc, _, _ = _call(a, v, 4, rsa.U32, 0, rsa.U32, 8, outs, device=device)
        assert rc == -1 and b"ops" in err()
        # an ops bit whose output is NULL, an output whose bit is clear: each of the three
        for bit, at in ((1, 2), (2, 3), (4, 4)):
            missing = list(outs)
            missing[at] = None
            rc, _, _ = _call(a, v, 4, rsa.U32, 0, rsa.U32, 7, missing, device=device)
            assert rc == -1 and b"do not agree" in err()
            rc, _, _ = _call(a, v, 4, rsa.U32, 0, rsa.U32, 7 & ~bit, outs, device=device)
            assert rc == -1 and b"do not agree" in err()
        rc, _, _ = _call(a, v, 4, rsa.U32, 0, rsa.U32, 7, outs, idx_bytes=3, device=device)
        assert rc == -1 and b"idx_bytes" in err()
        if C.sizeof(C.c_size_t) == 8:
            rc, _, _ = _call(a, v, (1 << 32) + 1, rsa.U8, 0, rsa.U32, 7, outs, device=device)     # a count may be n itself
            assert rc == -1 and b"does not fit" in err()
    assert list(a) == [3, 1, 3, 2] and list(v) == [1, 2, 3, 4]
    for o in outs:
        assert (o == FILL).all()


@pytest.mark.parametrize("device", [False, True])
def test_no_elements_need_no_device(device):
    a = np.array([5], dtype=np.uint32)
    outs = _outs(1)
    rc, g, info = _call(a, a, 0, rsa.U32, 0, rsa.U32, 7, outs, device=device)
    assert rc == 0 and g == 0 and info.sort.early_exit == 1 and info.route == rsa.REDUCE_TRIVIAL
    rc, g, _ = _call(None, None, 0, rsa.F64, 1, rsa.F64, 0, [None] * 5, idx_bytes=8, device=device)     # nothing at all is fine with n == 0
    assert rc == 0 and g == 0
    for o in outs:
        assert (o == FILL).all()


def test_one_element_on_host_pointers_needs_no_device():
    cases = ((rsa.U32, np.uint32, 0xFFFFFFFF, 0xFFFFFFFF), (rsa.I32, np.int32, -5, (1 << 64) - 5), (rsa.U64, np.uint64, (1 << 63) + 1, (1 << 63) + 1),
             (rsa.I64, np.int64, -7, (1 << 64) - 7), (rsa.F32, np.float32, -2.5, None), (rsa.F64, np.float64, 1e300, None))
    for vdt, npt, value, want_sum in cases:
        key = np.array([0x80000001], dtype=np.uint32)
        val = np.array([value], dtype=npt)
        for ib in (4, 8):
            outs = _outs(1, vdt=npt, ib=ib)
            rc, g, info = _call(key, val, 1, rsa.I32, 1, vdt, 7, outs, idx_bytes=ib)
            assert rc == 0 and g == 1 and info.sort.early_exit == 1 and info.route == rsa.REDUCE_TRIVIAL
            k, c, s, mn, mx = outs
            assert k[0] == key[0] and c[0] == 1 and mn[0] == val[0] and mx[0] == val[0]
            if want_sum is None:
                assert s.view(np.float64)[0] == float(val[0])
            else:
                assert int(s[0]) == want_sum
        # outputs left out: keys alone, with ops == 0
        outs = _outs(1, vdt=npt)
        rc, g, _ = _call(key, val, 1, rsa.I32, 0, vdt, 0, [outs[0], None, None, None, None])
        assert rc == 0 and g == 1 and outs[0][0] == key[0] and (outs[1] == FILL).all()
    k, c, s, mn, mx, info = rsa.radix_sort_reduce_host(np.array([9], dtype=np.uint16), np.array([-3], dtype=np.int64), rsa.U16, rsa.I64, min=True, max=True,
                                                     counts=True)
    assert list(k) == [9] and list(c) == [1] and int(s[0]) == (1 << 64) - 3 and list(mn) == [-3] and list(mx) == [-3]


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    a = np.array([3, 1, 3, 2], dtype=np.uint32)
    v = np.array([1, 2, 3, 4], dtype=np.uint32)
    outs = _outs(4)
    for device in (False, True):
        for n in ((4, 2, 1) if device else (4, 2)):       # (one element on DEVICE pointers needs the device for its copies)
            rc, g, _ = _call(a, v, n, rsa.U32, 0, rsa.U32, 7, outs, device=device)
            assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_reduce_host(a, v, rsa.U32, rsa.U32)
    assert list(a) == [3, 1, 3, 2] and list(v) == [1, 2, 3, 4]
    for o in outs:
        assert (o == FILL).all()


def test_python_wrappers_check_their_arguments():
    a = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="do not match"):
        rsa.radix_sort_reduce_host(a, a, rsa.U64, rsa.U32)
    with pytest.raises(rsa.RsxError, match="do not match"):
        rsa.radix_sort_reduce_host(a, a, rsa.U32, rsa.U64)
    with pytest.raises(rsa.RsxError, match="do not match"):
        rsa.radix_sort_reduce_host(a, a[:3], rsa.U32, rsa.U32)
    with pytest.raises(rsa.RsxError, match="room"):
        rsa.radix_sort_reduce_host(a, a, rsa.U32, rsa.U32, sum=np.zeros(3, dtype=np.uint64))
    with pytest.raises(rsa.RsxError, match="val_dtype"):
        rsa.radix_sort_reduce_host(a.view(np.uint16)[:4], np.zeros(4, dtype=np.uint16), rsa.U16, rsa.U16)
    k, c, s, mn, mx, info = rsa.radix_sort_reduce_host(a[:0], a[:0], rsa.U32, rsa.U32, counts=True)
    assert k.size == 0 and c.size == 0 and s.size == 0 and mn is None and mx is None and info.route == rsa.REDUCE_TRIVIAL
