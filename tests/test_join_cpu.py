"""rsx_sort_join[_device] and rsx_join_pairs[_device] without a GPU: the symbols, every argument check of both phases, the trivial
cases on host pointers, the Python wrappers' own checks, and the refusal to do anything else on the CPU (there is no CPU path)
with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import radix_sorting_amd as rsa

FILL = 0xA5A5A5A5
P = lambda a: None if a is None else a.ctypes.data


def _join(left, n, right, m, dtype, order, start, count, perm, idx_bytes, flags=0, device=False, null_left=False, null_right=False, null_pairs=False):
    lib = rsa.lib()
    info, pairs = rsa.JoinInfo(), C.c_uint64(FILL)
    lp = None if null_left else P(left)
    rp = None if null_right else P(right)
    pp = None if null_pairs else C.byref(pairs)
    if device:
        rc = lib.rsx_sort_join_device(lp, n, rp, m, dtype, order, P(start), P(count), P(perm), idx_bytes, flags, None, pp, C.byref(info))
    else:
        rc = lib.rsx_sort_join(lp, n, rp, m, dtype, order, P(start), P(count), P(perm), idx_bytes, flags, pp, C.byref(info))
    return rc, int(pairs.value), info


def _pairs(start, count, perm, n, m, idx_bytes, flags, out_left, out_right, capacity, device=False, null_pairs=False):
    lib = rsa.lib()
    pairs = C.c_uint64(FILL)
    pp = None if null_pairs else C.byref(pairs)
    if device:
        rc = lib.rsx_join_pairs_device(P(start), P(count), P(perm), n, m, idx_bytes, flags, P(out_left), P(out_right), capacity, None, pp)
    else:
        rc = lib.rsx_join_pairs(P(start), P(count), P(perm), n, m, idx_bytes, flags, P(out_left), P(out_right), capacity, pp)
    return rc, int(pairs.value)


def _fill(size, dtype=np.uint32):
    return np.full(size, FILL, dtype=dtype)


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    for name in ("rsx_sort_join", "rsx_sort_join_device", "rsx_join_pairs", "rsx_join_pairs_device"):
        assert name in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_join.argtypes) == 13 and len(lib.rsx_sort_join_device.argtypes) == 14
    assert len(lib.rsx_join_pairs.argtypes) == 11 and len(lib.rsx_join_pairs_device.argtypes) == 12
    assert C.sizeof(rsa.JoinInfo) == 80 and rsa.JoinInfo.table_bytes.offset == 16 and rsa.JoinInfo.sort.offset == 24
    assert (rsa.JOIN_TRIVIAL, rsa.JOIN_TABLE, rsa.JOIN_SEARCH, rsa.JOIN_MERGE) == (0, 1, 2, 3)
    assert rsa.JOIN_LEFT == 1 and rsa.JOIN_ROW_TILE == 1024 and rsa.JOIN_EXPAND_TILE == 4096


def test_join_bad_arguments_are_rejected():
    lib = rsa.lib()
    a, b = np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    start, count, perm = _fill(4), _fill(4), _fill(2)
    for device in (False, True):
        for kw, what in ((dict(dtype=99), b"bad argument"), (dict(order=2), b"bad argument"), (dict(flags=2), b"bad argument"),
                         (dict(null_left=True), b"bad argument"), (dict(null_right=True), b"bad argument"), (dict(null_pairs=True), b"bad argument"),
                         (dict(idx_bytes=3), b"idx_bytes"), (dict(idx_bytes=0), b"idx_bytes")):
            args = dict(dtype=rsa.U32, order=0, idx_bytes=4)
            args.update(kw)
            rc, _, _ = _join(a, 4, b, 2, args.pop("dtype"), args.pop("order"), start, count, perm, args.pop("idx_bytes"), device=device, **args)
            assert rc == -1 and what in lib.rsx_last_error(), (device, kw, lib.rsx_last_error())
        if C.sizeof(C.c_size_t) == 8:
            rc, _, _ = _join(a, (1 << 32) + 1, b, 2, rsa.U8, 0, None, None, None, 4, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
            rc, _, _ = _join(a, 4, b, (1 << 32) + 1, rsa.U8, 0, None, None, None, 4, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert not a.any() and not b.any()
    assert (start == FILL).all() and (count == FILL).all() and (perm == FILL).all()


def test_pairs_bad_arguments_are_rejected():
    lib = rsa.lib()
    start, count, perm = np.zeros(3, dtype=np.uint32), np.ones(3, dtype=np.uint32), np.arange(2, dtype=np.uint32)
    ol_, or_ = _fill(8), _fill(8)
    for device in (False, True):
        rc, _ = _pairs(start, count, perm, 3, 2, 4, 0, None, None, 8, device=device)
        assert rc == -1 and b"both outputs" in lib.rsx_last_error()
        rc, _ = _pairs(start, count, perm, 3, 2, 3, 0, ol_, or_, 8, device=device)
        assert rc == -1 and b"idx_bytes" in lib.rsx_last_error()
        rc, _ = _pairs(start, count, perm, 3, 2, 4, 2, ol_, or_, 8, device=device)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _pairs(start, None, perm, 3, 2, 4, 0, ol_, or_, 8, device=device)          # no counts
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _pairs(None, count, perm, 3, 2, 4, 0, ol_, or_, 8, device=device)           # out_right wants start ...
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _pairs(start, count, None, 3, 2, 4, 0, ol_, or_, 8, device=device)          # ... and right_perm
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        rc, _ = _pairs(start, count, perm, 3, 2, 4, 0, ol_, or_, 8, device=device, null_pairs=True)
        assert rc == -1 and b"bad argument" in lib.rsx_last_error()
        if C.sizeof(C.c_size_t) == 8:
            rc, _ = _pairs(start, count, perm, (1 << 32) + 1, 2, 4, 0, ol_, or_, 8, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
            rc, _ = _pairs(start, count, perm, 3, (1 << 32) + 1, 4, 0, ol_, or_, 8, device=device)
            assert rc == -1 and b"does not fit" in lib.rsx_last_error()
    assert (ol_ == FILL).all() and (or_ == FILL).all()


@pytest.mark.parametrize("idx", [np.uint32, np.uint64])
def test_join_trivial_cases_on_host_pointers_need_no_device(idx):
    ib = np.dtype(idx).itemsize
    left, right = np.array([5, 3, 9], dtype=np.uint32), np.array([4, 4], dtype=np.uint32)
    # no right rows: nothing matches
    start, count, perm = _fill(4, idx), _fill(4, idx), _fill(3, idx)
    rc, pairs, info = _join(left, 3, right, 0, rsa.U32, 0, start, count, perm, ib, null_right=True)
    assert rc == 0 and pairs == 0 and info.route == rsa.JOIN_TRIVIAL and info.key_bytes == 4
    assert list(count[:3]) == [0, 0, 0] and count[3] == idx(FILL) and start[3] == idx(FILL) and (perm == idx(FILL)).all()
    rc, pairs, _ = _join(left, 3, right, 0, rsa.U32, 1, None, None, None, ib, flags=rsa.JOIN_LEFT)
    assert rc == 0 and pairs == 3
    # no left rows: right_perm is an iota
    rc, pairs, info = _join(left, 0, right, 2, rsa.U32, 0, start, count, perm, ib, flags=rsa.JOIN_LEFT, null_left=True)
    assert rc == 0 and pairs == 0 and info.route == rsa.JOIN_TRIVIAL
    assert list(perm[:2]) == [0, 1] and perm[2] == idx(FILL) and count[3] == idx(FILL)
    assert list(left) == [5, 3, 9] and list(right) == [4, 4]
    # the device form needs no device where that leaves nothing to write
    rc, pairs, info = _join(left, 0, right, 2, rsa.U32, 0, start, count, None, ib, device=True)
    assert rc == 0 and pairs == 0 and info.route == rsa.JOIN_TRIVIAL
    rc, pairs, info = _join(left, 3, right, 0, rsa.U32, 0, None, None, perm, ib, flags=rsa.JOIN_LEFT, device=True)
    assert rc == 0 and pairs == 3 and info.route == rsa.JOIN_TRIVIAL


def test_pairs_trivial_cases_on_host_pointers_need_no_device():
    lib = rsa.lib()
    start, perm = np.zeros(3, dtype=np.uint32), np.arange(2, dtype=np.uint32)
    ol_, or_ = _fill(8), _fill(8)
    for device in (False, True):
        rc, pairs = _pairs(start, np.zeros(3, dtype=np.uint32), perm, 0, 2, 4, rsa.JOIN_LEFT, ol_, or_, 8, device=device)     # no rows
        assert rc == 0 and pairs == 0
    rc, pairs = _pairs(start, np.zeros(3, dtype=np.uint32), perm, 3, 2, 4, 0, ol_, or_, 8)     # no matches, inner: no pairs
    assert rc == 0 and pairs == 0
    rc, pairs = _pairs(start, np.array([2, 0, 7], dtype=np.uint32), perm, 3, 2, 4, 0, ol_, or_, 8)     # 9 pairs, room for 8
    assert rc == -1 and pairs == 9 and b"does not fit" in lib.rsx_last_error()
    rc, pairs = _pairs(start, np.array([2, 0, 7], dtype=np.uint32), perm, 3, 2, 4, rsa.JOIN_LEFT, ol_, None, 9)
    assert (rc == -1 and pairs == 10 and b"does not fit" in lib.rsx_last_error())
    rc, pairs = _pairs(start, np.array([1 << 62, 1 << 62, 5], dtype=np.uint64), np.arange(2, dtype=np.uint64), 3, 2, 8, 0,
                       np.zeros(1, dtype=np.uint64), None, 1 << 40)
    assert rc == -1 and pairs == (1 << 63) + 5
    assert (ol_ == FILL).all() and (or_ == FILL).all()


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    left, right = np.array([3, 1, 3, 2], dtype=np.uint32), np.array([2, 9], dtype=np.uint32)
    start, count, perm = _fill(4), _fill(4), _fill(2)
    for device in (False, True):
        rc, pairs, _ = _join(left, 4, right, 2, rsa.U32, 0, start, count, perm, 4, device=device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
        rc, pairs, _ = _join(left, 1, right, 1, rsa.U32, 0, None, None, None, 4, device=device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    rc, _, _ = _join(left, 4, right, 0, rsa.U32, 0, start, count, None, 4, device=True)     # zeros to write into "device" memory
    assert rc == -2
    ol_, or_ = _fill(8), _fill(8)
    for device in (False, True):
        rc, pairs = _pairs(np.zeros(4, dtype=np.uint32), np.array([1, 0, 1, 0], dtype=np.uint32), np.arange(2, dtype=np.uint32), 4, 2, 4, 0, ol_, or_, 8,
                           device=device)
        assert rc == -2 and b"no gfx950" in rsa.lib().rsx_last_error()
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_join_host(left, right, rsa.U32)
    assert list(left) == [3, 1, 3, 2] and list(right) == [2, 9]
    assert (start == FILL).all() and (count == FILL).all() and (perm == FILL).all() and (ol_ == FILL).all() and (or_ == FILL).all()


def test_python_wrappers_check_their_arguments():
    left = np.array([3, 1, 3, 2], dtype=np.uint32)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_join_host(left, np.array([1], dtype=np.uint32), rsa.U64)
    with pytest.raises(rsa.RsxError, match="key type"):
        rsa.radix_sort_join_host(left, np.array([1], dtype=np.uint64), rsa.U32)
    with pytest.raises(rsa.RsxError, match="neither"):
        rsa.radix_sort_join_host(left, left, rsa.U32, how="outer")
    with pytest.raises(rsa.RsxError, match="neither"):
        rsa.radix_sort_join(None, None, how="right")
    li, ri, info, st, ct, pm = rsa.radix_sort_join_host(left, np.zeros(0, dtype=np.uint32), rsa.U32)     # nothing matches: no device needed
    assert info.route == rsa.JOIN_TRIVIAL and list(ct) == [0, 0, 0, 0] and pm.size == 0
    li, ri, info, st, ct, pm = rsa.radix_sort_join_host(np.zeros(0, dtype=np.uint32), left, rsa.U32)
    assert li.size == 0 and ri.size == 0 and list(pm) == [0, 1, 2, 3]
