"""rsx_sort_lex / rsx_sort_lex_device without a GPU: the yardstick itself (the oracle chain of tests/lex_lib.py against
np.lexsort), the grouping rule's restatement, the symbols and structure sizes, every argument error with its message, n == 0
and the host form's n == 1, and the refusal to do anything on the CPU (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import lex_lib as ll
import oracle_lib as ol
import radix_sorting_amd as rsa

ALL_DTYPES = list(range(10))


def _tie_heavy(n, dt, seed, bits=3):
    """Columns masked to a few low bits plus the sign / exponent end, so that ties across columns decide most places."""
    width = 8 * ol.DTYPE_SIZE[dt]
    mask = ((1 << bits) - 1) | (1 << (width - 1))
    return ol.splitmix_fill(n, dt, seed, mask)


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
def test_oracle_chain_equals_lexsort(order):
    """want_perm (the expected value of every GPU test) against np.lexsort over kdf_keys of the columns, reversed."""
    n = 389
    for first in ALL_DTYPES:
        dtypes = [first, ALL_DTYPES[(first + 3) % 10], ALL_DTYPES[(first + 7) % 10]]
        cols = [_tie_heavy(n, dt, 100 + 10 * first + j) for j, dt in enumerate(dtypes)]
        orders = [order, ol.ASC, ol.DESC if order == ol.ASC else ol.ASC]
        want = ll.want_perm(cols, dtypes, orders)
        assert np.array_equal(want, ll.lexsort_perm(cols, dtypes, orders)), ol.DTYPE_NAMES[first]
        assert np.array_equal(np.sort(want), np.arange(n))
    # one column: the oracle's ranks themselves
    col = _tie_heavy(n, ol.F32, 7)
    assert np.array_equal(ll.want_perm([col], [ol.F32], [order]), ol.oracle_rank(col, ol.F32, 4, order)[0])


def test_grouping_rule_restated():
    u8, u16, u32, u64 = ol.U8, ol.U16, ol.U32, ol.U64
    assert ll.want_groups([u32, u32], 4) == [(1, 1, 4, u32), (0, 1, 4, u32)]
    assert ll.want_groups([u32, u32], 8) == [(0, 2, 8, u64)]
    assert ll.want_groups([u16, u16], 4) == [(0, 2, 4, u32)]
    assert ll.want_groups([u16, u16], 1) == [(1, 1, 2, u16), (0, 1, 2, u16)]
    assert ll.want_groups([u8] * 4, 4) == [(0, 4, 4, u32)]
    assert ll.want_groups([u8] * 9, 8) == [(1, 8, 8, u64), (0, 1, 1, u16)]
    assert ll.want_groups([u8] * 9, 4) == [(5, 4, 4, u32), (1, 4, 4, u32), (0, 1, 1, u16)]
    assert ll.want_groups([u8, u16, u8], 4) == [(0, 3, 4, u32)]
    assert ll.want_groups([ol.I8, ol.F32], 4) == [(1, 1, 4, ol.F32), (0, 1, 1, u16)]
    assert ll.want_groups([ol.I8, ol.F32], 8) == [(0, 2, 5, u64)]
    assert ll.want_groups([u64, u32], 4) == [(1, 1, 4, u32), (0, 1, 8, u64)]
    assert ll.want_groups([ol.F64], 1) == [(0, 1, 8, ol.F64)]


def test_symbols_are_exported_and_bound():
    names = [n for n, _, _ in rsa.ABI]
    assert "rsx_sort_lex" in names and "rsx_sort_lex_device" in names
    lib = rsa.lib()
    assert len(lib.rsx_sort_lex.argtypes) == 6
    assert len(lib.rsx_sort_lex_device.argtypes) == 7
    assert C.sizeof(rsa.LexCol) == 16
    assert C.sizeof(rsa.LexGroup) == 32
    assert C.sizeof(rsa.LexInfo) == 16 + 16 * 32
    assert rsa.LEX_MAX_COLS == 16
    assert callable(rsa.radix_sort_lex) and callable(rsa.radix_sort_lex_host)


def _call(arr, ncols, n, out, idx_bytes, device):
    if device:
        return ll.call_device_raw(arr, ncols, n, None if out is None else out.ctypes.data, idx_bytes)
    return ll.call_host(arr, ncols, n, out, idx_bytes)


@pytest.mark.parametrize("device", [False, True])
def test_bad_arguments_are_rejected(device):
    a = np.arange(4, dtype=np.uint32)
    b = np.arange(4, dtype=np.uint16)
    out = np.full(4, 0xA5A5A5A5, dtype=np.uint32)
    who = "rsx_sort_lex_device" if device else "rsx_sort_lex"
    good = ll.lex_cols([a.ctypes.data, b.ctypes.data], [rsa.U32, rsa.U16])
    cases = [
        (good, 0, 4, out, 4, "ncols = 0"),
        (ll.lex_cols([a.ctypes.data] * 17, [rsa.U32] * 17), 17, 4, out, 4, "ncols = 17"),
        (None, 2, 4, out, 4, "cols is NULL"),
        (ll.lex_cols([a.ctypes.data, None], [rsa.U32, rsa.U16]), 2, 4, out, 4, "column 1 is NULL"),
        (ll.lex_cols([a.ctypes.data, b.ctypes.data], [rsa.U32, 10]), 2, 4, out, 4, "column 1: unknown dtype 10"),
        (ll.lex_cols([a.ctypes.data, b.ctypes.data], [rsa.U32, rsa.U16], [2, 0]), 2, 4, out, 4, "column 0: unknown order 2"),
        (good, 2, 4, out, 3, "idx_bytes = 3"),
        (good, 2, 4, out, 2, "idx_bytes = 2"),
        (good, 2, 4, None, 4, "the output is NULL"),
    ]
    if C.sizeof(C.c_size_t) == 8:
        cases.append((good, 2, (1 << 32) + 1, out, 4, "does not fit"))
    for arr, ncols, n, o, ib, msg in cases:
        rc, err, info = _call(arr, ncols, n, o, ib, device)
        assert rc == -1, (msg, rc, err)
        assert err.startswith(who + ":") and msg in err, (msg, err)
        assert info.ngroups == 0
    assert list(a) == [0, 1, 2, 3] and list(b) == [0, 1, 2, 3] and np.all(out == 0xA5A5A5A5)


@pytest.mark.parametrize("device", [False, True])
def test_n_zero_needs_no_device(device):
    a = np.array([5, 3, 9], dtype=np.uint32)
    out = np.full(2, 0xC3C3C3C3, dtype=np.uint32)
    arr = ll.lex_cols([a.ctypes.data, a.ctypes.data], [rsa.U32, rsa.F32], [0, 1])
    rc, err, info = _call(arr, 2, 0, out, 4, device)
    assert rc == 0, err
    assert (info.ncols, info.ngroups, info.early_exit) == (2, 0, 1) and 1 <= info.pack_bytes <= 8
    assert np.all(out == 0xC3C3C3C3) and list(a) == [5, 3, 9]
    # (no buffers at all)
    rc, err, info = _call(ll.lex_cols([None], [rsa.U8]), 1, 0, None, 8, device)
    assert rc == 0 and info.early_exit == 1


def test_host_form_n_one_needs_no_device():
    a = np.array([5], dtype=np.uint64)
    for idt in (np.uint32, np.uint64):
        out = np.full(2, 0xC3, dtype=idt)
        rc, err, info = ll.call_host(ll.lex_cols([a.ctypes.data, a.ctypes.data], [rsa.U64, rsa.I64]), 2, 1, out, out.itemsize)
        assert rc == 0, err
        assert (info.ngroups, info.early_exit) == (0, 1)
        assert list(out) == [0, 0xC3] and a[0] == 5
    idx, info = rsa.radix_sort_lex_host([a], [rsa.U64])
    assert list(idx) == [0] and info.early_exit == 1


def test_pack_bytes_switch_is_read(monkeypatch):
    a = np.zeros(1, dtype=np.uint8)
    arr = ll.lex_cols([a.ctypes.data], [rsa.U8])
    out = np.zeros(1, dtype=np.uint32)
    try:
        for value, want in (("1", 1), ("8", 8), ("5", 5), ("0", 4), ("9", 4), ("x", 4), (None, 4)):
            if value is None:
                monkeypatch.delenv("RSX_LEX_PACK_BYTES", raising=False)
            else:
                monkeypatch.setenv("RSX_LEX_PACK_BYTES", value)
            rsa.reload_env()
            rc, err, info = ll.call_host(arr, 1, 0, out, 4)
            assert rc == 0 and info.pack_bytes == want, (value, info.pack_bytes)
    finally:
        monkeypatch.delenv("RSX_LEX_PACK_BYTES", raising=False)
        rsa.reload_env()


@pytest.mark.skipif(rsa.device_count() > 0, reason="a GPU is present")
def test_no_cpu_fallback_without_gpu():
    a = np.array([3, 1, 3, 2], dtype=np.uint32)
    b = np.array([1, 0, 0, 1], dtype=np.uint8)
    out = np.full(4, 0xC3, dtype=np.uint64)
    arr = ll.lex_cols([a.ctypes.data, b.ctypes.data], [rsa.U32, rsa.U8])
    for device in (False, True):
        rc, err, info = _call(arr, 2, 4, out, 8, device)
        assert rc == -2 and "no gfx950" in err
    with pytest.raises(rsa.RsxError, match="no gfx950"):
        rsa.radix_sort_lex_host([a, b], [rsa.U32, rsa.U8])
    assert list(a) == [3, 1, 3, 2] and list(b) == [1, 0, 0, 1] and list(out) == [0xC3] * 4
