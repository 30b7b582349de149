"""Expected values and call helpers for the rsx_sort_lex tests (test_lex_cpu.py, test_gpu_lex.py, test_gpu_lex_bounds.py).

The expected permutation never comes from the code under test: `want_perm` chains the ORACLE's stable rank sort
(oracle_lib.oracle_rank, the C restatement of radix_sort_rank) over the columns from the last to the first, which is the
definition of an LSD ordering by several keys.  `want_groups` restates the grouping rule of include/rsx.h from its text."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import radix_sorting_amd as rsa

NP_VIEW = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def want_perm(cols, dtypes, orders=None):
    """Start with the identity; for each column from the last to the first: perm = perm[oracle_rank(col[perm])]."""
    orders = [ol.ASC] * len(cols) if orders is None else orders
    n = np.asarray(cols[0]).size
    perm = np.arange(n, dtype=np.int64)
    for col, dt, order in reversed(list(zip(cols, dtypes, orders))):
        bits = np.ascontiguousarray(col, dtype=ol.NP_BITS[dt])
        perm = perm[ol.oracle_rank(bits[perm], dt, 4, order)[0].astype(np.int64)]
    return perm


def lexsort_perm(cols, dtypes, orders=None):
    """The same order by np.lexsort over the derived keys (its LAST key is the primary one: the columns go in reversed)."""
    orders = [ol.ASC] * len(cols) if orders is None else orders
    keys = [ol.kdf_keys(np.ascontiguousarray(c, dtype=ol.NP_BITS[dt]), dt, o) for c, dt, o in zip(cols, dtypes, orders)]
    return np.lexsort(keys[::-1]).astype(np.int64)


def want_groups(dtypes, P):
    """[(first_col, ncols, key_bytes, sorted_as)], group 0 first: walk from the LAST column towards column 0, a column joins
    the current group while the group's bytes plus its own are at most P; a column wider than P is a group of its own."""
    groups, end, size = [], len(dtypes), 0

    def emit(first):
        lone0 = not groups and end - first == 1
        groups.append((first, end - first, size, dtypes[first] if lone0 else ol.U16 if size <= 2 else ol.U32 if size <= 4 else ol.U64))

    for ci in range(len(dtypes) - 1, -1, -1):
        w = ol.DTYPE_SIZE[dtypes[ci]]
        if size and size + w > P:
            emit(ci + 1)
            end, size = ci + 1, 0
        size += w
    emit(0)
    return groups


def lex_cols(ptrs, dtypes, orders=None):
    orders = [ol.ASC] * len(ptrs) if orders is None else orders
    arr = (rsa.LexCol * max(len(ptrs), 1))()
    for i, (p, dt, o) in enumerate(zip(ptrs, dtypes, orders)):
        arr[i].data, arr[i].dtype, arr[i].order = p, dt, o
    return arr


def call_host(arr, ncols, n, out, idx_bytes):
    """rsx_sort_lex as the C ABI has it: (return code, message, info)."""
    info = rsa.LexInfo()
    rc = rsa.lib().rsx_sort_lex(arr, ncols, n, None if out is None else out.ctypes.data, idx_bytes, C.byref(info))
    return rc, rsa.lib().rsx_last_error().decode(), info


def call_device_raw(arr, ncols, n, out_ptr, idx_bytes, stream=None):
    info = rsa.LexInfo()
    rc = rsa.lib().rsx_sort_lex_device(arr, ncols, n, out_ptr, idx_bytes, stream, C.byref(info))
    return rc, rsa.lib().rsx_last_error().decode(), info


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(NP_VIEW[a.itemsize]).copy()).cuda()
