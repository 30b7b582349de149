"""radix_sorting_amd -- MI355X-native LSD radix sort behind eloj/radix-sorting's surface.

The product is ``librsx.so`` (hand-written HIP for gfx950, C ABI in
``include/rsx.h``) plus the C++ template headers in ``include/``.  This Python
package is only the thin host-side doorway used by the tests, ``bench.py`` and
the multi-GPU driver: it binds the C ABI with ctypes and passes torch tensors'
``data_ptr()`` / current stream straight through.  PyTorch is plumbing here
(device memory, streams, ``torch.distributed``); no sorting happens in Python
and there is no CPU fallback -- a missing library or GPU raises.

Function names and argument meaning follow the reference
(``radix_sort(src, aux, n, kdf)`` radix_sort.hpp:98-99,
``radix_sort_rank(src, index_buffer, n, kdf)`` radix_sort_rank.hpp:97-98).
"""
import ctypes as C
import threading
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (RSX_LIB: another build of the library, for A/B measurements of compile-time variants inside one gpurun call)
LIB_PATH = os.environ.get("RSX_LIB") or os.path.join(_HERE, "librsx.so")

# rsx_dtype (include/rsx.h)
U8, U16, U32, U64, I8, I16, I32, I64, F32, F64 = range(10)
DTYPE_SIZE = [1, 2, 4, 8, 1, 2, 4, 8, 4, 8]
ASCENDING, DESCENDING = 0, 1


class RsxError(RuntimeError):
    pass


class Profile(C.Structure):
    """rsx_profile: HIP-event kernel timings collected between profile_begin() and profile_end()."""
    _fields_ = [("hist_ms", C.c_double), ("scatter_ms", C.c_double), ("hist_launches", C.c_uint64),
                ("scatter_launches", C.c_uint64), ("hist_bytes", C.c_uint64), ("scatter_bytes", C.c_uint64),
                ("leaf_ms", C.c_double), ("leaf_launches", C.c_uint64), ("leaf_bytes", C.c_uint64),
                ("narrow_ms", C.c_double), ("narrow_launches", C.c_uint64), ("narrow_bytes", C.c_uint64),
                ("called_off_ms", C.c_double), ("called_off_launches", C.c_uint64)]


class Info(C.Structure):
    """rsx_info: what the front half of rs_sort_main decided (radix_sort.hpp:48-80)."""
    _fields_ = [("key_bytes", C.c_uint32), ("ncols", C.c_uint32), ("cols", C.c_uint32 * 8),
                ("early_exit", C.c_uint32), ("result_in_aux", C.c_uint32), ("hybrid", C.c_uint32)]

    def kept_columns(self):
        return [int(self.cols[i]) for i in range(self.ncols)]


# rsx_unique_info.route
UNIQUE_TRIVIAL, UNIQUE_BITMAP_LDS, UNIQUE_BITMAP_GLOBAL, UNIQUE_TABLE, UNIQUE_SORT = range(5)


class UniqueInfo(C.Structure):
    """rsx_unique_info: the route rsx_sort_unique* took and what the front half of the sort decided."""
    _fields_ = [("sort", Info), ("route", C.c_uint32), ("varying_bits", C.c_uint32), ("table_bytes", C.c_uint64)]


# rsx_group_info.route
GROUP_TRIVIAL, GROUP_RANK_LDS, GROUP_RANK_GLOBAL, GROUP_TABLE, GROUP_SORT = range(5)


class GroupInfo(C.Structure):
    """rsx_group_info: the route rsx_sort_group* took and what the front half of the sort decided."""
    _fields_ = [("sort", Info), ("route", C.c_uint32), ("varying_bits", C.c_uint32), ("table_bytes", C.c_uint64)]


# rsx_reduce_info.route, the bits of rsx_sort_reduce*'s ops
REDUCE_TRIVIAL, REDUCE_CELLS_LDS, REDUCE_CELLS_GLOBAL, REDUCE_SORT = range(4)
REDUCE_SUM, REDUCE_MIN, REDUCE_MAX = 1, 2, 4


class ReduceInfo(C.Structure):
    """rsx_reduce_info: the route rsx_sort_reduce* took and what the front half of the sort decided."""
    _fields_ = [("sort", Info), ("route", C.c_uint32), ("varying_bits", C.c_uint32), ("table_bytes", C.c_uint64)]


# rsx_rankdata_info.route
RANKDATA_TRIVIAL, RANKDATA_TABLE, RANKDATA_COUNT16, RANKDATA_SORT = range(4)


class RankdataInfo(C.Structure):
    """rsx_rankdata_info: the route rsx_sort_rankdata* took and what the front half of the sort decided."""
    _fields_ = [("sort", Info), ("route", C.c_uint32), ("varying_bits", C.c_uint32), ("table_bytes", C.c_uint64)]


# rsx_topk_info.route
TOPK_TRIVIAL, TOPK_SELECT, TOPK_SORT = range(3)


class TopkInfo(C.Structure):
    """rsx_topk_info: the route rsx_sort_topk* took and what it found about the k-th key."""
    _fields_ = [("route", C.c_uint32), ("key_bytes", C.c_uint32), ("input_reads", C.c_uint32), ("digit_passes", C.c_uint32),
                ("n_less", C.c_uint64), ("n_equal", C.c_uint64), ("kth_key", C.c_uint64)]


# rsx_nth_info.route
NTH_TRIVIAL, NTH_SELECT, NTH_SORT = range(3)
NTH_MAX_SELECT_RANKS = 64


class NthInfo(C.Structure):
    """rsx_nth_info: the route rsx_sort_nth* took and how far its selection had to go."""
    _fields_ = [("route", C.c_uint32), ("key_bytes", C.c_uint32), ("input_reads", C.c_uint32), ("digit_passes", C.c_uint32),
                ("active_buckets", C.c_uint32), ("from_prefix", C.c_uint32), ("candidates", C.c_uint64)]


# rsx_locate_info.route, the search route's cut-off, rsx_sort_locate*'s flags
LOCATE_TRIVIAL, LOCATE_TABLE, LOCATE_SEARCH, LOCATE_SORT = range(4)
LOCATE_MAX_SEARCH_VALUES = 4096
LOCATE_BINS_BELOW = 1
# the search kernel's tile (keys) and the least number of tiles of a workgroup's share (radix_sorting_amd/csrc/rsx_locate_shape.hpp)
LOCATE_TILE, LOCATE_SHARE_TILES = 4096, 4


class LocateInfo(C.Structure):
    """rsx_locate_info: the route rsx_sort_locate* took, what its search looked like and what the inner sort of the keys reported."""
    _fields_ = [("route", C.c_uint32), ("key_bytes", C.c_uint32), ("input_reads", C.c_uint32), ("distinct_values", C.c_uint32),
                ("search_steps", C.c_uint32), ("counter_sets", C.c_uint32), ("sort", Info)]


# rsx_partition_info.route, the scatter route's cut-off, rsx_sort_partition*'s flag
PARTITION_TRIVIAL, PARTITION_SCATTER, PARTITION_SORT = range(3)
PARTITION_MAX_EDGES = 255             # the most the scatter route takes (RSX_PARTITION_MAX_EDGES=255)
PARTITION_DEFAULT_MAX_EDGES = 3       # ... and what it takes by default
PARTITION_BELOW = 1
# the placement's tile (keys), the least number of tiles of a workgroup's share and the default of RSX_PARTITION_BALLOT_PARTS
# (radix_sorting_amd/csrc/rsx_partition_shape.hpp)
PARTITION_TILE, PARTITION_SHARE_TILES, PARTITION_BALLOT_PARTS = 8192, 2, 7


class PartitionInfo(C.Structure):
    """rsx_partition_info: the route rsx_sort_partition* took, what its search and ranking looked like and what the inner locate and
    rank sort of the sort route reported."""
    _fields_ = [("route", C.c_uint32), ("key_bytes", C.c_uint32), ("input_reads", C.c_uint32), ("distinct_edges", C.c_uint32),
                ("search_steps", C.c_uint32), ("rank_form", C.c_uint32), ("shares", C.c_uint32), ("locate", LocateInfo), ("sort", Info)]


# rsx_join_info.route, rsx_sort_join* / rsx_join_pairs*' flag, the expansion's tiles (rows, pairs: radix_sorting_amd/csrc/rsx_join_shape.hpp)
JOIN_TRIVIAL, JOIN_TABLE, JOIN_SEARCH, JOIN_MERGE = range(4)
JOIN_LEFT = 1
JOIN_ROW_TILE, JOIN_EXPAND_TILE = 1024, 4096


class JoinInfo(C.Structure):
    """rsx_join_info: the route rsx_sort_join* took, what it saw of the right keys and what the inner sort of the right side reported."""
    _fields_ = [("route", C.c_uint32), ("key_bytes", C.c_uint32), ("varying_bits", C.c_uint32), ("left_sorted", C.c_uint32),
                ("table_bytes", C.c_uint64), ("sort", Info)]


LEX_MAX_COLS = 16


class LexCol(C.Structure):
    """rsx_lex_col: one key column of rsx_sort_lex* (column 0 is the most significant one)."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_uint32), ("order", C.c_uint32)]


class LexGroup(C.Structure):
    """rsx_lex_group: the columns that were packed into one key and what the inner sort of that key reported."""
    _fields_ = [("first_col", C.c_uint32), ("ncols", C.c_uint32), ("key_bytes", C.c_uint32), ("sorted_as", C.c_uint32),
                ("kept_cols", C.c_uint32), ("hybrid", C.c_uint32), ("in_order", C.c_uint32), ("pad", C.c_uint32)]


class LexInfo(C.Structure):
    """rsx_lex_info: how rsx_sort_lex* grouped the columns; group[0] was sorted first (the least significant columns)."""
    _fields_ = [("ncols", C.c_uint32), ("ngroups", C.c_uint32), ("pack_bytes", C.c_uint32), ("early_exit", C.c_uint32),
                ("group", LexGroup * LEX_MAX_COLS)]

    def groups(self):
        return [(int(g.first_col), int(g.ncols), int(g.key_bytes), int(g.sorted_as)) for g in self.group[:self.ngroups]]


# rsx_segments_info.route, rsx_sort_segments*'s flag, the size classes and their seams (radix_sorting_amd/csrc/rsx_segments_shape.hpp)
SEGMENTS_TRIVIAL, SEGMENTS_LDS, SEGMENTS_MIXED, SEGMENTS_LEX = range(4)
SEGMENTS_LOCAL_IDX = 1
SEGMENTS_COPY, SEGMENTS_WAVE, SEGMENTS_GROUP, SEGMENTS_BLOCK, SEGMENTS_LONG = range(5)
SEGMENTS_CLASSES = 5
SEGMENTS_COPY_MAX, SEGMENTS_WAVE_MAX, SEGMENTS_GROUP_MAX = 1, 256, 2048     # the longest segment of the classes below BLOCK
SEGMENTS_LDS_BYTES, SEGMENTS_TEAM_FIXED, SEGMENTS_CAP_STEP = 163840, 256, 256
SEGMENTS_MAX_LONG = 4096              # the most RSX_SEGMENTS_MAX_LONG takes
SEGMENTS_DEFAULT_MAX_LONG = 8         # ... and its default; the classes (bits) in which the LDS route is the default: BLOCK
SEGMENTS_DEFAULT_CLASSES = 8


def SEGMENTS_CAP(dtype, with_idx):
    """The longest segment the LDS route takes for keys of ``dtype`` (``with_idx``: out_idx is wanted): rsx_segments_shape.hpp's
    segments_cap -- a workgroup's 160 KiB less sixteen rows of cells and the exchanged words, over two buffers of keys (and u16
    positions), in steps of 256, at most 65536."""
    per = 2 * (DTYPE_SIZE[dtype] + (2 if with_idx else 0))
    cap = (SEGMENTS_LDS_BYTES - 16 * 1024 - SEGMENTS_TEAM_FIXED) // per // SEGMENTS_CAP_STEP * SEGMENTS_CAP_STEP
    return min(cap, 65536)


class SegmentsInfo(C.Structure):
    """rsx_segments_info: the route rsx_sort_segments* took, the size classes of its segments and what the inner sorts reported."""
    _fields_ = [("route", C.c_uint32), ("key_bytes", C.c_uint32), ("cap", C.c_uint32), ("pad", C.c_uint32), ("max_len", C.c_uint64),
                ("n_long", C.c_uint64), ("class_count", C.c_uint64 * SEGMENTS_CLASSES), ("lex", LexInfo), ("sort", Info)]

    def classes(self):
        return [int(x) for x in self.class_count]


# every symbol include/rsx.h declares: (name, restype, argtypes)
_VP, _SZ, _I, _U32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
_PVP, _PINFO = C.POINTER(C.c_void_p), C.POINTER(Info)
_PUINFO, _PSZ = C.POINTER(UniqueInfo), C.POINTER(C.c_size_t)
_PTINFO = C.POINTER(TopkInfo)
_PGINFO = C.POINTER(GroupInfo)
_PRINFO = C.POINTER(RankdataInfo)
_PREDINFO = C.POINTER(ReduceInfo)
_PNINFO, _PU64 = C.POINTER(NthInfo), C.POINTER(C.c_uint64)
_PLCOL, _PLINFO = C.POINTER(LexCol), C.POINTER(LexInfo)
_PLOCINFO = C.POINTER(LocateInfo)
_PJINFO = C.POINTER(JoinInfo)
_PPARTINFO = C.POINTER(PartitionInfo)
_PSEGINFO = C.POINTER(SegmentsInfo)
ABI = [
    ("rsx_device_count", _I, []),
    ("rsx_last_error", C.c_char_p, []),
    ("rsx_version", C.c_char_p, []),
    ("rsx_dtype_size", _SZ, [_I]),
    ("rsx_workspace_bytes", _SZ, [_SZ, _I, _SZ]),
    ("rsx_release", None, []),
    ("rsx_reload_env", None, []),
    ("rsx_sort", _I, [_VP, _VP, _SZ, _I, _I, _PVP, _PINFO]),
    ("rsx_release_stream", None, [_VP]),
    ("rsx_sort_inplace_async", _I, [_VP, _VP, _SZ, _I, _I, _VP]),
    ("rsx_sort_inplace_async_hint", _I, [_VP, _VP, _SZ, _I, _I, _VP, C.c_uint32]),
    ("rsx_sort_inplace_async_ws", _I, [_VP, _VP, _SZ, _I, _I, _VP, _SZ, _VP]),
    ("rsx_workspace_bytes_fast", _SZ, [_SZ, _I]),
    ("rsx_async_route_ws", _I, [_VP, _SZ, _SZ, _I, _VP, C.POINTER(C.c_uint32)]),
    ("rsx_sort_pairs_inplace_async_ws", _I, [_VP, _VP, _VP, _VP, _SZ, _I, _SZ, _I, _VP, _SZ, _VP]),
    ("rsx_sort_pairs_inplace_async", _I, [_VP, _VP, _VP, _VP, _SZ, _I, _SZ, _I, _VP]),
    ("rsx_capture_histogram", _I, [_VP, _SZ]),
    ("rsx_sort_device", _I, [_VP, _VP, _SZ, _I, _I, _VP, _PVP, _PINFO]),
    ("rsx_sort_unique_device", _I, [_VP, _VP, _SZ, _I, _I, _VP, _SZ, _VP, _PVP, _PSZ, _PUINFO]),
    ("rsx_sort_unique", _I, [_VP, _VP, _SZ, _I, _I, _VP, _SZ, _PVP, _PSZ, _PUINFO]),
    ("rsx_sort_group_device", _I, [_VP, _SZ, _I, _I, _VP, _VP, _VP, _VP, _SZ, _VP, _PSZ, _PGINFO]),
    ("rsx_sort_group", _I, [_VP, _SZ, _I, _I, _VP, _VP, _VP, _VP, _SZ, _PSZ, _PGINFO]),
    ("rsx_sort_reduce_device", _I, [_VP, _VP, _SZ, _I, _I, _I, C.c_uint, _VP, _VP, _SZ, _VP, _VP, _VP, _VP, _PSZ, _PREDINFO]),
    ("rsx_sort_reduce", _I, [_VP, _VP, _SZ, _I, _I, _I, C.c_uint, _VP, _VP, _SZ, _VP, _VP, _VP, _PSZ, _PREDINFO]),
    ("rsx_sort_rankdata_device", _I, [_VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _VP, _PRINFO]),
    ("rsx_sort_rankdata", _I, [_VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _PRINFO]),
    ("rsx_sort_topk_device", _I, [_VP, _SZ, _SZ, _I, _I, _VP, _VP, _SZ, _VP, _PTINFO]),
    ("rsx_sort_topk", _I, [_VP, _SZ, _SZ, _I, _I, _VP, _VP, _SZ, _PTINFO]),
    ("rsx_sort_nth_device", _I, [_VP, _SZ, _PU64, _SZ, _I, _I, _VP, _VP, _SZ, _PU64, _PU64, _VP, _PNINFO]),
    ("rsx_sort_nth", _I, [_VP, _SZ, _PU64, _SZ, _I, _I, _VP, _VP, _SZ, _PU64, _PU64, _PNINFO]),
    ("rsx_sort_locate_device", _I, [_VP, _SZ, _VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _U32, _VP, _PLOCINFO]),
    ("rsx_sort_locate", _I, [_VP, _SZ, _VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _U32, _PLOCINFO]),
    ("rsx_sort_partition_device", _I, [_VP, _SZ, _VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _U32, _VP, _PPARTINFO]),
    ("rsx_sort_partition", _I, [_VP, _SZ, _VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _U32, _PPARTINFO]),
    ("rsx_sort_segments_device", _I, [_VP, _SZ, _VP, _SZ, _SZ, _I, _I, _VP, _VP, _U32, _VP, _PSEGINFO]),
    ("rsx_sort_segments", _I, [_VP, _SZ, _VP, _SZ, _SZ, _I, _I, _VP, _VP, _U32, _PSEGINFO]),
    ("rsx_sort_join_device", _I, [_VP, _SZ, _VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _U32, _VP, _PU64, _PJINFO]),
    ("rsx_sort_join", _I, [_VP, _SZ, _VP, _SZ, _I, _I, _VP, _VP, _VP, _SZ, _U32, _PU64, _PJINFO]),
    ("rsx_join_pairs_device", _I, [_VP, _VP, _VP, _SZ, _SZ, _SZ, _U32, _VP, _VP, C.c_uint64, _VP, _PU64]),
    ("rsx_join_pairs", _I, [_VP, _VP, _VP, _SZ, _SZ, _SZ, _U32, _VP, _VP, C.c_uint64, _PU64]),
    ("rsx_sort_lex_device", _I, [_PLCOL, _SZ, _SZ, _VP, _SZ, _VP, _PLINFO]),
    ("rsx_sort_lex", _I, [_PLCOL, _SZ, _SZ, _VP, _SZ, _PLINFO]),
    ("rsx_sort_pairs_device", _I, [_VP, _VP, _VP, _VP, _SZ, _I, _SZ, _I, _VP, _PINFO]),
    ("rsx_sort_rank", _I, [_VP, _VP, _SZ, _I, _SZ, _I, _PVP, _PINFO]),
    ("rsx_sort_rank_device", _I, [_VP, _VP, _SZ, _I, _SZ, _I, _VP, _PVP, _PINFO]),
    ("rsx_sort_records", _I, [_VP, _VP, _SZ, _SZ, _VP, _SZ, _PVP, _PINFO]),
    ("rsx_sort_records_tagged", _I, [_VP, _VP, _SZ, _SZ, _SZ, _I, _I, _PVP, _PINFO]),
    ("rsx_sort_records_tagged_device", _I, [_VP, _VP, _SZ, _SZ, _SZ, _I, _I, _VP, _PVP, _PINFO]),
    ("rsx_sort_rank_keys", _I, [_VP, _SZ, _VP, _SZ, _SZ, _PVP, _PINFO]),
    ("rsx_histogram_device", _I, [_VP, _SZ, _I, _I, _VP, _VP, _VP]),
    ("rsx_msd_split_device", _I, [_VP, _VP, _SZ, _I, _I, _I, _VP, _VP]),
    ("rsx_msd_split_async", _I, [_VP, _VP, _SZ, _I, _I, _I, _VP, _VP]),
    ("rsx_sort_rank_inplace_async", _I, [_VP, _VP, _SZ, _I, _SZ, _I, _VP]),
    ("rsx_verify_poll", _I, [_VP, C.POINTER(C.c_uint64)]),
    ("rsx_async_route", _I, [_VP, C.POINTER(C.c_uint32)]),
    ("rsx_sort_multi", _I, [_VP, _VP, _SZ, _I, _I, _VP, _I, _PVP, _PINFO]),
    ("rsx_profile_begin", _I, []),
    ("rsx_profile_end", _I, [C.POINTER(Profile)]),
    ("rsx_fill_splitmix_device", _I, [_VP, _SZ, _SZ, C.c_uint64, C.c_uint64, C.c_uint64, _VP]),
    ("rsx_spin_device", _I, [C.c_uint64, _VP]),
]

_lib = None


def lib():
    """The loaded librsx.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RsxError("%s is missing: build it with `make lib` (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 (SONAME
        # libamdhip64.so.7, the same as /opt/rocm's); whichever copy is mapped first serves every
        # later NEEDED entry of that SONAME, and a second copy cannot see the GPU.  Where torch is
        # installed it therefore has to be imported before librsx.so pulls in /opt/rocm's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        handle = C.CDLL(LIB_PATH)
        for name, res, args in ABI:
            f = getattr(handle, name)      # AttributeError here means the ABI and the header diverged
            f.restype = res
            f.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise RsxError("rsx error %d: %s" % (rc, lib().rsx_last_error().decode()))


def reload_env():
    """Have the library read its RSX_* environment switches again (it reads them once, at its first call)."""
    lib().rsx_reload_env()


def device_count():
    return int(lib().rsx_device_count())


def require_gpu():
    if device_count() <= 0:
        raise RsxError("no gfx950 (MI355X) device visible to HIP; radix_sorting_amd has no CPU path")


# ---- torch-facing helpers -------------------------------------------------------------------

def _torch_dtype_code(t):
    import torch
    table = {torch.uint8: U8, torch.int8: I8, torch.int16: I16, torch.int32: I32, torch.int64: I64,
             torch.float32: F32, torch.float64: F64}
    for name, code in (("uint16", U16), ("uint32", U32), ("uint64", U64)):
        if hasattr(torch, name):
            table[getattr(torch, name)] = code
    if t.dtype not in table:
        raise RsxError("unsupported tensor dtype %s" % t.dtype)
    return table[t.dtype]


def _stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _check_dev(*tensors):
    """Every buffer handed to the kernels as a raw pointer: a contiguous tensor on the CURRENT device."""
    import torch
    cur = torch.cuda.current_device()
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise RsxError("expected contiguous device tensors")
        if t.device.index != cur:
            raise RsxError("tensor on cuda:%d but the current device is cuda:%d (the library works on the current device)"
                           % (t.device.index, cur))


def _same_shape(a, b, what):
    """`b` is the ping-pong partner of `a`: same element size, at least as many elements."""
    if b.element_size() != a.element_size() or b.numel() < a.numel():
        raise RsxError("%s does not match its buffer (element size %d vs %d, %d vs %d elements)"
                       % (what, b.element_size(), a.element_size(), b.numel(), a.numel()))


_armed_hist = threading.local()   # keeps the armed array alive: the library only holds its address


def capture_histogram(hist):
    """rsx_capture_histogram: arm the calling thread's next blocking sort to write the counts of loop 1
    (radix_sort.hpp:48-58) into `hist` (numpy uint64, >= 256 * key bytes entries); None disarms.

    The library keeps the raw address until a sort reaches its histogram: prefer ``with capturing_histogram(hist):``,
    which disarms on the way out whatever happened in between (an exception before the sort, an *_async call that
    never captures), so that no later sort of this thread writes into an array that is gone."""
    if hist is None:
        check(lib().rsx_capture_histogram(None, 0))
        _armed_hist.ref = None
    else:
        import numpy as np
        if hist.dtype != np.uint64 or not hist.flags["C_CONTIGUOUS"]:
            raise RsxError("capture_histogram wants a contiguous numpy uint64 array")
        check(lib().rsx_capture_histogram(hist.ctypes.data, hist.size))
        _armed_hist.ref = hist


class capturing_histogram:
    """Context manager around capture_histogram: armed on entry, disarmed on exit (rsx_capture_histogram(NULL, 0))."""

    def __init__(self, hist):
        self.hist = hist

    def __enter__(self):
        capture_histogram(self.hist)
        return self.hist

    def __exit__(self, *exc):
        capture_histogram(None)
        return False


def radix_sort(src, aux, dtype=None, order=ASCENDING, stream=None):
    """radix_sort(src, aux, n) on device tensors (radix_sort.hpp:98-115).

    Returns (result, info): ``result`` is ``src`` or ``aux`` by the reference's
    returned-pointer rule.  ``dtype`` overrides the rsx_dtype code, so bit
    patterns held in an int32/int64 tensor can be sorted as uint32/uint64/float.
    The scatter passes are only enqueued on ``stream``.
    """
    _check_dev(src, aux)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    _same_shape(src, aux, "aux")
    res, info = C.c_void_p(), Info()
    check(lib().rsx_sort_device(src.data_ptr(), aux.data_ptr(), src.numel(), code, order, _stream_ptr(stream),
                                C.byref(res), C.byref(info)))
    return (aux if info.result_in_aux else src), info


def radix_sort_unique(src, aux, dtype=None, order=ASCENDING, counts=None, stream=None):
    """rsx_sort_unique_device: the distinct keys of ``src`` in order of kdf(key) (distinct BIT PATTERNS: -0.0 and +0.0 are two).

    Returns (result[:n_unique], counts[:n_unique] or None, info): ``result`` is ``src`` or ``aux``; ``counts`` is an int32 /
    int64 (or uint32 / uint64) device tensor with room for n entries that receives how often each distinct key occurs.
    ``src`` is consumed; the call returns once n_unique is known."""
    _check_dev(src, aux)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    _same_shape(src, aux, "aux")
    cptr, cbytes = None, 0
    if counts is not None:
        _check_dev(counts)
        cbytes = counts.element_size()
        if counts.numel() < src.numel():
            raise RsxError("counts must have room for n entries")
        cptr = counts.data_ptr()
    res, nu, info = C.c_void_p(), C.c_size_t(0), UniqueInfo()
    check(lib().rsx_sort_unique_device(src.data_ptr(), aux.data_ptr(), src.numel(), code, order, cptr, cbytes, _stream_ptr(stream),
                                       C.byref(res), C.byref(nu), C.byref(info)))
    out = aux if (src.numel() and res.value == aux.data_ptr() and res.value != src.data_ptr()) else src
    return out[:nu.value], (None if counts is None else counts[:nu.value]), info


def radix_sort_group(src, dtype=None, order=ASCENDING, idx_dtype=None, keys=False, counts=False, first=False, stream=None,
                     inverse=True):
    """rsx_sort_group_device: for every key of ``src`` (not written) the index of its group among the distinct keys in order
    of kdf(key) -- what ``torch.unique(sorted=True, return_inverse=True)`` calls the inverse, by BIT PATTERN (-0.0 and +0.0
    are two groups).

    Returns (inverse, keys[:G] or None, counts[:G] or None, first[:G] or None, info): ``keys`` are radix_sort_unique's,
    ``counts[j]`` the size of group j, ``first[j]`` the smallest index whose key is ``keys[j]``.  ``keys`` / ``counts`` /
    ``first`` / ``inverse``: True allocates the output (n elements; ``idx_dtype``, default torch.int32, for the three index
    arrays), False leaves it out, a device tensor with room for n elements is written in place.  Asking for counts or first
    gives up the sort-free routes except the one-column table (first: that one too).  The call returns once G is known."""
    import torch
    _check_dev(src)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    n = src.numel()
    idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()

    def buf(want, what, dt, size):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(n, dtype=dt, device=src.device)
        _check_dev(want)
        if want.numel() < n or want.element_size() != size:
            raise RsxError("%s must have room for n elements of the right size" % what)
        return want

    inv = buf(inverse, "inverse", idx_dtype, idx_bytes)
    k = buf(keys, "keys", src.dtype, src.element_size())
    cn = buf(counts, "counts", idx_dtype, idx_bytes)
    fi = buf(first, "first", idx_dtype, idx_bytes)
    ptr = lambda t: None if t is None else t.data_ptr()
    ng, info = C.c_size_t(0), GroupInfo()
    check(lib().rsx_sort_group_device(src.data_ptr(), n, code, order, ptr(inv), ptr(k), ptr(cn), ptr(fi), idx_bytes,
                                      _stream_ptr(stream), C.byref(ng), C.byref(info)))
    g = ng.value
    cut = lambda t: None if t is None else t[:g]
    return (None if inv is None else inv[:n]), cut(k), cut(cn), cut(fi), info


def _reduce_ops(sum_buf, min_buf, max_buf):
    return (REDUCE_SUM if sum_buf is not None else 0) | (REDUCE_MIN if min_buf is not None else 0) | (REDUCE_MAX if max_buf is not None else 0)


def radix_sort_reduce(keys, vals, dtype=None, val_dtype=None, order=ASCENDING, idx_dtype=None, sum=True, min=False, max=False,
                      counts=False, keys_out=True, stream=None):
    """rsx_sort_reduce_device: per group of bit-equal ``keys`` (not written), in order of kdf(key), the number of elements and
    the sum, the smallest and the largest of the ``vals`` (not written; 4- or 8-byte elements) that stand beside them -- what
    ``torch.unique(return_inverse=True)`` + ``index_add_`` / ``scatter_reduce``, ``np.bincount(k, weights=v)`` or a COO
    ``coalesce()`` compute.

    Returns (keys[:G] or None, counts[:G] or None, sum[:G] or None, min[:G] or None, max[:G] or None, info).  ``sum`` is 64 bits
    wide: int64 holding the u64 / i64 sum modulo 2^64 for integer values, float64 for float values.  ``min`` / ``max`` are in the
    values' type, ordered by the value's own KDF (floats by bit pattern: -0.0 below +0.0, a NaN with the sign bit clear above
    +inf: a NaN does not poison them).  Each of ``keys_out`` / ``counts`` / ``sum`` / ``min`` / ``max``: True allocates the output
    (n elements; ``idx_dtype``, default torch.int32, for the counts), False leaves it out, a device tensor with room for n elements
    is written in place.  The call returns once G is known."""
    import torch
    _check_dev(keys, vals)
    code = _torch_dtype_code(keys) if dtype is None else dtype
    vcode = _torch_dtype_code(vals) if val_dtype is None else val_dtype
    if keys.element_size() != DTYPE_SIZE[code]:
        raise RsxError("keys do not match the key type")
    if vals.element_size() != DTYPE_SIZE[vcode] or vals.numel() < keys.numel():
        raise RsxError("vals do not match the value type or the keys")
    n = keys.numel()
    idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()
    sum_dtype = torch.float64 if vcode in (F32, F64) else torch.int64

    def buf(want, what, dt, size):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(n, dtype=dt, device=keys.device)
        _check_dev(want)
        if want.numel() < n or want.element_size() != size:
            raise RsxError("%s must have room for n elements of the right size" % what)
        return want

    k = buf(keys_out, "keys_out", keys.dtype, keys.element_size())
    cn = buf(counts, "counts", idx_dtype, idx_bytes)
    sm = buf(sum, "sum", sum_dtype, 8)
    mn = buf(min, "min", vals.dtype, vals.element_size())
    mx = buf(max, "max", vals.dtype, vals.element_size())
    ptr = lambda t: None if t is None else t.data_ptr()
    ng, info = C.c_size_t(0), ReduceInfo()
    check(lib().rsx_sort_reduce_device(keys.data_ptr(), vals.data_ptr(), n, code, order, vcode, _reduce_ops(sm, mn, mx), ptr(k), ptr(cn),
                                       idx_bytes, ptr(sm), ptr(mn), ptr(mx), _stream_ptr(stream), C.byref(ng), C.byref(info)))
    g = ng.value
    cut = lambda t: None if t is None else t[:g]
    return cut(k), cut(cn), cut(sm), cut(mn), cut(mx), info


def radix_sort_rankdata(src, dtype=None, order=ASCENDING, idx_dtype=None, place=True, less=False, equal=False, stream=None):
    """rsx_sort_rankdata_device: for every key of ``src`` (not written) where it stands in the stable sorted order by kdf(key)
    -- ``place``, the inverse of radix_sort_rank's permutation --, how many keys are smaller (``less``) and how many are equal
    to it, itself included (``equal``), by BIT PATTERN (-0.0 and +0.0 are two keys).  All 0-based.

    Returns (place, less, equal, info), None for what was not asked for.  ``place`` / ``less`` / ``equal``: True allocates the
    output (n elements of ``idx_dtype``, default torch.int32), False leaves it out, a device tensor of exactly the room for n
    elements or more is written in place; at least one must be wanted.  Asking for the place gives up the count table of up
    to 16 varying bits (one varying byte column keeps its sort-free route)."""
    import torch
    _check_dev(src)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    n = src.numel()
    idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()

    def buf(want, what):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(n, dtype=idx_dtype, device=src.device)
        _check_dev(want)
        if want.numel() < n or want.element_size() != idx_bytes:
            raise RsxError("%s must have room for n elements of the right size" % what)
        return want

    pl, le, eq = buf(place, "place"), buf(less, "less"), buf(equal, "equal")
    ptr = lambda t: None if t is None else t.data_ptr()
    info = RankdataInfo()
    check(lib().rsx_sort_rankdata_device(src.data_ptr(), n, code, order, ptr(pl), ptr(le), ptr(eq), idx_bytes, _stream_ptr(stream),
                                         C.byref(info)))
    cut = lambda t: None if t is None else t[:n]
    return cut(pl), cut(le), cut(eq), info


RANKDATA_METHODS = ("ordinal", "min", "max", "average", "dense")


def rankdata(src, method="ordinal", dtype=None, order=ASCENDING, idx_dtype=None, stream=None):
    """The rank of every key of ``src`` among all of them, as ``scipy.stats.rankdata`` assigns it -- but 0-BASED where scipy's
    ranks are 1-based (add 1 for scipy's), and by bit pattern of the keys.  ``method``: "ordinal" (ties in index order: the
    place of radix_sort_rankdata), "min" (less), "max" (less + equal - 1), "average" (less + (equal - 1) / 2, a float64
    tensor) or "dense" (radix_sort_group's inverse).  Only the arrays the method needs are asked for, so "min" and "max" take
    the table routes where they apply.  Returns (ranks, info)."""
    if method not in RANKDATA_METHODS:
        raise RsxError("rankdata: method %r is none of %s" % (method, ", ".join(RANKDATA_METHODS)))
    if method == "dense":
        inv, _, _, _, info = radix_sort_group(src, dtype=dtype, order=order, idx_dtype=idx_dtype, stream=stream)
        return inv, info
    if method == "ordinal":
        pl, _, _, info = radix_sort_rankdata(src, dtype, order, idx_dtype, place=True, stream=stream)
        return pl, info
    if method == "min":
        _, le, _, info = radix_sort_rankdata(src, dtype, order, idx_dtype, place=False, less=True, stream=stream)
        return le, info
    _, le, eq, info = radix_sort_rankdata(src, dtype, order, idx_dtype, place=False, less=True, equal=True, stream=stream)
    if method == "max":
        return le + eq - 1, info
    import torch
    return le.to(torch.float64) + (eq.to(torch.float64) - 1.0) / 2.0, info


def radix_sort_locate(src, vals, dtype=None, order=ASCENDING, idx_dtype=None, less=True, equal=False, bins=False, below=False,
                      stream=None):
    """rsx_sort_locate_device: where the values ``vals`` (any order, repeats allowed, need not occur in ``src``; neither tensor is
    written) fall in the sorted order of ``src`` by kdf(key), by BIT PATTERN (-0.0 and +0.0 are two keys):
    ``less[j]`` keys are below ``vals[j]``, ``equal[j]`` equal it, and key i has ``bins[i]`` values at or below it
    (``below=True``: strictly below it).

    Returns (info, less, equal, bins), None for what was not asked for.  ``less`` / ``equal`` / ``bins``: True allocates the output
    (m resp. n elements of ``idx_dtype``, default torch.int32), False leaves it out, a device tensor with room for them is
    written in place; at least one must be wanted."""
    import torch
    _check_dev(src, vals)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code] or vals.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src and vals do not match the key type")
    n, m = src.numel(), vals.numel()
    idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()

    def buf(want, count, what):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(count, dtype=idx_dtype, device=src.device)
        _check_dev(want)
        if want.numel() < count or want.element_size() != idx_bytes:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    le, eq, bi = buf(less, m, "less"), buf(equal, m, "equal"), buf(bins, n, "bins")
    ptr = lambda t: None if t is None else t.data_ptr()
    info = LocateInfo()
    check(lib().rsx_sort_locate_device(src.data_ptr(), n, vals.data_ptr(), m, code, order, ptr(le), ptr(eq), ptr(bi), idx_bytes,
                                       LOCATE_BINS_BELOW if below else 0, _stream_ptr(stream), C.byref(info)))
    cut = lambda t, count: None if t is None else t[:count]
    return info, cut(le, m), cut(eq, m), cut(bi, n)


def searchsorted(src, vals, side="left", dtype=None, order=ASCENDING, idx_dtype=None, stream=None):
    """``np.searchsorted(np.sort(src), vals, side)`` / ``torch.searchsorted(torch.sort(src).values, vals, right=side == "right")``
    without sorting ``src`` where the values are few -- in the library's order of the keys (by bit pattern through the KDF:
    NaNs have a place, -0.0 stands before +0.0).  Returns (positions, info)."""
    if side not in ("left", "right"):
        raise RsxError("searchsorted: side %r is neither 'left' nor 'right'" % (side,))
    info, le, eq, _ = radix_sort_locate(src, vals, dtype, order, idx_dtype, less=True, equal=side == "right", stream=stream)
    return (le if side == "left" else le + eq), info


def bucketize(src, edges, right=False, dtype=None, order=ASCENDING, idx_dtype=None, stream=None):
    """``torch.bucketize(src, torch.sort(edges).values, right=right)``: for every key the number of edges below it (``right=False``,
    the library's ``below=True``) or at or below it (``right=True``: also ``np.digitize(src, np.sort(edges))``).  The edges need
    not be sorted.  In the library's order of the keys, as searchsorted().  Returns (bins, info)."""
    info, _, _, bi = radix_sort_locate(src, edges, dtype, order, idx_dtype, less=False, bins=True, below=not right, stream=stream)
    return bi, info


def radix_sort_partition(src, edges, dtype=None, order=ASCENDING, idx_dtype=None, keys=True, idx=False, offsets=True, below=False,
                         stream=None):
    """rsx_sort_partition_device: the keys of ``src`` listed part by part as the values ``edges`` (any order, repeats allowed, need
    not occur in ``src``; neither tensor is written) cut them -- key i falls in part ``#{ j : edges[j] <= src[i] }`` (``below=True``:
    ``<``) in the library's order of the keys, the parts come in ascending order and inside a part the keys keep their input order.

    Returns (info, keys, idx, offsets), None for what was not asked for: ``keys`` the n keys in that order, ``idx`` the input row
    of every output position (``torch.argsort(bins, stable=True)``), ``offsets`` m + 2 entries -- part p is
    ``[offsets[p], offsets[p + 1])``.  Each: True allocates the output (``idx_dtype``, default torch.int32, for ``idx`` and
    ``offsets``), False leaves it out, a device tensor with room for it is written in place; ``keys`` or ``idx`` must be wanted."""
    import torch
    _check_dev(src, edges)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code] or edges.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src and edges do not match the key type")
    n, m = src.numel(), edges.numel()
    idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()

    def buf(want, count, what, dt, size):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(count, dtype=dt, device=src.device)
        _check_dev(want)
        if want.numel() < count or want.element_size() != size:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    ke = buf(keys, n, "keys", src.dtype, src.element_size())
    ix, of = buf(idx, n, "idx", idx_dtype, idx_bytes), buf(offsets, m + 2, "offsets", idx_dtype, idx_bytes)
    ptr = lambda t: None if t is None else t.data_ptr()
    info = PartitionInfo()
    check(lib().rsx_sort_partition_device(src.data_ptr(), n, edges.data_ptr(), m, code, order, ptr(ke), ptr(ix), ptr(of), idx_bytes,
                                          PARTITION_BELOW if below else 0, _stream_ptr(stream), C.byref(info)))
    cut = lambda t, count: None if t is None else t[:count]
    return info, cut(ke, n), cut(ix, n), cut(of, m + 2)


def partition_even(src, parts, dtype=None, order=ASCENDING, idx_dtype=None, keys=True, idx=False, below=False, stream=None):
    """``src`` cut into ``parts`` (1 .. 65) parts of as equal size as its ties allow: radix_sort_nth finds the keys at the ranks
    i * n // parts of the sorted order, radix_sort_partition splits by them.  With ``below=False`` (the default) a key equal to a
    splitter goes to the part above it, so ``offsets[i]`` is the number of keys below the i-th splitter (nth's ``n_less``):
    exactly ``i * n // parts`` where the keys are distinct.  Returns (info, keys, idx, offsets, splitters) as radix_sort_partition does, ``offsets`` of parts + 1 entries."""
    if not 1 <= parts <= NTH_MAX_SELECT_RANKS + 1:
        raise RsxError("partition_even: parts = %r is not in 1 .. %d" % (parts, NTH_MAX_SELECT_RANKS + 1))
    n = src.numel()
    if n == 0:
        raise RsxError("partition_even: no keys")
    splitters, _, _, _, _ = radix_sort_nth(src, [i * n // parts for i in range(1, parts)], dtype=dtype, order=order, want_idx=False,
                                           stream=stream)
    info, ke, ix, of = radix_sort_partition(src, splitters, dtype, order, idx_dtype, keys=keys, idx=idx, offsets=True, below=below,
                                            stream=stream)
    return info, ke, ix, of, splitters


def radix_sort_segments(src, offsets=None, rows=None, dtype=None, order=ASCENDING, idx_dtype=None, keys=True, idx=False, local_idx=False,
                        stream=None):
    """rsx_sort_segments_device: the keys of ``src`` cut into segments and every segment sorted on its own, stably, in the library's
    order of the keys.  ``offsets``: a device tensor of m + 1 non-decreasing entries from 0 to n (4- or 8-byte integers; their width
    is the width of the indices), segment s is ``[offsets[s], offsets[s + 1])``; or ``rows``: m equal rows of n / m keys.  Neither
    ``src`` nor ``offsets`` is written.

    Returns (info, keys, idx), None for what was not asked for: ``keys`` the n keys, every segment in its own range, ``idx`` the
    input position of every output element -- in the whole array, or with ``local_idx`` counted from the segment's start
    (``torch.sort(dim=-1).indices``).  Each: True allocates the output (``idx_dtype``, default the offsets' type or torch.int32),
    False leaves it out, a device tensor with room for it is written in place; one of the two must be wanted."""
    import torch
    _check_dev(src)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    n = src.numel()
    if (offsets is None) == (rows is None):
        raise RsxError("radix_sort_segments: give either offsets or rows")
    if offsets is not None:
        _check_dev(offsets)
        if offsets.numel() < 1 or offsets.element_size() not in (4, 8):
            raise RsxError("offsets must hold m + 1 entries of 4 or 8 bytes")
        m = offsets.numel() - 1
        idx_dtype = offsets.dtype if idx_dtype is None else idx_dtype
    else:
        m = int(rows)
        idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()
    if offsets is not None and offsets.element_size() != idx_bytes:
        raise RsxError("offsets and idx must have elements of the same size")

    def buf(want, what, dt, size):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(n, dtype=dt, device=src.device)
        _check_dev(want)
        if want.numel() < n or want.element_size() != size:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    ke, ix = buf(keys, "keys", src.dtype, src.element_size()), buf(idx, "idx", idx_dtype, idx_bytes)
    ptr = lambda t: None if t is None else t.data_ptr()
    info = SegmentsInfo()
    check(lib().rsx_sort_segments_device(src.data_ptr(), n, ptr(offsets), m, idx_bytes, code, order, ptr(ke), ptr(ix),
                                         SEGMENTS_LOCAL_IDX if local_idx else 0, _stream_ptr(stream), C.byref(info)))
    cut = lambda t: None if t is None else t[:n]
    return info, cut(ke), cut(ix)


def sort_rows(x, descending=False, stream=None):
    """``torch.sort(x, dim=-1, descending=descending, stable=True)`` for a contiguous 2-D device tensor, in the library's order of
    the keys (by bit pattern through the KDF: NaNs have a place, -0.0 stands before +0.0).  Returns (values, indices), indices
    int64 and local to the row as torch's."""
    import torch
    if x.dim() != 2:
        raise RsxError("sort_rows: a 2-D tensor is expected")
    rows, cols = x.shape
    flat = x.contiguous().view(-1)
    if flat.numel() == 0:
        return torch.empty_like(x), torch.empty(x.shape, dtype=torch.int64, device=x.device)
    _, ke, ix = radix_sort_segments(flat, rows=rows, order=DESCENDING if descending else ASCENDING, idx_dtype=torch.int64, keys=True, idx=True,
                                    local_idx=True, stream=stream)
    return ke.view(rows, cols), ix.view(rows, cols)


def _join_how(how):
    if how not in ("inner", "left"):
        raise RsxError("join: how %r is neither 'inner' nor 'left'" % (how,))
    return JOIN_LEFT if how == "left" else 0


def radix_sort_join_ranges(left, right, dtype=None, order=ASCENDING, how="inner", idx_dtype=None, start=True, count=True,
                           right_perm=True, stream=None):
    """rsx_sort_join_device, phase 1 of the join alone: one range into the sorted right side per left row.

    Returns (n_pairs, start, count, right_perm, info), None for what was not asked for: the rows of ``right`` that match
    ``left[i]`` by kdf(key), by BIT PATTERN, are ``right_perm[start[i] : start[i] + count[i]]`` (``start[i]`` is unspecified
    where ``count[i] == 0``); ``n_pairs`` is the number of pairs ``how`` yields.  ``start`` / ``count`` / ``right_perm``: True
    allocates the output (n resp. m elements of ``idx_dtype``, default torch.int32), False leaves it out, a device tensor with
    room for them is written in place; none at all is legal (the number of pairs alone).  Neither input is written."""
    import torch
    flags = _join_how(how)
    _check_dev(left, right)
    code = _torch_dtype_code(left) if dtype is None else dtype
    if left.element_size() != DTYPE_SIZE[code] or right.element_size() != DTYPE_SIZE[code]:
        raise RsxError("left and right do not match the key type")
    n, m = left.numel(), right.numel()
    idx_dtype = torch.int32 if idx_dtype is None else idx_dtype
    idx_bytes = torch.empty(0, dtype=idx_dtype).element_size()

    def buf(want, size, what):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(size, dtype=idx_dtype, device=left.device)
        _check_dev(want)
        if want.numel() < size or want.element_size() != idx_bytes:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    st, ct, pm = buf(start, n, "start"), buf(count, n, "count"), buf(right_perm, m, "right_perm")
    ptr = lambda t: None if t is None else t.data_ptr()
    info, pairs = JoinInfo(), C.c_uint64(0)
    check(lib().rsx_sort_join_device(left.data_ptr(), n, right.data_ptr(), m, code, order, ptr(st), ptr(ct), ptr(pm), idx_bytes, flags,
                                     _stream_ptr(stream), C.byref(pairs), C.byref(info)))
    cut = lambda t, size: None if t is None else t[:size]
    return int(pairs.value), cut(st, n), cut(ct, n), cut(pm, m), info


def radix_sort_join_pairs(start, count, right_perm, how="inner", left_idx=True, right_idx=True, n_pairs=None, stream=None):
    """rsx_join_pairs_device, phase 2 of the join alone: the ranges of radix_sort_join_ranges expanded into the pairs
    (left_idx[p], right_idx[p]), ordered by left row, then by right row; ``how="left"``: a left row without a match yields one
    pair whose right index is -1.  ``left_idx`` / ``right_idx``: True allocates exactly the number of pairs (``n_pairs`` as phase 1
    returned it; None: the library counts them first), False leaves the output out (not both), a device tensor is written in
    place and must have room for the pairs.  Returns (left_idx, right_idx, n_pairs)."""
    import torch
    flags = _join_how(how)
    _check_dev(start, count, right_perm)
    n, m = count.numel(), right_perm.numel()
    idx_bytes = count.element_size()
    if start.element_size() != idx_bytes or right_perm.element_size() != idx_bytes or start.numel() < n:
        raise RsxError("start, count and right_perm must be of one index type, start as long as count")
    pairs = C.c_uint64(0)

    def run(lo, ro, capacity):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib().rsx_join_pairs_device(start.data_ptr(), count.data_ptr(), right_perm.data_ptr(), n, m, idx_bytes, flags, ptr(lo), ptr(ro),
                                           capacity, _stream_ptr(stream), C.byref(pairs))

    if n_pairs is None and (left_idx is True or right_idx is True):
        # a call without room: it writes nothing and says how many pairs there are
        rc = run(torch.empty(1, dtype=count.dtype, device=count.device), None, 0)
        if rc != 0 and pairs.value == 0:
            check(rc)
        n_pairs = int(pairs.value)

    def buf(want, what):
        if want is False or want is None:
            return None
        if want is True:
            return torch.empty(n_pairs, dtype=count.dtype, device=count.device)
        _check_dev(want)
        if want.element_size() != idx_bytes:
            raise RsxError("%s must be of the inputs' index type" % what)
        return want

    lo, ro = buf(left_idx, "left_idx"), buf(right_idx, "right_idx")
    if n_pairs == 0 and (lo is not None or ro is not None):
        return lo, ro, 0     # (an empty tensor has no address to hand over)
    check(run(lo, ro, min([t.numel() for t in (lo, ro) if t is not None] or [0])))
    total = int(pairs.value)
    cut = lambda t: None if t is None else t[:total]
    return cut(lo), cut(ro), total


def radix_sort_join(left, right, how="inner", dtype=None, order=ASCENDING, idx_dtype=None, return_ranges=False, ranges=None,
                    stream=None):
    """The equi-join of two key columns (``pandas.merge(..., how=how)``'s indexers, SQL ``JOIN ... ON a.k = b.k``): every pair
    (i, j) with kdf(left[i]) == kdf(right[j]) by BIT PATTERN (-0.0 and +0.0 differ, a NaN matches the NaN of the same bits),
    ordered by i, then by j.  ``how="left"``: a left row without a match yields one pair (i, -1).

    Returns (left_idx, right_idx, info): phase 1 (rsx_sort_join_device) finds the ranges and the number of pairs, exactly that
    many are allocated (``idx_dtype``, default torch.int32), phase 2 (rsx_join_pairs_device) writes them.  ``return_ranges=True``
    appends (start, count, right_perm) to the result; ``ranges=(start, count, right_perm)`` as an earlier call returned them
    skips phase 1 (``left`` and ``right`` are not looked at and ``info`` is None)."""
    info, n_pairs = None, None
    if ranges is None:
        n_pairs, st, ct, pm, info = radix_sort_join_ranges(left, right, dtype, order, how, idx_dtype, stream=stream)
    else:
        st, ct, pm = ranges
    li, ri, _ = radix_sort_join_pairs(st, ct, pm, how, n_pairs=n_pairs, stream=stream)
    return (li, ri, info, st, ct, pm) if return_ranges else (li, ri, info)


def isin(src, test, dtype=None, order=ASCENDING, stream=None):
    """``np.isin(src, test)`` / ``torch.isin(src, test)`` on the derived keys, by BIT PATTERN: phase 1 of the join for ``count``
    alone, then ``> 0``.  Nothing is sorted where at most 16 bits of ``test`` vary.  Returns (mask, info)."""
    _, _, ct, _, info = radix_sort_join_ranges(src, test, dtype, order, start=False, count=True, right_perm=False, stream=stream)
    return ct != 0, info


def radix_sort_topk(src, k, dtype=None, order=ASCENDING, keys_out=None, idx_out=None, want_idx=True, stream=None):
    """rsx_sort_topk_device: the first ``k`` entries of the stable sorted order of ``src``, which is not written.

    Returns (keys, idx or None, info): ``keys[j]`` is the bit-exact image of ``src[idx[j]]`` and ``idx`` the first k entries
    of radix_sort_rank's result (equal keys in ascending index order).  Outputs of k elements are allocated when none are
    given: ``keys`` of src's dtype, ``idx`` int32 when n < 2^31, otherwise int64 (``want_idx=False``: no indices)."""
    import torch
    _check_dev(src)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    n, k = src.numel(), int(k)
    if keys_out is None:
        keys_out = torch.empty(k, dtype=src.dtype, device=src.device)
    if idx_out is None and want_idx:
        idx_out = torch.empty(k, dtype=torch.int32 if n < 2 ** 31 else torch.int64, device=src.device)
    for t, what, size in ((keys_out, "keys_out", src.element_size()), (idx_out, "idx_out", None)):
        if t is None:
            continue
        _check_dev(t)
        if t.numel() < k or (size is not None and t.element_size() != size):
            raise RsxError("%s must have room for k elements of the right size" % what)
    info = TopkInfo()
    check(lib().rsx_sort_topk_device(src.data_ptr(), n, k, code, order, keys_out.data_ptr(),
                                     None if idx_out is None else idx_out.data_ptr(),
                                     4 if idx_out is None else idx_out.element_size(), _stream_ptr(stream), C.byref(info)))
    return keys_out[:k], (None if idx_out is None else idx_out[:k]), info


def _nth_ranks(ranks, n):
    """The rank list of radix_sort_nth* as a contiguous uint64 array plus the two host arrays the call fills."""
    import numpy as np
    r = np.asarray(ranks)
    if r.ndim != 1:
        raise RsxError("ranks must be a one-dimensional sequence")
    if r.size and r.dtype.kind not in "iu":
        raise RsxError("ranks must be integers")
    if r.size and r.dtype.kind == "i" and int(r.min()) < 0:
        raise RsxError("ranks must not be negative")
    if r.size and int(r.max()) >= n:
        raise RsxError("rank exceeds n (largest rank %d, n = %d)" % (int(r.max()), n))
    r = np.ascontiguousarray(r, dtype=np.uint64)
    return r, np.zeros(r.size, dtype=np.uint64), np.zeros(r.size, dtype=np.uint64)


def _u64p(a):
    return a.ctypes.data_as(_PU64)


def radix_sort_nth(src, ranks, dtype=None, order=ASCENDING, keys_out=None, idx_out=None, want_idx=True, stream=None):
    """rsx_sort_nth_device: the entries at the positions ``ranks`` (0-based, any order, repeats allowed) of the stable sorted
    order of ``src``, which is not written.

    Returns (keys, idx or None, n_less, n_equal, info): ``idx[j]`` is entry ``ranks[j]`` of radix_sort_rank's result and
    ``keys[j]`` the bit-exact image of ``src[idx[j]]``; ``n_less`` / ``n_equal`` are numpy uint64 arrays: how many elements
    order before that key and how many equal it.  Outputs of m elements are allocated when none are given: ``keys`` of src's
    dtype, ``idx`` int32 when n < 2^31, otherwise int64 (``want_idx=False``: no indices)."""
    import torch
    _check_dev(src)
    code = _torch_dtype_code(src) if dtype is None else dtype
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    n = src.numel()
    r, n_less, n_equal = _nth_ranks(ranks, n)
    m = r.size
    if keys_out is None:
        keys_out = torch.empty(m, dtype=src.dtype, device=src.device)
    if idx_out is None and want_idx:
        idx_out = torch.empty(m, dtype=torch.int32 if n < 2 ** 31 else torch.int64, device=src.device)
    for t, what, size in ((keys_out, "keys_out", src.element_size()), (idx_out, "idx_out", None)):
        if t is None:
            continue
        _check_dev(t)
        if t.numel() < m or (size is not None and t.element_size() != size):
            raise RsxError("%s must have room for one element of the right size per rank" % what)
    info = NthInfo()
    check(lib().rsx_sort_nth_device(src.data_ptr(), n, _u64p(r), m, code, order, keys_out.data_ptr(),
                                    None if idx_out is None else idx_out.data_ptr(),
                                    4 if idx_out is None else idx_out.element_size(), _u64p(n_less), _u64p(n_equal),
                                    _stream_ptr(stream), C.byref(info)))
    return keys_out[:m], (None if idx_out is None else idx_out[:m]), n_less, n_equal, info


def _lex_cols(ptrs, codes, orders):
    n = len(ptrs)
    if orders is None:
        orders = [ASCENDING] * n
    if len(codes) != n or len(orders) != n:
        raise RsxError("orders / dtypes must have one entry per column")
    arr = (LexCol * max(n, 1))()
    for i in range(n):
        arr[i].data, arr[i].dtype, arr[i].order = ptrs[i], codes[i], orders[i]
    return arr


def radix_sort_lex(cols, orders=None, dtypes=None, idx_out=None, stream=None):
    """rsx_sort_lex_device: the stable argsort of the rows of ``cols`` (device tensors of one length, none of them written).

    ``cols[0]`` is the MOST significant column, as in ORDER BY -- the reverse of ``np.lexsort``'s argument order.  ``orders``
    and ``dtypes`` give one rsx_order / rsx_dtype code per column (default: ascending, the tensor's own type).  Returns
    (idx, info): ``idx`` is int32 when n < 2^31, otherwise int64, unless ``idx_out`` (n 4- or 8-byte entries) is given."""
    import torch
    cols = list(cols)
    if cols:
        _check_dev(*cols)
    n = cols[0].numel() if cols else 0
    codes = [_torch_dtype_code(t) for t in cols] if dtypes is None else list(dtypes)
    if len(codes) != len(cols):
        raise RsxError("orders / dtypes must have one entry per column")
    for t, code in zip(cols, codes):
        if t.numel() != n:
            raise RsxError("every column must have the same number of elements")
        if 0 <= code < len(DTYPE_SIZE) and t.element_size() != DTYPE_SIZE[code]:
            raise RsxError("a column does not match its key type")
    if idx_out is None:
        dev = cols[0].device if cols else "cuda"
        idx_out = torch.empty(n, dtype=torch.int32 if n < 2 ** 31 else torch.int64, device=dev)
    _check_dev(idx_out)
    if idx_out.numel() < n:
        raise RsxError("idx_out must have room for n entries")
    arr = _lex_cols([t.data_ptr() for t in cols], codes, orders)
    info = LexInfo()
    check(lib().rsx_sort_lex_device(arr, len(cols), n, idx_out.data_ptr(), idx_out.element_size(), _stream_ptr(stream), C.byref(info)))
    return idx_out[:n], info


HINT_EVEN_TOP_DIGITS = 1


def radix_sort_inplace_async(buf, scratch, dtype=None, order=ASCENDING, stream=None, hints=0):
    """rsx_sort_inplace_async: no host synchronisation, the sorted keys always end in ``buf`` (graph-capturable).
    ``hints`` (rsx_sort_inplace_async_hint): HINT_EVEN_TOP_DIGITS -- the caller has counted the keys by their top varying byte."""
    _check_dev(buf, scratch)
    code = _torch_dtype_code(buf) if dtype is None else dtype
    if buf.element_size() != DTYPE_SIZE[code]:
        raise RsxError("buf does not match the key type")
    _same_shape(buf, scratch, "scratch")
    if hints:
        check(lib().rsx_sort_inplace_async_hint(buf.data_ptr(), scratch.data_ptr(), buf.numel(), code, order, _stream_ptr(stream),
                                                int(hints)))
    else:
        check(lib().rsx_sort_inplace_async(buf.data_ptr(), scratch.data_ptr(), buf.numel(), code, order, _stream_ptr(stream)))
    return buf


def workspace_bytes_fast(n, dtype):
    """rsx_workspace_bytes_fast: a workspace that also holds the slots of a sort without a histogram (the *_ws sort then takes
    that route inside it)."""
    return int(lib().rsx_workspace_bytes_fast(n, dtype))


def async_route_ws(workspace, n, dtype, stream=None):
    """rsx_async_route_ws: the route the last rsx_sort_inplace_async_ws in `workspace` took (waits for the stream)."""
    r = C.c_uint32(0)
    check(lib().rsx_async_route_ws(workspace.data_ptr(), workspace.numel() * workspace.element_size(), n, dtype, _stream_ptr(stream),
                                   C.byref(r)))
    return int(r.value)


def workspace_bytes(n, dtype, payload_bytes=0):
    """rsx_workspace_bytes: what a workspace for the *_ws entry points must hold at least."""
    return int(lib().rsx_workspace_bytes(n, dtype, payload_bytes))


def radix_sort_inplace_async_ws(buf, scratch, workspace, dtype=None, order=ASCENDING, stream=None):
    """rsx_sort_inplace_async_ws: as radix_sort_inplace_async with every piece of device state in `workspace` (a uint8 device
    tensor the caller keeps for as long as a graph captured from this call lives)."""
    _check_dev(buf, scratch, workspace)
    code = _torch_dtype_code(buf) if dtype is None else dtype
    if buf.element_size() != DTYPE_SIZE[code]:
        raise RsxError("buf does not match the key type")
    _same_shape(buf, scratch, "scratch")
    check(lib().rsx_sort_inplace_async_ws(buf.data_ptr(), scratch.data_ptr(), buf.numel(), code, order, workspace.data_ptr(),
                                          workspace.numel() * workspace.element_size(), _stream_ptr(stream)))
    return buf


def radix_sort_pairs_inplace_async_ws(keys, keys_scratch, vals, vals_scratch, workspace, dtype=None, order=ASCENDING, stream=None):
    _check_dev(keys, keys_scratch, vals, vals_scratch, workspace)
    code = _torch_dtype_code(keys) if dtype is None else dtype
    if keys.element_size() != DTYPE_SIZE[code] or vals.element_size() not in (4, 8) or vals.numel() != keys.numel():
        raise RsxError("keys/vals do not match")
    _same_shape(keys, keys_scratch, "keys_scratch")
    _same_shape(vals, vals_scratch, "vals_scratch")
    check(lib().rsx_sort_pairs_inplace_async_ws(keys.data_ptr(), keys_scratch.data_ptr(), vals.data_ptr(), vals_scratch.data_ptr(),
                                                keys.numel(), code, vals.element_size(), order, workspace.data_ptr(),
                                                workspace.numel() * workspace.element_size(), _stream_ptr(stream)))
    return keys, vals


def release_stream(stream=None):
    """rsx_release_stream: free the library's workspace of (current device, stream)."""
    lib().rsx_release_stream(_stream_ptr(stream))


def radix_sort_pairs_inplace_async(keys, keys_scratch, vals, vals_scratch, dtype=None, order=ASCENDING, stream=None):
    """rsx_sort_pairs_inplace_async: keys and payloads sorted in place by the keys, no host synchronisation."""
    _check_dev(keys, keys_scratch, vals, vals_scratch)
    code = _torch_dtype_code(keys) if dtype is None else dtype
    if keys.element_size() != DTYPE_SIZE[code] or vals.element_size() not in (4, 8) or vals.numel() != keys.numel():
        raise RsxError("keys/vals do not match")
    _same_shape(keys, keys_scratch, "keys_scratch")
    _same_shape(vals, vals_scratch, "vals_scratch")
    check(lib().rsx_sort_pairs_inplace_async(keys.data_ptr(), keys_scratch.data_ptr(), vals.data_ptr(), vals_scratch.data_ptr(),
                                             keys.numel(), code, vals.element_size(), order, _stream_ptr(stream)))
    return keys, vals


def radix_sort_rank_inplace_async(src, index_buffer, dtype=None, order=ASCENDING, stream=None):
    """rsx_sort_rank_inplace_async: the stable argsort of ``src`` without a host synchronisation; the ranks always end in
    ``index_buffer[:n]`` (``index_buffer``: 2n int32 / int64 entries).  Returns that view."""
    _check_dev(src, index_buffer)
    code = _torch_dtype_code(src) if dtype is None else dtype
    n = src.numel()
    if src.element_size() != DTYPE_SIZE[code] or index_buffer.element_size() not in (4, 8) or index_buffer.numel() < 2 * n:
        raise RsxError("index_buffer must hold 2n 4- or 8-byte entries")
    check(lib().rsx_sort_rank_inplace_async(src.data_ptr(), index_buffer.data_ptr(), n, code, index_buffer.element_size(), order,
                                            _stream_ptr(stream)))
    return index_buffer[:n]


def verify_poll(stream=None):
    """rsx_verify_poll: wait for the stream and return the mismatches RSX_VERIFY=1 found in device-scheduled sorts since
    the last poll (raises RsxError if there are any)."""
    bad = C.c_uint64(0)
    check(lib().rsx_verify_poll(_stream_ptr(stream), C.byref(bad)))
    return int(bad.value)


def async_route(stream=None):
    """rsx_async_route: wait for the stream and return the route (as rsx_info.hybrid) the last radix_sort_inplace_async on it took."""
    r = C.c_uint32(0)
    check(lib().rsx_async_route(_stream_ptr(stream), C.byref(r)))
    return int(r.value)


def radix_sort_pairs(keys, keys_aux, vals, vals_aux, dtype=None, order=ASCENDING, stream=None):
    """Stable key+payload sort (struct-of-arrays); returns (keys_result, vals_result, info)."""
    _check_dev(keys, keys_aux, vals, vals_aux)
    code = _torch_dtype_code(keys) if dtype is None else dtype
    if keys.element_size() != DTYPE_SIZE[code] or vals.numel() != keys.numel() or vals.element_size() not in (4, 8):
        raise RsxError("keys/vals do not match")
    _same_shape(keys, keys_aux, "keys_aux")
    _same_shape(vals, vals_aux, "vals_aux")
    info = Info()
    check(lib().rsx_sort_pairs_device(keys.data_ptr(), keys_aux.data_ptr(), vals.data_ptr(), vals_aux.data_ptr(),
                                      keys.numel(), code, vals.element_size(), order, _stream_ptr(stream),
                                      C.byref(info)))
    if info.result_in_aux:
        return keys_aux, vals_aux, info
    return keys, vals, info


def radix_sort_rank(src, index_buffer, dtype=None, order=ASCENDING, stream=None):
    """radix_sort_rank(src, index_buffer, n) on device tensors (radix_sort_rank.hpp:97-112).

    ``index_buffer`` holds 2n int32/int64 entries; returns (ranks_view, info) where
    ranks_view is the half of index_buffer the reference would return.
    """
    _check_dev(src, index_buffer)
    code = _torch_dtype_code(src) if dtype is None else dtype
    n = src.numel()
    if src.element_size() != DTYPE_SIZE[code]:
        raise RsxError("src does not match the key type")
    if index_buffer.numel() < 2 * n or index_buffer.element_size() not in (4, 8):
        raise RsxError("index_buffer must hold 2n 4- or 8-byte entries")
    res, info = C.c_void_p(), Info()
    check(lib().rsx_sort_rank_device(src.data_ptr(), index_buffer.data_ptr(), n, code, index_buffer.element_size(),
                                     order, _stream_ptr(stream), C.byref(res), C.byref(info)))
    half = index_buffer[n:2 * n] if info.result_in_aux else index_buffer[:n]
    return half, info


def fill_splitmix(t, seed, mask=0xFFFFFFFFFFFFFFFF, first_index=0, stream=None):
    """Fill a device tensor with the SURVEY.md section 4 / 8d splitmix64 sequence (counter-based on the GPU)."""
    _check_dev(t)
    check(lib().rsx_fill_splitmix_device(t.data_ptr(), t.numel(), t.element_size(), seed, mask, first_index,
                                         _stream_ptr(stream)))
    return t


def spin(microseconds, stream=None):
    """Keep the (current) stream busy for about `microseconds`."""
    require_gpu()
    check(lib().rsx_spin_device(int(microseconds), _stream_ptr(stream)))


def profile_begin():
    check(lib().rsx_profile_begin())


def profile_end():
    p = Profile()
    check(lib().rsx_profile_end(C.byref(p)))
    return p


# ---- host (numpy) entry points: the C ABI exactly as the C++ template wrapper calls it -----

def radix_sort_host(src, aux, dtype, order=ASCENDING):
    """rsx_sort on host numpy buffers; returns (result_array, info)."""
    res, info = C.c_void_p(), Info()
    check(lib().rsx_sort(src.ctypes.data, aux.ctypes.data, src.size, dtype, order, C.byref(res), C.byref(info)))
    return (aux if info.result_in_aux else src), info


def radix_sort_unique_host(src, aux, dtype, order=ASCENDING, counts=None):
    """rsx_sort_unique on host numpy buffers; returns (result[:n_unique], counts[:n_unique] or None, info).  ``counts``: a
    numpy array of 4- or 8-byte integers with room for n entries."""
    res, nu, info = C.c_void_p(), C.c_size_t(0), UniqueInfo()
    cptr, cbytes = (None, 0) if counts is None else (counts.ctypes.data, counts.itemsize)
    check(lib().rsx_sort_unique(src.ctypes.data, aux.ctypes.data, src.size, dtype, order, cptr, cbytes, C.byref(res), C.byref(nu),
                                C.byref(info)))
    out = aux if (src.size and res.value == aux.ctypes.data and res.value != src.ctypes.data) else src
    return out[:nu.value], (None if counts is None else counts[:nu.value]), info


def radix_sort_group_host(src, dtype, order=ASCENDING, idx_dtype=None, keys=False, counts=False, first=False, inverse=True):
    """rsx_sort_group on a host numpy buffer; returns (inverse, keys[:G] or None, counts[:G] or None, first[:G] or None, info)
    as radix_sort_group does (``idx_dtype``: a 4- or 8-byte numpy integer type, default uint32; an output may also be given
    as a numpy array with room for n elements)."""
    import numpy as np
    if src.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("src does not match the key type")
    n = src.size
    idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)

    def buf(want, what, dt):
        if want is False or want is None:
            return None
        if want is True:
            return np.empty(n, dtype=dt)
        if want.size < n or want.itemsize != np.dtype(dt).itemsize:
            raise RsxError("%s must have room for n elements of the right size" % what)
        return want

    inv, k = buf(inverse, "inverse", idx_dtype), buf(keys, "keys", src.dtype)
    cn, fi = buf(counts, "counts", idx_dtype), buf(first, "first", idx_dtype)
    ptr = lambda a: None if a is None else a.ctypes.data
    ng, info = C.c_size_t(0), GroupInfo()
    check(lib().rsx_sort_group(src.ctypes.data, n, dtype, order, ptr(inv), ptr(k), ptr(cn), ptr(fi), idx_dtype.itemsize,
                               C.byref(ng), C.byref(info)))
    g = ng.value
    cut = lambda a: None if a is None else a[:g]
    return (None if inv is None else inv[:n]), cut(k), cut(cn), cut(fi), info


def radix_sort_reduce_host(keys, vals, dtype, val_dtype, order=ASCENDING, idx_dtype=None, sum=True, min=False, max=False, counts=False,
                           keys_out=True):
    """rsx_sort_reduce on host numpy buffers; returns (keys[:G], counts[:G], sum[:G], min[:G], max[:G], info), None where one was
    not asked for, as radix_sort_reduce does (``idx_dtype``: a 4- or 8-byte numpy integer type, default uint32; ``sum`` comes as
    uint64 bit patterns for integer values and float64 for float values; an output may also be given as a numpy array with room
    for n elements)."""
    import numpy as np
    if keys.itemsize != DTYPE_SIZE[dtype] or vals.itemsize != DTYPE_SIZE[val_dtype] or vals.size < keys.size:
        raise RsxError("keys / vals do not match their types")
    n = keys.size
    idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)
    sum_dtype = np.float64 if val_dtype in (F32, F64) else np.uint64

    def buf(want, what, dt):
        if want is False or want is None:
            return None
        if want is True:
            return np.empty(n, dtype=dt)
        if want.size < n or want.itemsize != np.dtype(dt).itemsize:
            raise RsxError("%s must have room for n elements of the right size" % what)
        return want

    k, cn, sm = buf(keys_out, "keys_out", keys.dtype), buf(counts, "counts", idx_dtype), buf(sum, "sum", sum_dtype)
    mn, mx = buf(min, "min", vals.dtype), buf(max, "max", vals.dtype)
    ptr = lambda a: None if a is None else a.ctypes.data
    ng, info = C.c_size_t(0), ReduceInfo()
    check(lib().rsx_sort_reduce(keys.ctypes.data, vals.ctypes.data, n, dtype, order, val_dtype, _reduce_ops(sm, mn, mx), ptr(k), ptr(cn),
                                idx_dtype.itemsize, ptr(sm), ptr(mn), ptr(mx), C.byref(ng), C.byref(info)))
    g = ng.value
    cut = lambda a: None if a is None else a[:g]
    return cut(k), cut(cn), cut(sm), cut(mn), cut(mx), info


def radix_sort_rankdata_host(src, dtype, order=ASCENDING, idx_dtype=None, place=True, less=False, equal=False):
    """rsx_sort_rankdata on a host numpy buffer; returns (place, less, equal, info) as radix_sort_rankdata does (``idx_dtype``:
    a 4- or 8-byte numpy integer type, default uint32; an output may also be given as a numpy array with room for n elements)."""
    import numpy as np
    if src.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("src does not match the key type")
    n = src.size
    idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)

    def buf(want, what):
        if want is False or want is None:
            return None
        if want is True:
            return np.empty(n, dtype=idx_dtype)
        if want.size < n or want.itemsize != idx_dtype.itemsize:
            raise RsxError("%s must have room for n elements of the right size" % what)
        return want

    pl, le, eq = buf(place, "place"), buf(less, "less"), buf(equal, "equal")
    ptr = lambda a: None if a is None else a.ctypes.data
    info = RankdataInfo()
    check(lib().rsx_sort_rankdata(src.ctypes.data, n, dtype, order, ptr(pl), ptr(le), ptr(eq), idx_dtype.itemsize, C.byref(info)))
    cut = lambda a: None if a is None else a[:n]
    return cut(pl), cut(le), cut(eq), info


def radix_sort_topk_host(src, k, dtype, order=ASCENDING, want_idx=True, idx_dtype=None):
    """rsx_sort_topk on a host numpy buffer; returns (keys, idx or None, info) as radix_sort_topk does (``idx_dtype``: a
    4- or 8-byte numpy integer type; default uint32 when n < 2^32, otherwise uint64)."""
    import numpy as np
    k = int(k)
    keys = np.empty(k, dtype=src.dtype)
    idx = None
    if want_idx:
        idx = np.empty(k, dtype=idx_dtype if idx_dtype is not None else (np.uint32 if src.size < 2 ** 32 else np.uint64))
    info = TopkInfo()
    check(lib().rsx_sort_topk(src.ctypes.data, src.size, k, dtype, order, keys.ctypes.data, None if idx is None else idx.ctypes.data,
                              4 if idx is None else idx.itemsize, C.byref(info)))
    return keys, idx, info


def radix_sort_nth_host(src, ranks, dtype, order=ASCENDING, want_idx=True, idx_dtype=None):
    """rsx_sort_nth on a host numpy buffer; returns (keys, idx or None, n_less, n_equal, info) as radix_sort_nth does
    (``idx_dtype``: a 4- or 8-byte numpy integer type; default uint32 when n < 2^32, otherwise uint64)."""
    import numpy as np
    if src.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("src does not match the key type")
    r, n_less, n_equal = _nth_ranks(ranks, src.size)
    keys = np.empty(r.size, dtype=src.dtype)
    idx = None
    if want_idx:
        idx = np.empty(r.size, dtype=idx_dtype if idx_dtype is not None else (np.uint32 if src.size < 2 ** 32 else np.uint64))
    info = NthInfo()
    check(lib().rsx_sort_nth(src.ctypes.data, src.size, _u64p(r), r.size, dtype, order, keys.ctypes.data,
                             None if idx is None else idx.ctypes.data, 4 if idx is None else idx.itemsize, _u64p(n_less),
                             _u64p(n_equal), C.byref(info)))
    return keys, idx, n_less, n_equal, info


def radix_sort_locate_host(src, vals, dtype, order=ASCENDING, idx_dtype=None, less=True, equal=False, bins=False, below=False):
    """rsx_sort_locate on host numpy buffers; returns (info, less, equal, bins) as radix_sort_locate does (``idx_dtype``: a 4- or
    8-byte numpy integer type, default uint32; an output may also be given as a numpy array with room for its elements)."""
    import numpy as np
    vals = np.ascontiguousarray(vals)
    if src.itemsize != DTYPE_SIZE[dtype] or vals.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("src and vals do not match the key type")
    n, m = src.size, vals.size
    idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)

    def buf(want, count, what):
        if want is False or want is None:
            return None
        if want is True:
            return np.empty(count, dtype=idx_dtype)
        if want.size < count or want.itemsize != idx_dtype.itemsize:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    le, eq, bi = buf(less, m, "less"), buf(equal, m, "equal"), buf(bins, n, "bins")
    ptr = lambda a: None if a is None else a.ctypes.data
    info = LocateInfo()
    check(lib().rsx_sort_locate(src.ctypes.data, n, vals.ctypes.data, m, dtype, order, ptr(le), ptr(eq), ptr(bi), idx_dtype.itemsize,
                                LOCATE_BINS_BELOW if below else 0, C.byref(info)))
    cut = lambda a, count: None if a is None else a[:count]
    return info, cut(le, m), cut(eq, m), cut(bi, n)


def radix_sort_partition_host(src, edges, dtype, order=ASCENDING, idx_dtype=None, keys=True, idx=False, offsets=True, below=False):
    """rsx_sort_partition on host numpy buffers; returns (info, keys, idx, offsets) as radix_sort_partition does (``idx_dtype``: a
    4- or 8-byte numpy integer type, default uint32; an output may also be given as a numpy array with room for its elements)."""
    import numpy as np
    src, edges = np.ascontiguousarray(src), np.ascontiguousarray(edges)
    if src.itemsize != DTYPE_SIZE[dtype] or edges.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("src and edges do not match the key type")
    n, m = src.size, edges.size
    idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)

    def buf(want, count, what, dt):
        if want is False or want is None:
            return None
        if want is True:
            return np.empty(count, dtype=dt)
        if want.size < count or want.itemsize != np.dtype(dt).itemsize:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    ke, ix, of = buf(keys, n, "keys", src.dtype), buf(idx, n, "idx", idx_dtype), buf(offsets, m + 2, "offsets", idx_dtype)
    ptr = lambda a: None if a is None else a.ctypes.data
    info = PartitionInfo()
    check(lib().rsx_sort_partition(src.ctypes.data, n, edges.ctypes.data, m, dtype, order, ptr(ke), ptr(ix), ptr(of), idx_dtype.itemsize,
                                   PARTITION_BELOW if below else 0, C.byref(info)))
    cut = lambda a, count: None if a is None else a[:count]
    return info, cut(ke, n), cut(ix, n), cut(of, m + 2)


def radix_sort_segments_host(src, dtype, offsets=None, rows=None, order=ASCENDING, idx_dtype=None, keys=True, idx=False, local_idx=False):
    """rsx_sort_segments on host numpy buffers; returns (info, keys, idx) as radix_sort_segments does (``offsets``: a numpy array of
    m + 1 4- or 8-byte integers, or ``rows``; ``idx_dtype``: default the offsets' type or uint32)."""
    import numpy as np
    src = np.ascontiguousarray(src)
    if src.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("src does not match the key type")
    n = src.size
    if (offsets is None) == (rows is None):
        raise RsxError("radix_sort_segments_host: give either offsets or rows")
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets)
        if offsets.size < 1 or offsets.itemsize not in (4, 8):
            raise RsxError("offsets must hold m + 1 entries of 4 or 8 bytes")
        m = offsets.size - 1
        idx_dtype = np.dtype(offsets.dtype if idx_dtype is None else idx_dtype)
        if idx_dtype.itemsize != offsets.itemsize:
            raise RsxError("offsets and idx must have elements of the same size")
    else:
        m = int(rows)
        idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)

    def buf(want, what, dt):
        if want is False or want is None:
            return None
        if want is True:
            return np.empty(n, dtype=dt)
        if want.size < n or want.itemsize != np.dtype(dt).itemsize:
            raise RsxError("%s must have room for its elements of the right size" % what)
        return want

    ke, ix = buf(keys, "keys", src.dtype), buf(idx, "idx", idx_dtype)
    ptr = lambda a: None if a is None else a.ctypes.data
    info = SegmentsInfo()
    check(lib().rsx_sort_segments(src.ctypes.data, n, ptr(offsets), m, idx_dtype.itemsize, dtype, order, ptr(ke), ptr(ix),
                                  SEGMENTS_LOCAL_IDX if local_idx else 0, C.byref(info)))
    cut = lambda a: None if a is None else a[:n]
    return info, cut(ke), cut(ix)


def radix_sort_join_host(left, right, dtype, order=ASCENDING, how="inner", idx_dtype=None):
    """rsx_sort_join and rsx_join_pairs on host numpy buffers; returns (left_idx, right_idx, info, start, count, right_perm)
    (``idx_dtype``: a 4- or 8-byte numpy integer type, default uint32; a missing match under how="left" is all ones)."""
    import numpy as np
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    if left.itemsize != DTYPE_SIZE[dtype] or right.itemsize != DTYPE_SIZE[dtype]:
        raise RsxError("left and right do not match the key type")
    flags = _join_how(how)
    n, m = left.size, right.size
    idx_dtype = np.dtype(np.uint32 if idx_dtype is None else idx_dtype)
    st, ct, pm = np.empty(n, dtype=idx_dtype), np.empty(n, dtype=idx_dtype), np.empty(m, dtype=idx_dtype)
    info, pairs = JoinInfo(), C.c_uint64(0)
    check(lib().rsx_sort_join(left.ctypes.data, n, right.ctypes.data, m, dtype, order, st.ctypes.data, ct.ctypes.data, pm.ctypes.data,
                              idx_dtype.itemsize, flags, C.byref(pairs), C.byref(info)))
    total = int(pairs.value)
    li, ri = np.empty(total, dtype=idx_dtype), np.empty(total, dtype=idx_dtype)
    check(lib().rsx_join_pairs(st.ctypes.data, ct.ctypes.data, pm.ctypes.data, n, m, idx_dtype.itemsize, flags, li.ctypes.data,
                               ri.ctypes.data, total, C.byref(pairs)))
    if int(pairs.value) != total:
        raise RsxError("rsx_join_pairs found %d pairs, rsx_sort_join %d" % (int(pairs.value), total))
    return li, ri, info, st, ct, pm


def radix_sort_lex_host(cols, dtypes, orders=None, idx_dtype=None):
    """rsx_sort_lex on host numpy columns (``cols[0]`` the most significant); returns (idx, info).  ``idx_dtype``: a 4- or
    8-byte numpy integer type; default uint32 when n < 2^32, otherwise uint64."""
    import numpy as np
    cols = list(cols)
    n = cols[0].size if cols else 0
    idx = np.empty(n, dtype=idx_dtype if idx_dtype is not None else (np.uint32 if n < 2 ** 32 else np.uint64))
    arr = _lex_cols([a.ctypes.data for a in cols], list(dtypes), orders)
    info = LexInfo()
    check(lib().rsx_sort_lex(arr, len(cols), n, idx.ctypes.data, idx.itemsize, C.byref(info)))
    return idx, info


def radix_sort_multi_host(src, aux, dtype, order=ASCENDING, devices=None):
    """rsx_sort_multi on host numpy buffers: one process, the work spread over `devices` (HIP device indices, one per rank;
    default: every visible device once).  Returns (result_array, info) with the reference's returned-pointer rule."""
    if devices is None:
        devices = list(range(max(device_count(), 1)))
    dev = (C.c_int * len(devices))(*devices)
    res, info = C.c_void_p(), Info()
    check(lib().rsx_sort_multi(src.ctypes.data, aux.ctypes.data, src.size, dtype, order, dev, len(devices), C.byref(res),
                               C.byref(info)))
    return (aux if info.result_in_aux else src), info


def radix_sort_rank_host(src, index_buffer, dtype, order=ASCENDING):
    res, info = C.c_void_p(), Info()
    n = src.size
    check(lib().rsx_sort_rank(src.ctypes.data, index_buffer.ctypes.data, n, dtype, index_buffer.itemsize, order,
                              C.byref(res), C.byref(info)))
    return (index_buffer[n:2 * n] if info.result_in_aux else index_buffer[:n]), info


def radix_sort_records_tagged_host(src, aux, key_offset, key_dtype, order=ASCENDING):
    """rsx_sort_records_tagged: numpy records (structured array or 2-D rows) ordered by the scalar field at key_offset."""
    res, info = C.c_void_p(), Info()
    n = len(src)
    rec_bytes = src.nbytes // max(n, 1)
    check(lib().rsx_sort_records_tagged(src.ctypes.data, aux.ctypes.data, n, rec_bytes, key_offset, key_dtype, order,
                                        C.byref(res), C.byref(info)))
    return (aux if info.result_in_aux else src), info


def radix_sort_records_tagged(src, aux, rec_bytes, key_offset, key_dtype, order=ASCENDING, stream=None):
    """rsx_sort_records_tagged_device on torch uint8 tensors holding n records of rec_bytes each."""
    require_gpu()
    _check_dev(src, aux)
    nbytes = src.numel() * src.element_size()
    if rec_bytes <= 0 or nbytes % rec_bytes:
        raise RsxError("src holds %d bytes: not a whole number of %d-byte records" % (nbytes, rec_bytes))
    if aux.numel() * aux.element_size() < nbytes:
        raise RsxError("aux is smaller than src")
    if key_offset < 0 or key_offset + DTYPE_SIZE[key_dtype] > rec_bytes:
        raise RsxError("the key does not lie inside the record")
    res, info = C.c_void_p(), Info()
    n = nbytes // rec_bytes
    check(lib().rsx_sort_records_tagged_device(src.data_ptr(), aux.data_ptr(), n, rec_bytes, key_offset, key_dtype, order,
                                               _stream_ptr(stream), C.byref(res), C.byref(info)))
    return (aux if res.value == aux.data_ptr() else src), info


def radix_sort_records_host(src, aux, keys):
    """rsx_sort_records: records (numpy structured / 2-D array rows) ordered by precomputed unsigned keys."""
    res, info = C.c_void_p(), Info()
    n = keys.size
    rec_bytes = src.nbytes // max(n, 1)
    check(lib().rsx_sort_records(src.ctypes.data, aux.ctypes.data, n, rec_bytes, keys.ctypes.data, keys.itemsize,
                                 C.byref(res), C.byref(info)))
    return (aux if info.result_in_aux else src), info
