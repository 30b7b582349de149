"""Shared by tests/test_gpu_partition*.py and tests/test_partition_lib_cpu.py: the stable multi-way split of the keys by given
edges, from NumPy on the ORACLE's derived keys (never from the code under test) -- the bins are locate_lib.Want.bins, the order is
np.argsort(bins, kind="stable"), the keys are the input read through it and offsets[j] counts the bins below j --, the scatter
route's shape restated from radix_sorting_amd/csrc/rsx_partition_shape.hpp, and one way to call rsx_sort_partition_device.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import locate_lib as ll
import oracle_lib as ol
import radix_sorting_amd as rsa

TILE = rsa.PARTITION_TILE                                   # keys of one tile of the count and of the placement
SHARE = rsa.PARTITION_SHARE_TILES * rsa.PARTITION_TILE      # keys of the smallest share of a workgroup
BALLOT_PARTS = rsa.PARTITION_BALLOT_PARTS                   # the default seam between the two ranking forms (parts)


class Want(ll.Want):
    """What NumPy says about the split of the keys `bits` by a list of edges."""

    def split(self, edges, below):
        """(idx, keys, offsets): the input row of every output position (uint64), the raw keys in output order, the m + 2 offsets"""
        edges = np.ascontiguousarray(edges, dtype=ol.NP_BITS[self.dt])
        bins = self.bins(edges, below).astype(np.int64)
        idx = np.argsort(bins, kind="stable")
        offsets = np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=edges.size + 1))]).astype(np.uint64)
        assert offsets.size == edges.size + 2
        return idx.astype(np.uint64), self.bits[idx], offsets


def distinct_edges(edges, dt, order=ol.ASC):
    return int(np.unique(ol.kdf_keys(np.ascontiguousarray(edges, dtype=ol.NP_BITS[dt]), dt, order)).size)


def natural_route(edges, dt, order=ol.ASC, max_edges=rsa.PARTITION_MAX_EDGES):
    """The route is a function of the number of distinct edges and the switches, never of n (max_edges: what RSX_PARTITION_MAX_EDGES is
    set to; the GPU tests pin it to the most the scatter route takes, the library's default is rsa.PARTITION_DEFAULT_MAX_EDGES)"""
    return rsa.PARTITION_SCATTER if distinct_edges(edges, dt, order) <= max_edges else rsa.PARTITION_SORT


def rank_form(edges, dt, order=ol.ASC, seam=BALLOT_PARTS):
    """rsx_partition_shape.hpp's partition_rank_form: 1 (ballots) while the parts, D + 1, are at most the seam, else 2 (LDS cells)"""
    return 1 if distinct_edges(edges, dt, order) + 1 <= seam else 2


def shares(n, residue_bytes, key_bytes):
    """rsx_partition_shape.hpp's partition_grid: the workgroups over n keys whose first lies `residue_bytes` behind a 16-byte boundary"""
    head = min(n, ((16 - residue_bytes % 16) % 16) // key_bytes)
    tiles = (n - head) // TILE
    share_tiles = max(-(-tiles // 256), rsa.PARTITION_SHARE_TILES)
    return max(1, -(-tiles // share_tiles))


def call_device(src_t, n, edges_t, m, dt, order, idx_bytes, keys_t=None, idx_t=None, off_t=None, flags=0, stream=None):
    """rsx_sort_partition_device on device tensors (None: that output is not asked for).  Returns (rc, info)."""
    import torch
    info = rsa.PartitionInfo()
    s = stream if stream is not None else torch.cuda.current_stream()
    p = lambda t: None if t is None else t.data_ptr()
    rc = rsa.lib().rsx_sort_partition_device(p(src_t), n, p(edges_t), m, dt, order, p(keys_t), p(idx_t), p(off_t), idx_bytes, flags,
                                             C.c_void_p(s.cuda_stream), C.byref(info))
    return rc, info


def _host(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64).astype(np.uint64)


def _bits(t, dt):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(ol.NP_BITS[dt])


def check(tag, want, edges, src_t, edges_t, keys_t, idx_t, off_t, below, info, route=None, seam=BALLOT_PARTS):
    """The outputs (device tensors / numpy arrays of exactly n resp. m + 2 elements, or None) against NumPy; src and edges unchanged."""
    edges = np.ascontiguousarray(edges, dtype=ol.NP_BITS[want.dt])
    m, n = edges.size, want.bits.size
    widx, wkeys, woff = want.split(edges, below)
    if keys_t is not None:
        got = _bits(keys_t, want.dt)
        assert got.size == n and np.array_equal(got, wkeys), (tag, "keys", np.flatnonzero(got != wkeys)[:8], got[:8], wkeys[:8])
    if idx_t is not None:
        got = _host(idx_t)
        assert got.size == n and np.array_equal(got, widx), (tag, "idx", np.flatnonzero(got != widx)[:8], got[:8], widx[:8])
    if off_t is not None:
        got = _host(off_t)
        assert got.size == m + 2 and np.array_equal(got, woff), (tag, "offsets", np.flatnonzero(got != woff)[:8], got[:8], woff[:8])
    if src_t is not None:
        assert np.array_equal(_bits(src_t, want.dt), want.bits), (tag, "src was written")
    if edges_t is not None:
        assert np.array_equal(_bits(edges_t, want.dt), edges), (tag, "edges was written")
    if route is not None:
        assert info.route == route, (tag, "route", info.route, route)
    assert info.key_bytes == ol.DTYPE_SIZE[want.dt], tag
    if info.route == rsa.PARTITION_SCATTER:
        d, _, steps = ll.search_shape(edges, want.dt, want.order)
        assert info.input_reads == 2 and info.distinct_edges == d and info.search_steps == steps, (tag, info.distinct_edges, d, info.search_steps, steps)
        assert info.rank_form == (1 if d + 1 <= seam else 2), (tag, "rank_form", info.rank_form, d, seam)
        assert 1 <= info.shares <= 256, (tag, info.shares)
    elif info.route == rsa.PARTITION_SORT:
        assert (info.input_reads, info.search_steps, info.rank_form, info.shares) == (0, 0, 0, 0), tag
        assert info.locate.route in (rsa.LOCATE_TABLE, rsa.LOCATE_SEARCH, rsa.LOCATE_SORT), (tag, info.locate.route)
