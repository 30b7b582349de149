"""Shared by tests/test_gpu_segments*.py and tests/test_segments_lib_cpu.py: many independent arrays sorted in one call, from NumPy on
the ORACLE's derived keys (never from the code under test) -- per segment, np.argsort(ol.kdf_keys(seg), kind="stable") --, the LDS
route's classes and caps restated from radix_sorting_amd/csrc/rsx_segments_shape.hpp, and one way to call rsx_sort_segments_device.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import radix_sorting_amd as rsa

COPY, WAVE, GROUP, BLOCK, LONG = range(5)
CLASSES = 5
LDS_BYTES = 163840     # a CU's LDS: what one workgroup may declare
TEAM_FIXED, CAP_STEP, IDX_BYTES = 256, 256, 2
COPY_MAX, WAVE_MAX, GROUP_MAX = 1, 256, 2048
TEAM_WAVES = {WAVE: 1, GROUP: 4, BLOCK: 16}
WG_TEAMS = {COPY: 256, WAVE: 4, GROUP: 1, BLOCK: 1}


# ---- rsx_segments_shape.hpp, restated ------------------------------------------------------------------------------------------
def elem_bytes(key_bytes, with_idx):
    return key_bytes + (IDX_BYTES if with_idx else 0)


def team_bytes(waves, key_bytes, with_idx, stride):
    return waves * 1024 + TEAM_FIXED + 2 * stride * elem_bytes(key_bytes, with_idx)


def cap(key_bytes, with_idx):
    room = LDS_BYTES - 16 * 1024 - TEAM_FIXED
    return min(room // (2 * elem_bytes(key_bytes, with_idx)) // CAP_STEP * CAP_STEP, 65536)


def cap_of(dt, with_idx):
    return cap(ol.DTYPE_SIZE[dt], with_idx)


def class_of(length, cap_):
    if length <= COPY_MAX:
        return COPY
    if length > cap_:
        return LONG
    return WAVE if length <= WAVE_MAX else GROUP if length <= GROUP_MAX else BLOCK


def stride(cls, max_len, cap_):
    if cls == WAVE:
        return min(WAVE_MAX, cap_)
    if cls == GROUP:
        return min(GROUP_MAX, cap_)
    if cls != BLOCK:
        return 0
    return min(-(-max_len // CAP_STEP) * CAP_STEP, cap_)


def lds_bytes(cls, key_bytes, with_idx, max_len):
    if cls not in TEAM_WAVES:
        return 0
    return WG_TEAMS[cls] * team_bytes(TEAM_WAVES[cls], key_bytes, with_idx, stride(cls, max_len, cap(key_bytes, with_idx)))


def grid(cls, count):
    return -(-count // WG_TEAMS[cls])


def seam_lengths(cap_):
    """every length at which the code takes another path: 0, 1, 2, a wave's width, each class seam -1 / +0 / +1, cap -1 / +0 / +1"""
    out = [0, 1, 2, 63, 64, 65]
    for seam in (WAVE_MAX, GROUP_MAX, cap_):
        out += [seam - 1, seam, seam + 1]
    return out


# ---- the model -----------------------------------------------------------------------------------------------------------------
def uniform_offsets(n, m):
    assert m > 0 and n % m == 0
    return np.arange(m + 1, dtype=np.uint64) * np.uint64(n // m)


class Want:
    """What NumPy says about the segments [offsets[s], offsets[s + 1]) of the keys `bits`, each sorted on its own."""

    def __init__(self, bits, dt, offsets, order=ol.ASC):
        self.dt, self.order = dt, order
        self.bits = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
        self.offsets = np.ascontiguousarray(offsets).astype(np.int64)
        n, m = self.bits.size, self.offsets.size - 1
        assert self.offsets[0] == 0 and self.offsets[m] == n and (np.diff(self.offsets) >= 0).all()
        keys = ol.kdf_keys(self.bits, dt, order)
        self.local = np.zeros(n, dtype=np.uint64)
        for s in range(m):
            a, b = int(self.offsets[s]), int(self.offsets[s + 1])
            if b - a > 1:
                self.local[a:b] = np.argsort(keys[a:b], kind="stable")
        self.starts = np.repeat(self.offsets[:-1], np.diff(self.offsets)).astype(np.uint64)
        self.idx = self.local + self.starts
        self.keys = self.bits[self.idx.astype(np.int64)]
        self.lengths = np.diff(self.offsets)

    def classes(self, with_idx):
        """(class counts, max_len, n_long, cap) as rsx_segments_info reports them"""
        c = cap_of(self.dt, with_idx)
        counts = [0] * CLASSES
        for length in self.lengths:
            counts[class_of(int(length), c)] += 1
        return counts, int(self.lengths.max()) if self.lengths.size else 0, counts[LONG], c

    def natural_route(self, with_idx, force=None, max_long=rsa.SEGMENTS_DEFAULT_MAX_LONG):
        """The route is a function of the class counts and the switches.  force: what RSX_SEGMENTS_FORCE is set to (None, "1", "2")."""
        counts, _, n_long, _ = self.classes(with_idx)
        if self.bits.size == 0 or self.lengths.size == 0:
            return rsa.SEGMENTS_TRIVIAL
        lds = rsa.SEGMENTS_LDS if n_long == 0 else rsa.SEGMENTS_MIXED
        if force == "2" or n_long > max_long:
            return rsa.SEGMENTS_LEX
        if force == "1":
            return lds
        by_default = all(rsa.SEGMENTS_DEFAULT_CLASSES >> cls & 1 for cls in (WAVE, GROUP, BLOCK) if counts[cls])
        return lds if by_default else rsa.SEGMENTS_LEX


def call_device(src_t, n, off_t, m, dt, order, idx_bytes, keys_t=None, idx_t=None, flags=0, stream=None):
    """rsx_sort_segments_device on device tensors (None: that output is not asked for; off_t None: uniform rows).  Returns (rc, info)."""
    import torch
    info = rsa.SegmentsInfo()
    s = stream if stream is not None else torch.cuda.current_stream()
    p = lambda t: None if t is None else t.data_ptr()
    rc = rsa.lib().rsx_sort_segments_device(p(src_t), n, p(off_t), m, idx_bytes, dt, order, p(keys_t), p(idx_t), flags,
                                            C.c_void_p(s.cuda_stream), C.byref(info))
    return rc, info


def _host(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64).astype(np.uint64)


def _bits(t, dt):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(ol.NP_BITS[dt])


def check(tag, want, src_t, off_t, keys_t, idx_t, local, info, route=None):
    """The outputs (device tensors / numpy arrays of exactly n elements, or None) against NumPy; src and offsets unchanged; the
    info's classes against the model's."""
    n = want.bits.size
    if keys_t is not None:
        got = _bits(keys_t, want.dt)
        assert got.size == n and np.array_equal(got, want.keys), (tag, "keys", np.flatnonzero(got != want.keys)[:8], got[:8], want.keys[:8])
    if idx_t is not None:
        got, widx = _host(idx_t), (want.local if local else want.idx)
        assert got.size == n and np.array_equal(got, widx), (tag, "idx", np.flatnonzero(got != widx)[:8], got[:8], widx[:8])
    if src_t is not None:
        assert np.array_equal(_bits(src_t, want.dt), want.bits), (tag, "src was written")
    if off_t is not None:
        assert np.array_equal(_host(off_t).astype(np.int64), want.offsets), (tag, "offsets was written")
    if route is not None:
        assert info.route == route, (tag, "route", info.route, route)
    assert info.key_bytes == ol.DTYPE_SIZE[want.dt], tag
    if info.route != rsa.SEGMENTS_TRIVIAL:
        counts, max_len, n_long, c = want.classes(idx_t is not None)
        assert info.cap == c and info.max_len == max_len and info.n_long == n_long, (tag, info.cap, c, info.max_len, max_len, info.n_long, n_long)
        assert info.classes() == counts, (tag, "classes", info.classes(), counts)
    if info.route == rsa.SEGMENTS_LDS:
        assert info.n_long == 0, tag
    if info.route == rsa.SEGMENTS_MIXED:
        assert info.n_long > 0 and info.sort.key_bytes == info.key_bytes, tag
    if info.route == rsa.SEGMENTS_LEX and n > 1:
        assert info.lex.ncols == 2 and info.lex.ngroups >= 1, (tag, info.lex.ncols, info.lex.ngroups)
