"""rsx_sort_segments_device on the GPU against NumPy on the oracle's derived keys (tests/segments_lib.py), bit for bit: every case on the
route the library takes by itself, on the composed route (RSX_SEGMENTS_FORCE=2) and on the LDS / MIXED route (RSX_SEGMENTS_FORCE=1,
RSX_SEGMENTS_MAX_LONG pinned where segments too long for LDS exist), the route asserted, src and offsets unchanged.  Lengths at
every seam of the size classes, the shapes of m, uniform rows without offsets, inputs on which a per-call decision (kept columns,
pre-sorted exit) gives a wrong answer, stability, independence from a segment's position, bad offsets, streams."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa
import segments_lib as sg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_T = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NPI = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
FILL = -7
MAX_LONG = 8     # what RSX_SEGMENTS_MAX_LONG is pinned to under RSX_SEGMENTS_FORCE=1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes(monkeypatch):
    for name in ("RSX_SEGMENTS_FORCE", "RSX_SEGMENTS_MAX_LONG"):
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    for name in ("RSX_SEGMENTS_FORCE", "RSX_SEGMENTS_MAX_LONG"):
        monkeypatch.delenv(name, raising=False)
    rsa.reload_env()


def _set(monkeypatch, force, max_long=None):
    if force is None:
        monkeypatch.delenv("RSX_SEGMENTS_FORCE", raising=False)
    else:
        monkeypatch.setenv("RSX_SEGMENTS_FORCE", force)
    if max_long is None:
        monkeypatch.delenv("RSX_SEGMENTS_MAX_LONG", raising=False)
    else:
        monkeypatch.setenv("RSX_SEGMENTS_MAX_LONG", str(max_long))
    rsa.reload_env()


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_NPI[a.itemsize]).copy()).cuda()


def _offsets_dev(off, ib):
    return _dev(np.asarray(off).astype(np.uint32 if ib == 4 else np.uint64))


def _run(tag, monkeypatch, want, ib=4, keys=True, idx=True, local=False, uniform=False, forces=(None, "2", "1"), stream=None):
    """one case on every route asked for; returns the infos by force"""
    dt, n, m = want.dt, want.bits.size, want.offsets.size - 1
    kb = ol.DTYPE_SIZE[dt]
    src_t = _dev(want.bits)
    off_t = None if uniform else _offsets_dev(want.offsets, ib)
    infos = {}
    for force in forces:
        max_long = MAX_LONG if force == "1" else None
        _set(monkeypatch, force, max_long)
        keys_t = torch.full((n,), FILL, dtype=_T[kb], device="cuda") if keys else None
        idx_t = torch.full((n,), FILL, dtype=_T[ib], device="cuda") if idx else None
        rc, info = sg.call_device(src_t, n, off_t, m, dt, want.order, ib, keys_t, idx_t, rsa.SEGMENTS_LOCAL_IDX if local else 0, stream=stream)
        assert rc == 0, (tag, force, rsa.lib().rsx_last_error())
        torch.cuda.synchronize()
        route = want.natural_route(idx, force, MAX_LONG if force == "1" else rsa.SEGMENTS_DEFAULT_MAX_LONG)
        sg.check("%s force=%s" % (tag, force), want, src_t, off_t, keys_t, idx_t, local, info, route)
        infos[force] = info
    return infos


def _shuffled_offsets(lengths, seed):
    lengths = np.random.default_rng(seed).permutation(np.asarray(lengths, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(lengths)])


# ---- 1. lengths at every seam ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [ol.U8, ol.U16, ol.U32, ol.F32, ol.I64, ol.F64])
@pytest.mark.parametrize("outs", ["keys", "idx", "both"])
def test_lengths_at_every_seam(dt, outs, monkeypatch):
    keys, idx = outs != "idx", outs != "keys"
    cap = sg.cap_of(dt, idx)
    off = _shuffled_offsets(sg.seam_lengths(cap), 7000 + dt)
    bits = ol.splitmix_fill(int(off[-1]), dt, 7100 + dt)
    # idx bytes, local, order rotate over the cases so that every value of each meets every dtype and every output set
    k = dt + ["keys", "idx", "both"].index(outs)
    combos = ((4, False, ol.ASC), (8, True, ol.DESC)) if k % 2 == 0 else ((8, False, ol.ASC), (4, True, ol.DESC))
    if dt == ol.U32:     # ... and the other pairings of local / global with the order meet the seam lengths on one dtype
        combos += ((4, False, ol.DESC), (8, True, ol.ASC))
    for ib, local, order in combos:
        want = sg.Want(bits, dt, off, order)
        infos = _run("seams %s %s ib=%d local=%d order=%d" % (ol.DTYPE_NAMES[dt], outs, ib, local, order), monkeypatch, want, ib, keys, idx, local)
        assert infos["1"].route == rsa.SEGMENTS_MIXED and infos["1"].n_long == 1     # cap + 1 is counted in n_long
        assert infos["1"].sort.key_bytes == ol.DTYPE_SIZE[dt]


# ---- 2. shapes of m -------------------------------------------------------------------------------------------------------------
def test_one_segment_is_the_rank_sort(monkeypatch):
    for dt, n in ((ol.U32, 5000), (ol.F64, 7168), (ol.I16, 20011)):
        bits = ol.splitmix_fill(n, dt, 7200 + dt)
        want = sg.Want(bits, dt, [0, n])
        ranks, _, _, _ = ol.oracle_rank(bits, dt, 4)
        assert np.array_equal(want.idx, ranks.astype(np.uint64))
        _run("m=1 %s" % ol.DTYPE_NAMES[dt], monkeypatch, want)
        src_t = _dev(bits)
        ib_t = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        got, _ = rsa.radix_sort_rank(src_t, ib_t, dtype=dt)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32).astype(np.uint64), want.idx)


def test_shapes_of_m(monkeypatch):
    dt = ol.U32
    n = 3001
    bits = ol.splitmix_fill(n, dt, 7301)
    _run("m == n", monkeypatch, sg.Want(bits, dt, np.arange(n + 1)))
    # m == n + 5: empty segments at the front, in the middle and at the end
    off = np.concatenate([[0, 0, 0], np.arange(1, 1500), [1499, 1499], np.arange(1500, n + 1), [n]])
    assert off.size == n + 6
    _run("m == n + 5", monkeypatch, sg.Want(bits, dt, off), ib=8, local=True)
    _run("all keys in the last segment", monkeypatch, sg.Want(bits, dt, [0] * 40 + [n]))
    cap = sg.cap_of(dt, True)
    full = ol.splitmix_fill(cap, dt, 7302)
    infos = _run("1000 empty segments around one of cap keys", monkeypatch, sg.Want(full, dt, [0] * 501 + [cap] * 501))
    assert infos["1"].route == rsa.SEGMENTS_LDS and infos["1"].classes() == [1000, 0, 0, 1, 0]


# ---- 3. uniform rows without offsets --------------------------------------------------------------------------------------------
def test_uniform_rows_without_offsets(monkeypatch):
    dt = ol.F32
    cap = sg.cap_of(dt, True)
    for rows, cols in ((1, 4099), (4099, 1), (257, 33), (7, cap), (3, cap + 1)):
        n = rows * cols
        bits = ol.splitmix_fill(n, dt, 7400 + rows)
        want = sg.Want(bits, dt, sg.uniform_offsets(n, rows), ol.DESC if rows == 257 else ol.ASC)
        infos = _run("%d x %d" % (rows, cols), monkeypatch, want, ib=8 if rows == 7 else 4, local=rows != 1, uniform=True)
        assert infos["1"].route == (rsa.SEGMENTS_MIXED if cols > cap else rsa.SEGMENTS_LDS)
    x = torch.from_numpy(ol.splitmix_fill(257 * 33, ol.I32, 7450).view(np.int32).reshape(257, 33).copy()).cuda()
    for descending in (False, True):
        values, indices = rsa.sort_rows(x, descending=descending)
        tv, ti = torch.sort(x, dim=-1, descending=descending, stable=True)
        assert values.shape == tv.shape and indices.shape == ti.shape and indices.dtype == ti.dtype
        assert torch.equal(values, tv) and torch.equal(indices, ti)


# ---- 4. per-segment decisions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [ol.U32, ol.I64])
def test_per_segment_decisions(dt, monkeypatch):
    kb = ol.DTYPE_SIZE[dt]
    rng = np.random.default_rng(7500 + dt)
    ut = ol.NP_BITS[dt]
    parts = []
    for length in (12, 200, 1500, 5000):
        r = rng.integers(0, 256, size=(5, length)).astype(ut)
        base = ut(0x5A5A5A5A5A5A5A5A & ((1 << (8 * kb)) - 1))
        low, high = ut(0xFF), ut(0xFF) << ut(8 * (kb - 1))
        a = (base & ~low) | r[0]                                        # A varies only in byte 0
        b = (base & ~high) | (r[1] << ut(8 * (kb - 1)))                 # B only in the highest byte
        c = ol.splitmix_fill(length, dt, 7600 + length).astype(ut)      # C in all
        srt = np.sort(ol.splitmix_fill(length, dt, 7700 + length))      # bit patterns ascending ...
        keyed = srt[np.argsort(ol.kdf_keys(srt, dt), kind="stable")]   # ... and in the order of the derived keys: a sorted segment
        equal = np.full(length, c[0], dtype=ut)                         # a sorted segment of equal keys
        parts += [a, b, c, keyed, c[::-1].copy(), equal, keyed[::-1].copy(), a[:length // 2]]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    bits = np.concatenate(parts)
    for order in (ol.ASC, ol.DESC):
        _run("decisions %s order=%d" % (ol.DTYPE_NAMES[dt], order), monkeypatch, sg.Want(bits, dt, off, order), ib=4 if order == ol.ASC else 8,
             local=order == ol.DESC)


# ---- 5. stability ---------------------------------------------------------------------------------------------------------------
def test_stability(monkeypatch):
    lengths = [0, 1, 2, 40, 64, 65, 256, 257, 700, 2048, 2049, 6000, 11000, 300]
    off = _shuffled_offsets(lengths, 7800)
    n = int(off[-1])
    _run("u8", monkeypatch, sg.Want(ol.splitmix_fill(n, ol.U8, 7801), ol.U8, off), local=True)
    three = np.array([0x01000000, 0x00000002, 0xFF000300], dtype=np.uint32)[np.random.default_rng(7802).integers(0, 3, size=n)]
    _run("u32, 3 distinct values", monkeypatch, sg.Want(three, ol.U32, off))
    _run("u32, 3 distinct values, descending", monkeypatch, sg.Want(three, ol.U32, off, ol.DESC), ib=8)
    for dt, pats in ((ol.F32, [0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x3F800000, 0xBF800000]),
                     (ol.F64, [0x8000000000000000, 0x0, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001,
                               0x7FF0000000000001, 0x3FF0000000000000, 0xBFF0000000000000])):
        cap = sg.cap_of(dt, True)
        offf = _shuffled_offsets([x for x in lengths if x <= cap] + [cap], 7803)
        special = np.array(pats, dtype=ol.NP_BITS[dt])[np.random.default_rng(7804 + dt).integers(0, len(pats), size=int(offf[-1]))]
        _run("%s specials" % ol.DTYPE_NAMES[dt], monkeypatch, sg.Want(special, dt, offf), local=True)
        _run("%s specials, descending" % ol.DTYPE_NAMES[dt], monkeypatch, sg.Want(special, dt, offf, ol.DESC))


# ---- 6. independence from position ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [ol.U8, ol.U32, ol.U64])
def test_independence_from_position(dt, monkeypatch):
    kb = ol.DTYPE_SIZE[dt]
    per = 16 // kb     # elements to a 16-byte line
    lengths = [3, 17, 64, 100, 255, 256, 257, 300, 1000, 2047, 2048, 2049, 2500, 3000, 4097, 5000, 31, 1, 2, 6001]
    assert len(lengths) == 20
    contents = [ol.splitmix_fill(length, dt, 7900 + i) for i, length in enumerate(lengths)]
    results = []
    for shift in (0, 1):
        # a filler in front of segment i puts its start at element residue (i + shift) % per: the starts run through every residue
        # mod 16 bytes, and no segment starts at the same one in both layouts
        parts, cuts = [], [0]
        for i, c in enumerate(contents):
            fill = ol.splitmix_fill((i + shift - cuts[-1]) % per, dt, 7950 + i)
            parts += [fill, c]
            cuts += [cuts[-1] + fill.size, cuts[-1] + fill.size + c.size]
        bits = np.concatenate(parts)
        want = sg.Want(bits, dt, cuts)
        starts = {(cuts[2 * i + 1] * kb) % 16 for i in range(20)}
        assert starts == {r * kb for r in range(per)}, (shift, sorted(starts))     # every residue mod 16 bytes an element can start at
        results.append((want, cuts))
        src_t, off_t = _dev(bits), _offsets_dev(cuts, 4)
        for force in ("1", "2"):
            _set(monkeypatch, force, MAX_LONG)
            keys_t = torch.full((bits.size,), FILL, dtype=_T[kb], device="cuda")
            idx_t = torch.full((bits.size,), FILL, dtype=torch.int32, device="cuda")
            rc, info = sg.call_device(src_t, bits.size, off_t, len(cuts) - 1, dt, ol.ASC, 4, keys_t, idx_t, rsa.SEGMENTS_LOCAL_IDX)
            assert rc == 0, rsa.lib().rsx_last_error()
            torch.cuda.synchronize()
            sg.check("position shift=%d force=%s" % (shift, force), want, src_t, off_t, keys_t, idx_t, True, info)
            got_k, got_i = keys_t.cpu().numpy().view(ol.NP_BITS[dt]), idx_t.cpu().numpy()
            per_seg = [(got_k[cuts[2 * i + 1]:cuts[2 * i + 2]].copy(), got_i[cuts[2 * i + 1]:cuts[2 * i + 2]].copy()) for i in range(20)]
            results.append(per_seg)
    (_, _), a1, a2, (_, _), b1, b2 = results
    for x, y in ((a1, b1), (a2, b2), (a1, a2)):
        for (k0, i0), (k1, i1) in zip(x, y):
            assert np.array_equal(k0, k1) and np.array_equal(i0, i1)


# ---- 7. bad offsets -------------------------------------------------------------------------------------------------------------
def test_bad_offsets_are_refused_before_anything_is_written(monkeypatch):
    n = 5000
    bits = ol.splitmix_fill(n, ol.U32, 8001)
    good = np.array([0, 10, 10, 700, 3000, 3001, n])
    bads = []
    for at, value in ((3, 5), (0, 1), (6, n - 1), (6, n + 1)):     # decreasing in the middle, offsets[0] == 1, offsets[m] == n -/+ 1
        b = good.copy()
        b[at] = value
        bads.append(b)
    src_t = _dev(bits)
    for force in (None, "1", "2"):
        _set(monkeypatch, force, MAX_LONG if force == "1" else None)
        for ib in (4, 8):
            for b in bads:
                off_t = _offsets_dev(b, ib)
                keys_t = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
                idx_t = torch.full((n,), FILL, dtype=_T[ib], device="cuda")
                rc, _ = sg.call_device(src_t, n, off_t, good.size - 1, ol.U32, ol.ASC, ib, keys_t, idx_t)
                assert rc == -1 and b"bad offsets" in rsa.lib().rsx_last_error(), (force, ib, list(b))
                torch.cuda.synchronize()
                assert bool((keys_t == FILL).all()) and bool((idx_t == FILL).all()), (force, ib, list(b))
                assert np.array_equal(sg._host(off_t).astype(np.int64), b)
    assert np.array_equal(src_t.cpu().numpy().view(np.uint32), bits)


# ---- 8., 9. streams ------------------------------------------------------------------------------------------------------------
def test_capturing_stream_is_refused():
    n = 4096
    bits = ol.splitmix_fill(n, ol.U32, 8101)
    want = sg.Want(bits, ol.U32, [0, 100, n])
    src_t, off_t = _dev(bits), _offsets_dev([0, 100, n], 4)
    keys_t = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rc, info = sg.call_device(src_t, n, off_t, 2, ol.U32, ol.ASC, 4, keys_t, None, stream=s)     # (the context of this stream exists before the capture)
        assert rc == 0, rsa.lib().rsx_last_error()
    s.synchronize()
    sg.check("before the capture", want, src_t, off_t, keys_t, None, False, info)
    keys_t.fill_(FILL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, _ = sg.call_device(src_t, n, off_t, 2, ol.U32, ol.ASC, 4, keys_t, None, stream=torch.cuda.current_stream())
        err = rsa.lib().rsx_last_error()
    assert rc == -1 and b"capturing" in err
    torch.cuda.synchronize()
    assert bool((keys_t == FILL).all())
    rsa.lib().rsx_release_stream(s.cuda_stream)


def test_side_stream(monkeypatch):
    off = _shuffled_offsets([0, 1, 30, 300, 3000, 9000, 13000, 2], 8201)
    want = sg.Want(ol.splitmix_fill(int(off[-1]), ol.I32, 8202), ol.I32, off)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _run("side stream", monkeypatch, want, local=True, stream=stream)
    stream.synchronize()
    rsa.lib().rsx_release_stream(stream.cuda_stream)


# ---- 10. the info of a forced MIXED call ------------------------------------------------------------------------------------------
def test_info_of_a_mixed_call(monkeypatch):
    dt = ol.U64
    cap = sg.cap_of(dt, True)
    lengths = [cap + 1, 0, 5, 1, cap + 700, 300, 300, 2500, cap, 0, 2 * cap, 64, 1]
    off = np.concatenate([[0], np.cumsum(lengths)])
    want = sg.Want(ol.splitmix_fill(int(off[-1]), dt, 8301), dt, off)
    infos = _run("mixed", monkeypatch, want, ib=8, forces=("1",))
    info = infos["1"]
    counts, max_len, n_long, c = want.classes(True)
    assert info.route == rsa.SEGMENTS_MIXED and info.n_long == n_long == 3 and info.classes() == counts == [4, 2, 2, 2, 3]
    assert info.max_len == max_len == 2 * cap and info.cap == c == cap and info.sort.key_bytes == 8
    # one long segment more than the pinned RSX_SEGMENTS_MAX_LONG: the composed route
    _set(monkeypatch, "1", 2)
    src_t, off_t = _dev(want.bits), _offsets_dev(off, 8)
    idx_t = torch.full((want.bits.size,), FILL, dtype=torch.int64, device="cuda")
    rc, info = sg.call_device(src_t, want.bits.size, off_t, len(lengths), dt, ol.ASC, 8, None, idx_t)
    assert rc == 0, rsa.lib().rsx_last_error()
    torch.cuda.synchronize()
    sg.check("mixed, too many long", want, src_t, off_t, None, idx_t, False, info, rsa.SEGMENTS_LEX)
