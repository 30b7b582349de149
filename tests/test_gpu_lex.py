"""rsx_sort_lex_device on the GPU: the stable argsort by several key columns, against the oracle's chained rank sorts
(lex_lib.want_perm).

Every case runs at RSX_LEX_PACK_BYTES = 1, 4 and 8, asserts the info.group[] table against the grouping rule restated in
lex_lib.want_groups, compares the permutation with the oracle's element for element (so the three packings are identical) and
compares every column byte for byte with its original after every call.  The expected permutation is computed once per
(shape, pattern, n) and shared by the three packings; the long sizes run for a subset of the shapes only."""
import os
import subprocess

import numpy as np
import pytest

import lex_lib as ll
import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IT = {4: torch.int32, 8: torch.int64}
PACKS = (1, 4, 8)
A, D = ol.ASC, ol.DESC

SHORT = [2, 3, 255, 256, 257, 1023, 1025, 4099, 65537]
LONG = SHORT + [300001, (1 << 20) + 3]
# name -> (dtypes, orders, sizes)
SHAPES = {
    "u16,u16": ([ol.U16, ol.U16], [A, A], LONG),
    "4 x u8": ([ol.U8] * 4, [A] * 4, SHORT),
    "u8,u16,u8": ([ol.U8, ol.U16, ol.U8], [A, A, A], SHORT),
    "i8,f32": ([ol.I8, ol.F32], [A, A], SHORT),
    "u32,u32": ([ol.U32, ol.U32], [A, A], LONG),
    "f32 desc,i32": ([ol.F32, ol.I32], [D, A], SHORT),
    "u64,u32": ([ol.U64, ol.U32], [A, A], LONG),
    "f64,f64 desc,i64": ([ol.F64, ol.F64, ol.I64], [A, D, A], SHORT),
    "9 x u8": ([ol.U8] * 9, [A, D, A, A, D, A, A, A, D], SHORT),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_switches(monkeypatch):
    monkeypatch.delenv("RSX_LEX_PACK_BYTES", raising=False)
    rsa.reload_env()
    yield
    torch.cuda.synchronize()
    monkeypatch.delenv("RSX_LEX_PACK_BYTES", raising=False)
    rsa.reload_env()


def pack(monkeypatch, P):
    if P is None:
        monkeypatch.delenv("RSX_LEX_PACK_BYTES", raising=False)
    else:
        monkeypatch.setenv("RSX_LEX_PACK_BYTES", str(P))
    rsa.reload_env()


def tie_mask(dt, bits):
    """The low `bits` bits and the top bit: few distinct values of both signs."""
    return ((1 << bits) - 1) | (1 << (8 * ol.DTYPE_SIZE[dt] - 1))


def make_cols(dtypes, n, seed, pattern):
    if pattern == "uniform":
        return [ol.splitmix_fill(n, dt, seed + j) for j, dt in enumerate(dtypes)]
    if pattern == "ties":
        return [ol.splitmix_fill(n, dt, seed + j, tie_mask(dt, 2 + (j & 1))) for j, dt in enumerate(dtypes)]
    if pattern == "one constant":
        cols = [ol.splitmix_fill(n, dt, seed + j, tie_mask(dt, 3)) for j, dt in enumerate(dtypes)]
        cols[len(cols) // 2][:] = 0x5A
        return cols
    raise ValueError(pattern)


class Case:
    """Columns on the device (with a device copy of each to compare with afterwards) and the oracle's permutation."""

    def __init__(self, cols, dtypes, orders, want=None, dev=None):
        self.cols = [np.ascontiguousarray(c, dtype=ol.NP_BITS[dt]) for c, dt in zip(cols, dtypes)]
        self.dtypes, self.orders, self.n = list(dtypes), list(orders), self.cols[0].size
        self.dev = [ll.to_dev(c) for c in self.cols] if dev is None else dev
        self.saved = [t.clone() for t in self.dev]
        self.want = ll.want_perm(self.cols, self.dtypes, self.orders) if want is None else want

    def run(self, tag, monkeypatch, packs=PACKS, idx_bytes=4, stream=None):
        """One call per packing limit; returns {P: info}."""
        arr = ll.lex_cols([t.data_ptr() for t in self.dev], self.dtypes, self.orders)
        infos = {}
        for P in packs:
            pack(monkeypatch, P)
            out = torch.full((self.n,), 0x5A, dtype=_IT[idx_bytes], device="cuda")
            sp = None if stream is None else stream.cuda_stream
            rc, err, info = ll.call_device_raw(arr, len(self.dev), self.n, out.data_ptr(), idx_bytes, sp)
            what = "%s n=%d P=%s ib=%d" % (tag, self.n, P, idx_bytes)
            assert rc == 0, (what, err)
            if stream is not None:
                stream.synchronize()
            else:
                torch.cuda.synchronize()
            got = out.cpu().numpy().astype(np.int64)
            assert np.array_equal(got, self.want), (what, "first difference at", int(np.flatnonzero(got != self.want)[0]))
            limit = 4 if P is None else P
            assert info.pack_bytes == limit and info.ncols == len(self.dtypes), what
            assert info.groups() == ll.want_groups(self.dtypes, limit), (what, info.groups())
            every = all(info.group[g].in_order for g in range(info.ngroups))
            assert info.early_exit == (2 if every else 0), (what, info.early_exit)
            for g in range(info.ngroups):
                grp = info.group[g]
                assert grp.in_order in (0, 1) and grp.kept_cols <= ol.DTYPE_SIZE[grp.sorted_as], what
                assert grp.kept_cols <= grp.key_bytes or g == 0, what      # (unused high bytes are constant columns)
            for t, s in zip(self.dev, self.saved):
                assert torch.equal(t, s), (what, "a column was written")
            infos[P] = info
        return infos


# ---- the sweep ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", list(range(10)))
def test_one_column_equals_oracle_rank(dt, monkeypatch):
    for order in (A, D):
        for n in (2, 3, 257, 4099, 65537) + ((300001,) if dt in (ol.U32, ol.F64, ol.U16) else ()):
            bits = ol.splitmix_fill(n, dt, 7100 + dt, 0xFFFFFFFFFFF000FF)
            want = ol.oracle_rank(bits, dt, 4, order)[0].astype(np.int64)
            infos = Case([bits], [dt], [order], want).run("one " + ol.DTYPE_NAMES[dt], monkeypatch, idx_bytes=4 if n & 1 else 8)
            for P in PACKS:
                assert infos[P].ngroups == 1 and infos[P].group[0].sorted_as == dt


@pytest.mark.parametrize("pattern", ["uniform", "ties", "one constant"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sweep(shape, pattern, monkeypatch):
    dtypes, orders, sizes = SHAPES[shape]
    if pattern == "one constant":
        sizes = [n for n in sizes if n in (3, 257, 1025, 65537)]
    for i, n in enumerate(sizes):
        case = Case(make_cols(dtypes, n, 7200 + 16 * i, pattern), dtypes, orders)
        case.run("%s %s" % (shape, pattern), monkeypatch, idx_bytes=8 if i % 3 == 2 else 4)


@pytest.mark.parametrize("shape", ["u32,u32", "9 x u8", "f64,f64 desc,i64"])
def test_both_index_widths(shape, monkeypatch):
    dtypes, orders, _ = SHAPES[shape]
    for n in (257, 4099, 65537):
        case = Case(make_cols(dtypes, n, 7300, "ties"), dtypes, orders)
        case.run(shape, monkeypatch, idx_bytes=4)
        case.run(shape, monkeypatch, idx_bytes=8)


# ---- early exits --------------------------------------------------------------------------------------------------------

def test_all_rows_equal(monkeypatch):
    for shape in ("u32,u32", "9 x u8", "i8,f32", "u64,u32"):
        dtypes, orders, _ = SHAPES[shape]
        for n in (2, 257, 65537):
            cols = [np.full(n, 0x42, dtype=ol.NP_BITS[dt]) for dt in dtypes]
            infos = Case(cols, dtypes, orders, want=np.arange(n, dtype=np.int64)).run("all equal " + shape, monkeypatch)
            for P, info in infos.items():
                assert info.early_exit == 2 and all(info.group[g].in_order for g in range(info.ngroups)), (shape, n, P)


def test_rows_already_in_order(monkeypatch):
    for shape in ("u32,u32", "u16,u16", "f32 desc,i32", "u8,u16,u8"):
        dtypes, orders, _ = SHAPES[shape]
        for n in (257, 4099, 65537):
            cols = make_cols(dtypes, n, 7400, "ties")
            perm = ll.want_perm(cols, dtypes, orders)
            cols = [c[perm] for c in cols]
            infos = Case(cols, dtypes, orders, want=np.arange(n, dtype=np.int64)).run("in order " + shape, monkeypatch)
            # one group holds the whole tuple at P = 8: its sort takes the pre-sorted exit (run() ties early_exit to in_order)
            assert infos[8].ngroups == 1 and infos[8].early_exit == 2, shape
    # every column non-descending by itself: every group of every packing is in order
    n = 65537
    i = np.arange(n)
    cols = [(i // 4096).astype(np.uint8), (i // 16).astype(np.uint16), (i // 4).astype(np.uint32)]
    infos = Case(cols, [ol.U8, ol.U16, ol.U32], [A, A, A], want=np.arange(n, dtype=np.int64)).run("monotone columns", monkeypatch)
    assert all(info.early_exit == 2 for info in infos.values())


# ---- keys ---------------------------------------------------------------------------------------------------------------

def test_float_specials(monkeypatch):
    f32 = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                    0x00000001, 0x80000001, 0x3F800000, 0xBF800000], dtype=np.uint32)
    f64 = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0xFFF8000000ABCDEF, 0x0, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x1, 0x8000000000000001, 0x3FF0000000000000], dtype=np.uint64)
    n = 13 * 11 * 3 + 2
    j = np.arange(n)
    a, b = f32[(j * 7) % 13], f64[(j * 5) % 11]
    tie = ol.splitmix_fill(n, ol.U8, 7501, 0x3)
    for orders in ([A, A, A], [D, A, D], [A, D, A]):
        Case([a, tie, b], [ol.F32, ol.U8, ol.F64], orders).run("specials f32,u8,f64", monkeypatch)
        Case([b, a], [ol.F64, ol.F32], orders[:2]).run("specials f64,f32", monkeypatch)
        Case([tie, a], [ol.U8, ol.F32], orders[:2]).run("specials u8,f32", monkeypatch)


def test_signed_extremes(monkeypatch):
    n = 1027
    lo = ol.splitmix_fill(n, ol.U8, 7601, 0x81)
    a = ol.splitmix_fill(n, ol.U32, 7602, 0x80000001)
    a[::5] = 0x7FFFFFFF
    b = ol.splitmix_fill(n, ol.U16, 7603, 0x8001)
    b[::7] = 0x7FFF
    Case([lo, a, b], [ol.I8, ol.I32, ol.I16], [A, D, A]).run("signed extremes", monkeypatch)


# ---- call variants ------------------------------------------------------------------------------------------------------

def test_a_column_given_twice(monkeypatch):
    for n in (257, 65537):
        a = ol.splitmix_fill(n, ol.U32, 7701, 0x80000003)
        b = ol.splitmix_fill(n, ol.U16, 7702, 0x3)
        da, db = ll.to_dev(a), ll.to_dev(b)
        # the same memory as u32 ascending, as i32 descending and as f32: three orders of one pointer
        Case([a, b, a, a], [ol.U32, ol.U16, ol.I32, ol.F32], [A, A, D, A], dev=[da, db, da, da]).run("column twice", monkeypatch)
        Case([b, b], [ol.U16, ol.I16], [A, D], dev=[db, db]).run("column twice", monkeypatch)


@pytest.mark.parametrize("shape", ["u32,u32", "u16,u16", "4 x u8", "u64,u32", "i8,f32"])
def test_offset_column_equals_aligned_copy(shape, monkeypatch):
    """Every column one element off a 16-byte boundary: the element loads of the pack form, and the inner rank sort on a
    caller's column that is only element-aligned."""
    dtypes, orders, _ = SHAPES[shape]
    for n in (3, 257, 1025, 65537):
        cols = make_cols(dtypes, n, 7800, "ties")
        aligned = Case(cols, dtypes, orders)
        aligned.run(shape + " aligned", monkeypatch)
        dev = []
        for c in cols:
            raw = torch.zeros(n + 16, dtype=ll.to_dev(c[:1]).dtype, device="cuda")
            assert raw.data_ptr() % 16 == 0
            raw[1:n + 1].copy_(ll.to_dev(c))
            dev.append(raw[1:n + 1])
        Case(cols, dtypes, orders, want=aligned.want, dev=dev).run(shape + " one element off", monkeypatch)


def test_non_default_stream_and_growth(monkeypatch):
    s = torch.cuda.Stream()
    dtypes, orders, _ = SHAPES["u32,u32"]
    for n in (4099, 300001, 65537):
        case = Case(make_cols(dtypes, n, 7900 + n, "ties"), dtypes, orders)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            case.run("stream", monkeypatch, stream=s)
            case.run("stream", monkeypatch, idx_bytes=8, stream=s)
    rsa.lib().rsx_release_stream(s.cuda_stream)


def test_capturing_stream_is_refused(monkeypatch):
    dtypes, orders, _ = SHAPES["u32,u32"]
    n = 4099
    case = Case(make_cols(dtypes, n, 8001, "ties"), dtypes, orders)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        case.run("before the capture", monkeypatch, packs=(4,), stream=s)   # (the context of this stream exists before the capture)
    s.synchronize()
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    arr = ll.lex_cols([t.data_ptr() for t in case.dev], dtypes, orders)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc, err, _ = ll.call_device_raw(arr, 2, n, out.data_ptr(), 4, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and "capturing" in err
    torch.cuda.synchronize()
    assert not out.any()
    rsa.lib().rsx_release_stream(s.cuda_stream)


def test_four_mi_rows_with_no_switch_set(monkeypatch):
    """4 Mi + 5 rows of (u32, u32), nothing forced: the inner sorts pick whatever route their thresholds give."""
    n = (4 << 20) + 5
    dtypes, orders, _ = SHAPES["u32,u32"]
    cols = [ol.splitmix_fill(n, ol.U32, 8101, 0xFFFFF), ol.splitmix_fill(n, ol.U32, 8102)]
    infos = Case(cols, dtypes, orders).run("4 Mi + 5", monkeypatch, packs=(None,))
    assert infos[None].ngroups == 2


def test_n_one_and_n_zero_on_the_device(monkeypatch):
    a = ll.to_dev(np.array([7], dtype=np.uint32))
    for ib in (4, 8):
        out = torch.full((2,), 0x5A, dtype=_IT[ib], device="cuda")
        arr = ll.lex_cols([a.data_ptr(), a.data_ptr()], [ol.U32, ol.F32])
        rc, err, info = ll.call_device_raw(arr, 2, 1, out.data_ptr(), ib)
        torch.cuda.synchronize()
        assert rc == 0 and (info.ngroups, info.early_exit) == (0, 1) and out.tolist() == [0, 0x5A]
        rc, err, info = ll.call_device_raw(arr, 2, 0, out.data_ptr(), ib)
        assert rc == 0 and info.early_exit == 1 and out.tolist() == [0, 0x5A]


# ---- the upper layers ---------------------------------------------------------------------------------------------------

def test_python_wrappers(monkeypatch):
    n = 65537
    dtypes, orders = [ol.F32, ol.U8, ol.I64], [D, A, D]
    cols = make_cols(dtypes, n, 8201, "ties")
    want = ll.want_perm(cols, dtypes, orders)
    dev = [ll.to_dev(c) for c in cols]
    for P in PACKS:
        pack(monkeypatch, P)
        idx, info = rsa.radix_sort_lex(dev, orders=orders, dtypes=dtypes)
        torch.cuda.synchronize()
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy().astype(np.int64), want)
        assert info.groups() == ll.want_groups(dtypes, P)
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        idx, info = rsa.radix_sort_lex(dev, orders=orders, dtypes=dtypes, idx_out=out)
        torch.cuda.synchronize()
        assert idx.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
        hidx, info = rsa.radix_sort_lex_host(cols, dtypes, orders)
        assert hidx.dtype == np.uint32 and np.array_equal(hidx.astype(np.int64), want)
        assert info.groups() == ll.want_groups(dtypes, P)
        hidx, info = rsa.radix_sort_lex_host([cols[1], cols[0], cols[1]], [ol.U8, ol.F32, ol.I8], None, idx_dtype=np.uint64)
        assert np.array_equal(hidx.astype(np.int64), ll.want_perm([cols[1], cols[0], cols[1]], [ol.U8, ol.F32, ol.I8]))
    # the tensors' own types, ascending: torch's int8 / int32 columns
    pack(monkeypatch, None)
    t8, t32 = dev[1].view(torch.int8), dev[0].view(torch.int32)
    idx, info = rsa.radix_sort_lex([t8, t32])
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ll.want_perm([cols[1], cols[0]], [ol.I8, ol.I32]))
    with pytest.raises(rsa.RsxError, match="same number"):
        rsa.radix_sort_lex([t8, t32[:-1]])
    for c, s in zip(dev, [ll.to_dev(c) for c in cols]):
        assert torch.equal(c, s)


def test_cpp_template():
    exe = os.path.join(ROOT, "tests", "cpp", "lex_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "cpp"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "lex_check: ok" in out.stdout, out.stdout + out.stderr
