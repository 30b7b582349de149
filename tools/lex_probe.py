"""radix_sort_lex at three packing limits against the composition it replaces (profiles/lex_probe.txt).

For every (shape, n) four things are timed in ONE process, alternating inside each round, each between two device events and
ending in a synchronise:
    P=1, P=4, P=8   rsx_sort_lex_device with RSX_LEX_PACK_BYTES = 1, 4, 8 (1: one sort per column)
    composed        what a caller had to write before this entry point existed: radix_sort_rank on the last column, then per
                    earlier column a torch gather through the permutation and radix_sort_pairs with the permutation as payload
Round 0 warms every shape up and CHECKS each result on the device against torch.sort(stable=True) chained over the derived
keys, last column first; rounds 1 .. R are timed, each on columns freshly generated from seeds of their own.  Printed: the
median and [min .. max] of the timed rounds in ms.  A row is marked "!" when the default packing limit is slower than a forced
one by more than the spread (max - min) that one shows in the same row, and "<" when it is slower than the composition by
more than the composition's spread.

    python tools/lex_probe.py [--log2 20,24,27] [--rounds 5] [--shapes u32,u32+4xu8] [--default 4] [--out profiles/lex_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

A, D = rsa.ASCENDING, rsa.DESCENDING
FULL = 0xFFFFFFFFFFFFFFFF
# name -> [(rsx dtype, torch dtype, order, mask)], column 0 first (the most significant)
SHAPES = {
    "u32,u32": [(rsa.U32, torch.int32, A, FULL)] * 2,
    "u32,u32<2^20": [(rsa.U32, torch.int32, A, 0xFFFFF)] * 2,
    "u16,u16": [(rsa.U16, torch.int16, A, FULL)] * 2,
    "4xu8": [(rsa.U8, torch.int8, A, FULL)] * 4,
    "f32d,i32": [(rsa.F32, torch.int32, D, FULL), (rsa.I32, torch.int32, A, FULL)],
    "u64,u32": [(rsa.U64, torch.int64, A, FULL), (rsa.U32, torch.int32, A, FULL)],
}
PACKS = (1, 4, 8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(value):
    if value is None:
        os.environ.pop("RSX_LEX_PACK_BYTES", None)
    else:
        os.environ["RSX_LEX_PACK_BYTES"] = str(value)
    rsa.reload_env()


def derived_keys(t, code, order):
    """the column's derived keys as int64 values whose signed order is the library's order"""
    bits = 8 * rsa.DTYPE_SIZE[code]
    if bits == 64:
        u = t
        if code == rsa.U64:
            k = u ^ torch.iinfo(torch.int64).min
        elif code == rsa.I64:
            k = u
        else:
            k = torch.where(u < 0, ~u ^ torch.iinfo(torch.int64).min, u)
    else:
        u = t.to(torch.int64) & ((1 << bits) - 1)
        top = 1 << (bits - 1)
        if code in (rsa.I8, rsa.I16, rsa.I32):
            k = u ^ top
        elif code == rsa.F32:
            k = torch.where((u >> 31) != 0, u ^ 0xFFFFFFFF, u ^ top)
        else:
            k = u
    return ~k if order == D else k


def reference_perm(cols, shape):
    n = cols[0].numel()
    perm = torch.arange(n, dtype=torch.int64, device="cuda")
    for t, (code, _, order, _) in reversed(list(zip(cols, shape))):
        perm = perm[torch.sort(derived_keys(t[perm], code, order), stable=True)[1]]
    return perm


class Composed:
    """The parent commit's way: its own index buffer, gathered keys and ping-pong partners, as a caller has to keep them."""

    def __init__(self, shape, n):
        self.ib = torch.empty(2 * n, dtype=torch.int32, device="cuda")
        self.aux = [torch.empty(n, dtype=tdt, device="cuda") for _, tdt, _, _ in shape]
        self.keys = [torch.empty(n, dtype=tdt, device="cuda") for _, tdt, _, _ in shape]

    def __call__(self, cols, shape):
        code, _, order, _ = shape[-1]
        perm, _ = rsa.radix_sort_rank(cols[-1], self.ib, dtype=code, order=order)
        n = cols[0].numel()
        other = self.ib[n:] if perm.data_ptr() == self.ib.data_ptr() else self.ib[:n]
        for j in range(len(cols) - 2, -1, -1):
            code, _, order, _ = shape[j]
            keys = torch.index_select(cols[j], 0, perm, out=self.keys[j])
            _, perm2, _ = rsa.radix_sort_pairs(keys, self.aux[j], perm, other, dtype=code, order=order)
            if perm2.data_ptr() != perm.data_ptr():
                perm, other = perm2, perm
        return perm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="20,24,27")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="+".join(SHAPES), help="shape names joined by '+'")
    ap.add_argument("--default", type=int, default=4, help="the packing limit the library ships with (marks are against it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rsa.require_gpu()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/lex_probe.py: %d timed rounds after one checked warm-up round; ms, median [min .. max]; default P = %d" % (
        args.rounds, args.default))
    emit("#  %-13s %5s %-9s | %-25s | %-25s | %-25s | %-25s" % ("shape", "log2n", "sorts", "P=1", "P=4", "P=8", "composed (parent)"))
    for name in args.shapes.split("+"):
        shape = SHAPES[name]
        for lg in [int(x) for x in args.log2.split(",")]:
            n = 1 << lg
            cols = [torch.empty(n, dtype=tdt, device="cuda") for _, tdt, _, _ in shape]
            idx = torch.empty(n, dtype=torch.int32, device="cuda")
            composed = Composed(shape, n)
            codes, orders = [s[0] for s in shape], [s[2] for s in shape]
            t = {m: [] for m in PACKS + ("composed",)}
            ngroups = {}
            for r in range(args.rounds + 1):
                for j, (t_, s) in enumerate(zip(cols, shape)):
                    rsa.fill_splitmix(t_, 9100 + 131 * r + 17 * j, s[3])
                want = reference_perm(cols, shape).to(torch.int32) if r == 0 else None
                for P in PACKS:
                    setenv(P)
                    ms, (_, info) = timed(lambda: rsa.radix_sort_lex(cols, orders=orders, dtypes=codes, idx_out=idx))
                    t[P].append(ms)
                    ngroups[P] = info.ngroups
                    if r == 0:
                        assert torch.equal(idx, want), (name, lg, P)
                ms, perm = timed(lambda: composed(cols, shape))
                t["composed"].append(ms)
                if r == 0:
                    assert torch.equal(perm, want), (name, lg, "composed")
                    del want

            def fmt(v):
                v = v[1:]
                return "%8.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))
            med = {m: statistics.median(v[1:]) for m, v in t.items()}
            spread = {m: max(v[1:]) - min(v[1:]) for m, v in t.items()}
            flag = "!" if any(med[args.default] > med[P] + spread[P] for P in PACKS if P != args.default) else " "
            flag += "<" if med[args.default] > med["composed"] + spread["composed"] else " "
            emit("%s %-13s %5d %-9s | %s | %s | %s | %s" % (flag, name, lg, "/".join(str(ngroups[P]) for P in PACKS), fmt(t[1]), fmt(t[4]),
                                                         fmt(t[8]), fmt(t["composed"])))
            del cols, idx, composed
            torch.cuda.empty_cache()
    setenv(None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
