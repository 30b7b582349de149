"""radix_sort_reduce against its own sort route, against the sort alone and against what a caller had to do before it (DESIGN.md 4o;
profiles/reduce/reduce_probe.txt).

For every input row and each of three value columns -- u32 values with sums, f32 values with sums, minima and maxima, f64 values
with sums -- five things are timed in ONE process, alternating, after a warm-up round, each between two device events and ending
in a synchronise (`default` goes first in a round: behind the yardstick of the round before it reads slow):
    default   radix_sort_reduce as it chooses its route
    forced    the same with RSX_REDUCE_FORCE=2 (the sort route: a key + value sort of copies and the pass over the runs)
    cells24   the same with RSX_REDUCE_MAX_BITS=24: the cells in device memory wherever the library was compiled for them (what
              the default cut-off is decided from; the same as `default` where that takes the cells anyway)
    pairs     a copy of keys and values and radix_sort_pairs of the copies, alone: what the sort route cannot be faster than
    before    the way to the sums without the call: torch.unique(return_inverse=True) + index_add_, or, for 1-byte keys,
              torch.bincount(weights=) -- sums only, whatever the column asks for; one round after the warm-up (it takes seconds
              where few groups meet torch's float atomics, and is left out for float values with half the elements on one key:
              at the rate of the 256-group rows, 14 us per add and address, that cell alone would take minutes)
The sources are never written, so nothing is refilled between the calls.  The spread of a column is the run-to-run spread the
acceptance rule of DESIGN.md 4h / 4l / 4o refers to.  For rows on the LDS cells the last columns give the bytes per second of keys
and values read once, and that as a fraction of rsx_sort_locate's one-value row (3.1 TB/s, profiles/locate/locate_probe.txt).

A run may be cut into pieces, each a process of its own under a time limit of its own, that append to one file:
`--rows 0,1,2` takes the rows of that number only (the header is written by the piece that does not append).

    python tools/reduce_probe.py [--log2 26] [--rounds 3] [--rows 0,1] [--out profiles/reduce/reduce_probe.txt] [--append [--header]]
                                 [--no-before]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

ROUTES = ["TRIVIAL", "CELLS_LDS", "CELLS_GLOBAL", "SORT"]
LOCATE_ONE_VALUE_GBS = 3100.0


def rows():
    """(name, dtype code, carrier, mask, key bytes, kind)"""
    return [("u8 keys", rsa.U8, torch.int8, 0xFF, 1, "fill"),
            ("u32 V=8", rsa.U32, torch.int32, 0x0000FF00, 4, "fill"),
            ("u32 V=12", rsa.U32, torch.int32, 0x00F0F00F, 4, "fill"),
            ("u32 V=14", rsa.U32, torch.int32, 0x00F0FF03, 4, "fill"),
            ("u32 V=16", rsa.U32, torch.int32, 0x00F0FF0F, 4, "fill"),
            ("u32 V=20", rsa.U32, torch.int32, 0x0FF0FF0F, 4, "fill"),
            ("u32 uniform", rsa.U32, torch.int32, 0xFFFFFFFF, 4, "fill"),
            ("u64 < 2^40", rsa.U64, torch.int64, (1 << 40) - 1, 8, "fill"),
            ("u32 sorted, dups", rsa.U32, torch.int32, 0x00FFFFFF, 4, "sorted"),
            ("u32 V=12 half/1", rsa.U32, torch.int32, 0x00F0F00F, 4, "half"),
            ("u32 V=16 half/1", rsa.U32, torch.int32, 0x00F0FF0F, 4, "half")]


def columns():
    """(name, value dtype code, torch dtype, value bytes, sum, min, max)"""
    return [("u32 sum", rsa.U32, torch.int32, 4, True, False, False),
            ("f32 sum+min+max", rsa.F32, torch.float32, 4, True, True, True),
            ("f64 sum", rsa.F64, torch.float64, 8, True, False, False)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(**values):
    for name in ("RSX_REDUCE_FORCE", "RSX_REDUCE_MAX_BITS"):
        v = values.get(name)
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    rsa.reload_env()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-before", action="store_true")
    ap.add_argument("--header", action="store_true", help="write the header lines although appending")
    ap.add_argument("--rows", default=None, help="comma-separated row numbers (default: all)")
    args = ap.parse_args()
    rsa.require_gpu()
    n = 1 << args.log2
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        v = v[1:]
        if not v:
            return "%24s" % "-"
        if len(v) == 1:
            return "%7.3f %16s" % (v[0], "(one round)")
        return "%7.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))

    picked = None if args.rows is None else {int(x) for x in args.rows.split(",")}
    if not args.append or args.header:
        emit("# tools/reduce_probe.py: n = 2^%d elements, 4-byte counts, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.rounds))
        emit("# %-17s %-16s %-12s | %-24s | %-24s | %-12s %-24s | %-24s | %-24s | GB/s of keys + values read once, of locate's 3.1 TB/s" % (
            "input", "values", "route", "default", "RSX_REDUCE_FORCE=2", "route", "RSX_REDUCE_MAX_BITS=24", "copy + radix_sort_pairs", "before this call"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242)
    for number, (name, dt, tdt, mask, kb, kind) in enumerate(rows()):
        if picked is not None and number not in picked:
            continue
        src = torch.empty(n, dtype=tdt, device="cuda")
        rsa.fill_splitmix(src, 4242, mask)
        if kind == "sorted":
            src = torch.sort(src).values.contiguous()
        elif kind == "half":
            src[::2] = src[0]
        torch.cuda.synchronize()
        k0, k1 = torch.empty_like(src), torch.empty_like(src)
        okeys = torch.empty_like(src)
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        for cname, vdt, vtdt, vb, want_sum, want_min, want_max in columns():
            if vtdt.is_floating_point:
                vals = torch.randn(n, dtype=vtdt, device="cuda", generator=gen)
            else:
                vals = torch.empty(n, dtype=vtdt, device="cuda")
                rsa.fill_splitmix(vals, 4343)
            v0, v1 = torch.empty_like(vals), torch.empty_like(vals)
            sm = torch.empty(n, dtype=torch.float64 if vtdt.is_floating_point else torch.int64, device="cuda")
            mn = torch.empty_like(vals) if want_min else False
            mx = torch.empty_like(vals) if want_max else False

            def call():
                return rsa.radix_sort_reduce(src, vals, dtype=dt, val_dtype=vdt, sum=sm, min=mn, max=mx, counts=counts, keys_out=okeys)

            def pairs():
                k0.copy_(src)
                v0.copy_(vals)
                return rsa.radix_sort_pairs(k0, k1, v0, v1, dtype=dt)[2]

            def before():
                if kb == 1:
                    return torch.bincount(src.to(torch.int64) + 128, weights=vals.to(torch.float64))
                u, inv = torch.unique(src, return_inverse=True)
                acc = torch.zeros(u.numel(), dtype=sm.dtype, device="cuda")
                return acc.index_add_(0, inv, vals.to(sm.dtype))

            t = {"default": [], "forced": [], "cells24": [], "pairs": [], "before": []}
            started = time.time()
            route = route24 = None
            for r in range(args.rounds + 1):
                setenv()
                ms, out = timed(call)
                route = out[5].route
                t["default"].append(ms)
                setenv(RSX_REDUCE_FORCE=2)
                ms, out = timed(call)
                assert out[5].route in (rsa.REDUCE_SORT, rsa.REDUCE_TRIVIAL)
                t["forced"].append(ms)
                setenv(RSX_REDUCE_MAX_BITS=24)
                ms, out = timed(call)
                route24 = out[5].route
                t["cells24"].append(ms)
                setenv()
                ms, _ = timed(pairs)
                t["pairs"].append(ms)
                if not args.no_before and r < 2 and not (kind == "half" and vtdt.is_floating_point):
                    ms, res = timed(before)
                    del res
                    t["before"].append(ms)
            med = statistics.median(t["default"][1:])
            tail = ""
            if route == rsa.REDUCE_CELLS_LDS:
                gbs = n * (kb + vb) / med / 1e6
                tail = "%6.0f  %4.2f" % (gbs, gbs / LOCATE_ONE_VALUE_GBS)
            emit("  %-17s %-16s %-12s | %s | %s | %-12s %s | %s | %s | %s" % (name, cname, ROUTES[route], fmt(t["default"]), fmt(t["forced"]), ROUTES[route24],
                                                                          fmt(t["cells24"]), fmt(t["pairs"]), fmt(t["before"]), tail))
            print("    (%.1f s of wall time)" % (time.time() - started), flush=True)
            del vals, v0, v1, sm, mn, mx
            torch.cuda.empty_cache()
        del src, k0, k1, okeys, counts
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
