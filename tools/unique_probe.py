"""radix_sort_unique against the sort it replaces, 2^28 keys (profiles/unique/unique_probe.txt).

For every input row four things are timed in ONE process, alternating, after a warm-up round, each between two device events
and ending in a synchronise:
    default   radix_sort_unique as it chooses its route
    forced    the same with RSX_UNIQUE_MAX_BITS=0 (the sort route: the ordinary sort and one compaction)
    sort      the plain radix_sort (rsx_sort_device) of the same keys
    copy      a device-to-device copy of the n keys
The source is refilled from a pristine copy before every timed call (not timed).

    python tools/unique_probe.py [--log2 28] [--rounds 5] [--out profiles/unique/unique_probe.txt]
    python tools/unique_probe.py --plain-only      # one line: the plain sort of uniform u32 (for tools/ab_lib.py with RSX_LIB)
    python tools/unique_probe.py --sweep           # the V = 16 .. 28 rows at RSX_UNIQUE_MAX_BITS = 30 as well (the cut-off)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402


def mask_of(v):
    return (1 << v) - 1


def rows(n):
    out = [("u16 full range", rsa.U16, torch.int16, 0xFFFF, False)]
    for v in (16, 18, 20, 22, 24, 26, 28):
        out.append(("u32 V=%d" % v, rsa.U32, torch.int32, mask_of(v), False))
    out.append(("u32 uniform", rsa.U32, torch.int32, 0xFFFFFFFF, False))
    out.append(("u64 < 2^40", rsa.U64, torch.int64, mask_of(40), False))
    out.append(("u32 sorted, V=20", rsa.U32, torch.int32, mask_of(20), True))
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(max_bits):
    if max_bits is None:
        os.environ.pop("RSX_UNIQUE_MAX_BITS", None)
    else:
        os.environ["RSX_UNIQUE_MAX_BITS"] = str(max_bits)
    rsa.reload_env()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    rsa.require_gpu()
    n = 1 << args.log2
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.plain_only:
        orig = torch.empty(n, dtype=torch.int32, device="cuda")
        rsa.fill_splitmix(orig, 4242)
        src, aux = torch.empty_like(orig), torch.empty_like(orig)
        ts = []
        for r in range(args.rounds + 1):
            src.copy_(orig)
            t, _ = timed(lambda: rsa.radix_sort(src, aux, dtype=rsa.U32))
            if r:
                ts.append(t)
        print("plain sort u32 uniform 2^%d: median %.3f ms  min %.3f  max %.3f  (%d rounds)"
              % (args.log2, statistics.median(ts), min(ts), max(ts), len(ts)))
        return
    has_unique = hasattr(rsa, "radix_sort_unique")
    emit("# tools/unique_probe.py: n = 2^%d keys, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.rounds))
    emit("# %-18s %-14s %8s | %-24s | %-24s | %-24s | %-20s" % ("input", "route", "n_unique", "default", "RSX_UNIQUE_MAX_BITS=0", "plain sort", "d2d copy"))
    for name, dt, tdt, mask, presort in rows(n):
        orig = torch.empty(n, dtype=tdt, device="cuda")
        rsa.fill_splitmix(orig, 4242, mask)
        if presort:
            orig = torch.sort(orig)[0].contiguous()
        src, aux = torch.empty_like(orig), torch.empty_like(orig)
        t = {"default": [], "forced": [], "sort": [], "copy": [], "wide": []}
        route = nu = None
        for r in range(args.rounds + 1):
            setenv(None)
            src.copy_(orig)
            ms, (out, _, info) = timed(lambda: rsa.radix_sort_unique(src, aux, dtype=dt))
            route, nu = info.route, out.numel()
            t["default"].append(ms)
            setenv(0)
            src.copy_(orig)
            ms, (out0, _, info0) = timed(lambda: rsa.radix_sort_unique(src, aux, dtype=dt))
            assert out0.numel() == nu and (info0.route == rsa.UNIQUE_SORT or nu == 1)
            t["forced"].append(ms)
            if args.sweep:
                setenv(30)
                src.copy_(orig)
                ms, (out1, _, info1) = timed(lambda: rsa.radix_sort_unique(src, aux, dtype=dt))
                assert out1.numel() == nu
                t["wide"].append((ms, info1.route))
            setenv(None)
            src.copy_(orig)
            ms, _ = timed(lambda: rsa.radix_sort(src, aux, dtype=dt))
            t["sort"].append(ms)
            ms, _ = timed(lambda: aux.copy_(orig))
            t["copy"].append(ms)

        def fmt(v):
            v = v[1:]
            return "%7.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))
        routes = ["TRIVIAL", "BITMAP_LDS", "BITMAP_GLOBAL", "TABLE", "SORT"]
        line = "  %-18s %-14s %8d | %s | %s | %s | %s" % (name, routes[route], nu, fmt(t["default"]), fmt(t["forced"]), fmt(t["sort"]),
                                                          fmt(t["copy"]))
        if args.sweep:
            line += " | MAX_BITS=30: %s %s" % (fmt([m for m, _ in t["wide"]]), routes[t["wide"][-1][1]])
        emit(line)
        if name == "u32 uniform":
            extra = statistics.median(t["forced"][1:]) - statistics.median(t["sort"][1:])
            cp = statistics.median(t["copy"][1:])
            emit("#   sort route's extra over the plain sort: %.3f ms = %.2f x the copy (bound: 2 x)" % (extra, extra / cp))
        del orig, src, aux
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert has_unique


if __name__ == "__main__":
    main()
