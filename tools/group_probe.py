"""radix_sort_group against the sort route it replaces, 2^28 keys (profiles/group/group_probe.txt).

For every input row four things are timed in ONE process, alternating, after a warm-up round, each between two device events
and ending in a synchronise:
    default   radix_sort_group (the inverse alone) as it chooses its route
    forced    the same with RSX_GROUP_MAX_BITS=0 (the sort route: a key + index sort of a copy and the heads pass)
    pairs     rsx_sort_pairs_device alone on a copy of the keys and an iota payload (the copy and the iota are not timed)
    torch     torch.unique(sorted=True, return_inverse=True) on the same tensor, as an outside yardstick
The source is never written, so nothing is refilled between the group calls.

    python tools/group_probe.py [--log2 28] [--rounds 5] [--out profiles/group/group_probe.txt]
    python tools/group_probe.py --sweep           # every V from 16 to 30 at RSX_GROUP_MAX_BITS = 30 as well (the cut-off)
    python tools/group_probe.py --no-torch        # without the yardstick (torch.unique needs several n-sized buffers)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

ROUTES = ["TRIVIAL", "RANK_LDS", "RANK_GLOBAL", "TABLE", "SORT"]


def mask_of(v):
    return (1 << v) - 1


def rows(sweep):
    out = [("u16 full range", rsa.U16, torch.int16, 0xFFFF, False)]
    for v in (range(16, 31) if sweep else (16, 18, 20, 24, 28)):
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
        os.environ.pop("RSX_GROUP_MAX_BITS", None)
    else:
        os.environ["RSX_GROUP_MAX_BITS"] = str(max_bits)
    rsa.reload_env()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    rsa.require_gpu()
    n = 1 << args.log2
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/group_probe.py: n = 2^%d keys, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.rounds))
    emit("# %-18s %-12s %10s | %-24s | %-24s | %-24s | %-24s" % ("input", "route", "n_groups", "default", "RSX_GROUP_MAX_BITS=0",
                                                                   "pairs sort alone", "torch.unique + inverse"))
    for name, dt, tdt, mask, presort in rows(args.sweep):
        src = torch.empty(n, dtype=tdt, device="cuda")
        rsa.fill_splitmix(src, 4242, mask)
        if presort:
            src = torch.sort(src)[0].contiguous()
        inv = torch.empty(n, dtype=torch.int32, device="cuda")
        k0, k1 = torch.empty_like(src), torch.empty_like(src)
        v0, v1 = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        iota = torch.arange(n, dtype=torch.int32, device="cuda")
        t = {"default": [], "forced": [], "pairs": [], "torch": [], "wide": []}
        route = ng = None
        for r in range(args.rounds + 1):
            setenv(None)
            ms, out = timed(lambda: rsa.radix_sort_group(src, dtype=dt, inverse=inv, keys=k1))
            route, ng = out[4].route, out[1].numel()
            t["default"].append(ms)
            setenv(0)
            ms, out0 = timed(lambda: rsa.radix_sort_group(src, dtype=dt, inverse=inv, keys=k1))
            assert out0[1].numel() == ng and (out0[4].route == rsa.GROUP_SORT or ng == 1)
            t["forced"].append(ms)
            if args.sweep:
                setenv(30)
                ms, out1 = timed(lambda: rsa.radix_sort_group(src, dtype=dt, inverse=inv, keys=k1))
                assert out1[1].numel() == ng
                t["wide"].append((ms, out1[4].route))
            setenv(None)
            k0.copy_(src)
            v0.copy_(iota)
            ms, _ = timed(lambda: rsa.radix_sort_pairs(k0, k1, v0, v1, dtype=dt))
            t["pairs"].append(ms)
            if not args.no_torch:
                ms, tu = timed(lambda: torch.unique(src, sorted=True, return_inverse=True))
                assert tu[0].numel() == ng
                del tu
                t["torch"].append(ms)

        def fmt(v):
            v = v[1:]
            return "%7.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v)) if v else "%24s" % "-"
        line = "  %-18s %-12s %10d | %s | %s | %s | %s" % (name, ROUTES[route], ng, fmt(t["default"]), fmt(t["forced"]), fmt(t["pairs"]),
                                                          fmt(t["torch"]))
        if args.sweep:
            line += " | MAX_BITS=30: %s %s" % (fmt([m for m, _ in t["wide"]]), ROUTES[t["wide"][-1][1]])
        emit(line)
        extra = statistics.median(t["forced"][1:]) - statistics.median(t["pairs"][1:])
        emit("#   sort route's extra over the pairs sort alone (copy, iota, heads pass and scatter): %.3f ms" % extra)
        del src, inv, k0, k1, v0, v1, iota
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
