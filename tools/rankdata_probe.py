"""radix_sort_rankdata against its own sort route and against what a caller had to do before it (DESIGN.md 4m;
profiles/rankdata/rankdata_probe.txt).

For every input row and for each of the two questions -- the place alone, less + equal -- three things are timed in ONE process,
alternating, after a warm-up round, each between two device events and ending in a synchronise:
    default   radix_sort_rankdata as it chooses its route
    forced    the same with RSX_RANKDATA_NO_TABLES=1 (the sort route: a key + index sort of a copy, then the inverse scatter or the
              heads and the runs pass)
    before    the way to the same array without the call -- the place: radix_sort_rank and a torch scatter of an arange through
              its result; less + equal: radix_sort_group with counts, a torch cumsum and two gathers
and once per row
    pairs     rsx_sort_pairs_device alone on a copy of the keys and an iota payload (the copy and the iota are not timed)
The source is never written, so nothing is refilled between the calls.  The spread of a column is the run-to-run spread the
acceptance rule of DESIGN.md 4h / 4l / 4m refers to.

    python tools/rankdata_probe.py [--log2 26] [--rounds 5] [--out profiles/rankdata/rankdata_probe.txt] [--append]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

ROUTES = ["TRIVIAL", "TABLE", "COUNT16", "SORT"]


def rows():
    return [("u8 full range", rsa.U8, torch.int8, 0xFF),
            ("u32 one byte", rsa.U32, torch.int32, 0x00FF0000),
            ("u32 V=12", rsa.U32, torch.int32, 0x00F0FF00),
            ("u32 V=16", rsa.U32, torch.int32, 0x00F0FF0F),
            ("u16 full range", rsa.U16, torch.int16, 0xFFFF),
            ("u32 uniform", rsa.U32, torch.int32, 0xFFFFFFFF),
            ("u64 < 2^40", rsa.U64, torch.int64, (1 << 40) - 1)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(no_tables):
    if no_tables:
        os.environ["RSX_RANKDATA_NO_TABLES"] = "1"
    else:
        os.environ.pop("RSX_RANKDATA_NO_TABLES", None)
    rsa.reload_env()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    rsa.require_gpu()
    n = 1 << args.log2
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        v = v[1:]
        return "%7.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))

    emit("# tools/rankdata_probe.py: n = 2^%d keys, 4-byte indices, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.rounds))
    emit("# %-15s %-11s %-8s | %-24s | %-24s | %-24s" % ("input", "asked", "route", "default", "RSX_RANKDATA_NO_TABLES=1", "before this call"))
    for name, dt, tdt, mask in rows():
        src = torch.empty(n, dtype=tdt, device="cuda")
        rsa.fill_splitmix(src, 4242, mask)
        o0, o1 = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        ib = torch.empty(2 * n, dtype=torch.int32, device="cuda")
        k0, k1 = torch.empty_like(src), torch.empty_like(src)
        iota = torch.arange(n, dtype=torch.int32, device="cuda")

        def place_before():
            ranks, _ = rsa.radix_sort_rank(src, ib, dtype=dt)
            o0.scatter_(0, ranks.to(torch.int64), iota)       # (torch's scatter takes 8-byte indices)
            return o0

        def counts_before():
            inv, _, counts, _, _ = rsa.radix_sort_group(src, dtype=dt, inverse=o0, counts=o1)
            starts = torch.cumsum(counts, 0, dtype=torch.int64) - counts
            j = inv.to(torch.int64)
            return starts[j], counts[j]

        t = {k: [] for k in ("p_default", "p_forced", "p_before", "c_default", "c_forced", "c_before", "pairs")}
        p_route = c_route = None
        for r in range(args.rounds + 1):
            setenv(False)
            ms, out = timed(lambda: rsa.radix_sort_rankdata(src, dtype=dt, place=o0))
            p_route = out[3].route
            t["p_default"].append(ms)
            ms, out = timed(lambda: rsa.radix_sort_rankdata(src, dtype=dt, place=False, less=o0, equal=o1))
            c_route = out[3].route
            t["c_default"].append(ms)
            setenv(True)
            ms, out = timed(lambda: rsa.radix_sort_rankdata(src, dtype=dt, place=o0))
            assert out[3].route == rsa.RANKDATA_SORT
            t["p_forced"].append(ms)
            ms, out = timed(lambda: rsa.radix_sort_rankdata(src, dtype=dt, place=False, less=o0, equal=o1))
            assert out[3].route == rsa.RANKDATA_SORT
            t["c_forced"].append(ms)
            setenv(False)
            ms, _ = timed(place_before)
            t["p_before"].append(ms)
            ms, res = timed(counts_before)
            del res
            t["c_before"].append(ms)
            k0.copy_(src)
            ib[:n].copy_(iota)
            ms, _ = timed(lambda: rsa.radix_sort_pairs(k0, k1, ib[:n], ib[n:], dtype=dt))
            t["pairs"].append(ms)
        emit("  %-15s %-11s %-8s | %s | %s | %s" % (name, "place", ROUTES[p_route], fmt(t["p_default"]), fmt(t["p_forced"]), fmt(t["p_before"])))
        emit("  %-15s %-11s %-8s | %s | %s | %s" % (name, "less+equal", ROUTES[c_route], fmt(t["c_default"]), fmt(t["c_forced"]), fmt(t["c_before"])))
        pairs = statistics.median(t["pairs"][1:])
        emit("#   pairs sort alone %s; the sort route's extra over it: place (copy, iota, inverse scatter) %.3f ms, less + equal (copy, "
             "iota, heads, positions, runs pass) %.3f ms" % (fmt(t["pairs"]), statistics.median(t["p_forced"][1:]) - pairs,
                                                             statistics.median(t["c_forced"][1:]) - pairs))
        del src, o0, o1, ib, k0, k1, iota
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
