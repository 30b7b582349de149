"""radix_sort_locate against its own sort route and against what a caller had to do before it (DESIGN.md 4n;
profiles/locate/locate_probe.txt).

For every input row, every list of values and each of the two questions -- less + equal, less + equal + bins -- three things are
timed in ONE process, alternating, after a warm-up round, each between two device events and ending in a synchronise:
    default   radix_sort_locate as it chooses its route
    forced    the same with RSX_LOCATE_FORCE=2 (the sort route: a sort of a copy of the keys and binary searches)
    before    the way to the same arrays without the call: radix_sort of a copy of the keys, torch.searchsorted left and right
              over it; for the bins torch.sort of the values and torch.bucketize
The keys are signed where their width has a signed torch type, so that torch orders them as the library does.  The source is never
written, so nothing is refilled between the calls.  The spread of a column is the run-to-run spread the acceptance rule of
DESIGN.md 4h / 4l / 4m / 4n refers to.  Last, the contention case: one value, all keys equal, one set of LDS counters against the
default.

    python tools/locate_probe.py [--log2 26] [--rounds 5] [--out profiles/locate/locate_probe.txt] [--append]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

ROUTES = ["TRIVIAL", "TABLE", "SEARCH", "SORT"]


def rows():
    return [("i32 uniform", rsa.I32, torch.int32, 0xFFFFFFFF, 4),
            ("u64 < 2^40", rsa.U64, torch.int64, (1 << 40) - 1, 8),
            ("i16 full range", rsa.I16, torch.int16, 0xFFFF, 2)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(**values):
    for name in ("RSX_LOCATE_FORCE", "RSX_LOCATE_COUNTER_SETS"):
        v = values.get(name)
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    rsa.reload_env()


def value_lists(src, dt, tdt, kb, n):
    """(name, values): 1, 255 and 4096 quantile splitters of the keys; 4096 values inside one digit of the start table"""
    out = []
    for m in (1, 255, 4096):
        keys, _, _, _, _ = rsa.radix_sort_nth(src, [(i + 1) * n // (m + 1) for i in range(m)], dtype=dt, want_idx=False)
        out.append(("%d splitters" % m, keys.clone()))
    if kb >= 4:
        v = torch.arange(4095, dtype=torch.int64, device="cuda") * 3 + 1000
        far = torch.tensor([(1 << 39) if kb == 8 else (1 << 30)], dtype=torch.int64, device="cuda")
        out.append(("4096 in one digit", torch.cat([v, far]).to(tdt)))
    return out


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

    emit("# tools/locate_probe.py: n = 2^%d keys, 4-byte indices, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.rounds))
    emit("# %-15s %-18s %-14s %-7s | %-24s | %-24s | %-24s | GB/s of the keys read once" % ("input", "values", "asked", "route", "default", "RSX_LOCATE_FORCE=2", "before this call"))
    for name, dt, tdt, mask, kb in rows():
        src = torch.empty(n, dtype=tdt, device="cuda")
        rsa.fill_splitmix(src, 4242, mask)
        k0, k1 = torch.empty_like(src), torch.empty_like(src)
        bins = torch.empty(n, dtype=torch.int32, device="cuda")
        for vname, vals in value_lists(src, dt, tdt, kb, n):
            m = vals.numel()
            less, equal = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")

            def sorted_before():
                k0.copy_(src)
                res, _ = rsa.radix_sort(k0, k1, dtype=dt)
                lo = torch.searchsorted(res, vals, out_int32=True)
                hi = torch.searchsorted(res, vals, right=True, out_int32=True)
                return lo, hi - lo

            def bins_before():
                r = sorted_before()
                edges = torch.sort(vals).values
                return r, torch.bucketize(src, edges, out_int32=True, right=True)

            for asked, want_bins, before in (("less+equal", False, sorted_before), ("less+equal+bins", bins, bins_before)):
                t = {"default": [], "forced": [], "before": []}
                route = None
                for r in range(args.rounds + 1):
                    setenv()
                    ms, out = timed(lambda: rsa.radix_sort_locate(src, vals, dtype=dt, less=less, equal=equal, bins=want_bins))
                    route = out[0].route
                    t["default"].append(ms)
                    setenv(RSX_LOCATE_FORCE=2)
                    ms, out = timed(lambda: rsa.radix_sort_locate(src, vals, dtype=dt, less=less, equal=equal, bins=want_bins))
                    assert out[0].route == rsa.LOCATE_SORT
                    t["forced"].append(ms)
                    setenv()
                    ms, res = timed(before)
                    del res
                    t["before"].append(ms)
                emit("  %-15s %-18s %-14s %-7s | %s | %s | %s | %6.0f" % (name, vname, asked, ROUTES[route], fmt(t["default"]), fmt(t["forced"]), fmt(t["before"]),
                                                                         n * kb / statistics.median(t["default"][1:]) / 1e6))
            del less, equal
        del src, k0, k1, bins
        torch.cuda.empty_cache()
    # the contention case: every key lands on the same counter
    src = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    vals = src[:1].clone()
    less, equal = torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    t = {1: [], None: []}
    sets = {}
    for r in range(args.rounds + 1):
        for k in (1, None):
            setenv(RSX_LOCATE_COUNTER_SETS=k)
            ms, out = timed(lambda: rsa.radix_sort_locate(src, vals, dtype=rsa.I32, less=less, equal=equal))
            sets[k] = out[0].counter_sets
            t[k].append(ms)
    setenv()
    emit("# all keys equal, one value, less + equal: %d set of counters %s; the default, %d sets, %s" % (sets[1], fmt(t[1]), sets[None], fmt(t[None])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
