"""radix_sort_topk against the rank sort it replaces (profiles/topk_probe.txt).

For every (dtype, key set, n, k) five things are timed in ONE process, alternating inside each round, each between two device
events and ending in a synchronise:
    select    rsx_sort_topk_device with RSX_TOPK_FORCE=1 (MSD radix select, then a sort of k pairs)
    sort      the same with RSX_TOPK_FORCE=2 (the rank sort, first k kept)
    default   the same with the switch unset (the library's own choice; its route is printed)
    rank      rsx_sort_rank_device and a slice: the only way before this entry point existed
    torch     torch.topk(largest=False) on the same bits, for information only (its order among ties is not the library's)
Round 0 warms every shape up and CHECKS each of the three top-k results on the device against torch.sort(stable=True) of the
derived keys; rounds 1 .. R are timed, each on keys freshly generated from a seed of its own.  Printed: the median and
[min .. max] of the timed rounds in ms.  A row is marked "!" when the default is slower than the better forced route by more
than the spread (max - min) that route shows in the same row.

    python tools/topk_probe.py [--log2 16,18,20,22,24,26,28] [--rounds 5] [--dtypes u32,f32,u64] [--out profiles/topk_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

DTYPES = {"u32": (rsa.U32, torch.int32), "f32": (rsa.F32, torch.int32), "u64": (rsa.U64, torch.int64)}
KEYSETS = [("uniform", 0xFFFFFFFFFFFFFFFF), ("dup-heavy", 0xFFF000FF)]     # (the benchmark configs' & 0xFFF000FF keys)
ROUTES = ["TRIVIAL", "SELECT", "SORT"]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(value):
    if value is None:
        os.environ.pop("RSX_TOPK_FORCE", None)
    else:
        os.environ["RSX_TOPK_FORCE"] = value
    rsa.reload_env()


def derived_keys(src, code):
    """basic_kdfs::kdf of the bit patterns as int64 values whose signed order is the library's order"""
    if code == rsa.U64:
        return src ^ torch.iinfo(torch.int64).min
    u = src.to(torch.int64) & 0xFFFFFFFF
    if code == rsa.F32:
        neg = (u >> 31) != 0
        return torch.where(neg, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    return u


def ks_for(n):
    return [k for k in sorted({1, 64, 4096, 1 << 16, 1 << 20, n // 16, n // 4, n // 2}) if k <= n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="16,18,20,22,24,26,28")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtypes", default="u32,f32,u64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rsa.require_gpu()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/topk_probe.py: %d timed rounds after one checked warm-up round; ms, median [min .. max]" % args.rounds)
    emit("# %-4s %-9s %5s %10s %-7s | %-25s | %-25s | %-25s | %-25s | %-25s" % (
        "type", "keys", "log2n", "k", "default", "select (FORCE=1)", "sort (FORCE=2)", "default", "rank sort + slice", "torch.topk"))
    for name in args.dtypes.split(","):
        code, tdt = DTYPES[name]
        for kname, mask in KEYSETS:
            for lg in [int(x) for x in args.log2.split(",")]:
                n = 1 << lg
                src = torch.empty(n, dtype=tdt, device="cuda")
                ib = torch.empty(2 * n, dtype=torch.int32, device="cuda")
                rsa.fill_splitmix(src, 9000, mask)
                order = torch.sort(derived_keys(src, code), stable=True)[1]
                for k in ks_for(n):
                    want_idx = order[:k].to(torch.int32)
                    want_keys = src[order[:k]]
                    keys = torch.empty(k, dtype=tdt, device="cuda")
                    idx = torch.empty(k, dtype=torch.int32, device="cuda")
                    t = {m: [] for m in ("select", "sort", "default", "rank", "torch")}
                    route = None
                    for r in range(args.rounds + 1):
                        if r:
                            rsa.fill_splitmix(src, 9000 + 131 * r + k % 127, mask)
                        for m, value in (("select", "1"), ("sort", "2"), ("default", None)):
                            setenv(value)
                            ms, (_, _, info) = timed(lambda: rsa.radix_sort_topk(src, k, dtype=code, keys_out=keys, idx_out=idx))
                            t[m].append(ms)
                            if m == "default":
                                route = info.route
                            if r == 0:
                                assert torch.equal(idx, want_idx) and torch.equal(keys, want_keys), (name, kname, lg, k, m)
                        ms, _ = timed(lambda: rsa.radix_sort_rank(src, ib, dtype=code)[0][:k])
                        t["rank"].append(ms)
                        view = src.view(torch.float32) if code == rsa.F32 else src
                        ms, _ = timed(lambda: torch.topk(view, k, largest=False))
                        t["torch"].append(ms)

                    def fmt(v):
                        v = v[1:]
                        return "%8.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))
                    med = {m: statistics.median(v[1:]) for m, v in t.items()}
                    best = min(("select", "sort"), key=lambda m: med[m])
                    spread = max(t[best][1:]) - min(t[best][1:])
                    flag = "!" if med["default"] > med[best] + spread else " "
                    emit("%s %-4s %-9s %5d %10d %-7s | %s | %s | %s | %s | %s" % (
                        flag, name, kname, lg, k, ROUTES[route], fmt(t["select"]), fmt(t["sort"]), fmt(t["default"]), fmt(t["rank"]),
                        fmt(t["torch"])))
                del src, ib, order
                torch.cuda.empty_cache()
    setenv(None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
