"""radix_sort_nth against the rank sort it replaces (profiles/nth_probe.txt).

For every (key set, n, m) four things are timed in ONE process, alternating inside each round, each between two device events
and ending in a synchronise:
    select    rsx_sort_nth_device with RSX_NTH_FORCE=1 (multi-rank MSD radix select, then a sort of the candidates)
    sort      the same with RSX_NTH_FORCE=2 (the rank sort, m entries read through the ranks)
    default   the same with the switch unset (the library's own choice; its route is printed)
    rank      rsx_sort_rank_device and a gather of m entries: the only way before this entry point existed -- the yardstick
The m ranks are evenly spaced ((2 i + 1) n / 2 m: the median for m = 1, deciles' neighbours for m = 9).  Round 0 warms every
shape up and CHECKS each of the three results on the device against torch.sort(stable=True) of the derived keys; rounds 1 .. R
are timed, each on keys freshly generated from a seed of its own.  Printed: the median and [min .. max] of the timed rounds
in ms, and what the select route reported (histogram levels / reads of the input / candidates).  A row is marked "!" when the
default is slower than the better forced route by more than the spread (max - min) that route shows in the same row.

    python tools/nth_probe.py [--log2 18,20,22,24,26,28] [--m 1,9,64] [--rounds 5] [--keys u32,f32,u64] [--out profiles/nth_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

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
        os.environ.pop("RSX_NTH_FORCE", None)
    else:
        os.environ["RSX_NTH_FORCE"] = value
    rsa.reload_env()


def fill_u32(src, seed):
    rsa.fill_splitmix(src, seed)


def fill_f32(src, seed):
    """uniform floats in [0, 1), as their bit patterns"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    src.copy_(torch.rand(src.numel(), device="cuda", dtype=torch.float32, generator=g).view(torch.int32))


def fill_u64(src, seed):
    rsa.fill_splitmix(src, seed, (1 << 40) - 1)


# name: (rsx dtype, tensor dtype, generator)
KEYS = {"u32": (rsa.U32, torch.int32, fill_u32), "f32": (rsa.F32, torch.int32, fill_f32), "u64": (rsa.U64, torch.int64, fill_u64)}


def derived_keys(src, code):
    """basic_kdfs::kdf of the bit patterns as int64 values whose signed order is the library's order"""
    if code == rsa.U64:
        return src ^ torch.iinfo(torch.int64).min
    u = src.to(torch.int64) & 0xFFFFFFFF
    if code == rsa.F32:
        neg = (u >> 31) != 0
        return torch.where(neg, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="18,20,22,24,26,28")
    ap.add_argument("--m", default="1,9,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--keys", default="u32,f32,u64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rsa.require_gpu()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/nth_probe.py: %d timed rounds after one checked warm-up round; ms, median [min .. max]" % args.rounds)
    emit("# %-4s %5s %3s %-7s %-12s | %-25s | %-25s | %-25s | %-25s" % (
        "keys", "log2n", "m", "default", "lvl/rd/cand", "select (FORCE=1)", "sort (FORCE=2)", "default", "rank sort + gather"))
    for name in args.keys.split(","):
        code, tdt, fill = KEYS[name]
        for lg in [int(x) for x in args.log2.split(",")]:
            n = 1 << lg
            src = torch.empty(n, dtype=tdt, device="cuda")
            ib = torch.empty(2 * n, dtype=torch.int32, device="cuda")
            for m in [int(x) for x in args.m.split(",")]:
                ranks = [((2 * i + 1) * n) // (2 * m) for i in range(m)]
                ranks_t = torch.tensor(ranks, dtype=torch.int64, device="cuda")
                keys = torch.empty(m, dtype=tdt, device="cuda")
                idx = torch.empty(m, dtype=torch.int32, device="cuda")
                t = {k: [] for k in ("select", "sort", "default", "rank")}
                route, course = None, ""
                for r in range(args.rounds + 1):
                    fill(src, 9100 + 131 * r + m)
                    torch.cuda.synchronize()
                    if r == 0:
                        order = torch.sort(derived_keys(src, code), stable=True)[1]
                        want_idx = order[ranks_t].to(torch.int32)
                        want_keys = src[order[ranks_t]]
                        del order
                    for k, value in (("select", "1"), ("sort", "2"), ("default", None)):
                        setenv(value)
                        ms, (_, _, n_less, n_equal, info) = timed(
                            lambda: rsa.radix_sort_nth(src, ranks, dtype=code, keys_out=keys, idx_out=idx))
                        t[k].append(ms)
                        if k == "default":
                            route = info.route
                        if k == "select" and info.route == rsa.NTH_SELECT:
                            course = "%d/%d/%d" % (info.digit_passes, info.input_reads, info.candidates)
                        if r == 0:
                            assert torch.equal(idx, want_idx) and torch.equal(keys, want_keys), (name, lg, m, k)
                            assert all(int(a) <= q < int(a) + int(b) for a, b, q in zip(n_less, n_equal, ranks)), (name, lg, m, k)

                    def yardstick():
                        res = rsa.radix_sort_rank(src, ib, dtype=code)[0]
                        at = res[ranks_t]
                        return src[at.to(torch.int64)], at
                    ms, _ = timed(yardstick)
                    t["rank"].append(ms)

                def fmt(v):
                    v = v[1:]
                    return "%8.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))
                med = {k: statistics.median(v[1:]) for k, v in t.items()}
                best = min(("select", "sort"), key=lambda k: med[k])
                spread = max(t[best][1:]) - min(t[best][1:])
                flag = "!" if med["default"] > med[best] + spread else " "
                emit("%s %-4s %5d %3d %-7s %-12s | %s | %s | %s | %s" % (
                    flag, name, lg, m, ROUTES[route], course, fmt(t["select"]), fmt(t["sort"]), fmt(t["default"]), fmt(t["rank"])))
            del src, ib
            torch.cuda.empty_cache()
    setenv(None)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
