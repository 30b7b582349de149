"""radix_sort_segments against what a caller had to do before it (profiles/segments/segments_probe.txt).

For every shape three things are timed, each call between two device events and ending in a synchronise, after a warm-up call:
    baseline  what the PARENT commit offers through its public API for the same job: an id column built with torch
              (repeat_interleave of the segment numbers over the lengths), radix_sort_lex([ids, keys]), a gather of the keys and
              the subtraction of the segment's start from the permutation (local indices).  With --baseline-root DIR (a built
              checkout of the parent commit) it runs there, in a process of its own, once before and once after this build's
              rounds; its repetitions of both blocks make its spread.  Without, it runs on this build, whose radix_sort_lex is the
              parent's code, alternating with the other two -- and the heading says so.
    lds       radix_sort_segments with RSX_SEGMENTS_FORCE=1 and RSX_SEGMENTS_MAX_LONG=4096: the LDS route, MIXED where segments
              are longer than cap
    lex       the same with RSX_SEGMENTS_FORCE=2: the composed route
Shapes: 2^log2 u32 keys in uniform rows of 16, 256, 4096 and cap, keys + local indices; i32 keys under CSR-like offsets with
geometric lengths of mean 16, without long rows and with --long-counts rows of 100000 keys; f32 rows of 131072 keys (long rows
only) -- 2^log2 keys of them like every other shape, so [512, 131072] and [32, 131072], not the [64, 131072] a single batch would be.
Last column: the LDS route's algorithmic traffic -- the keys read once, keys and indices written once -- over the median time of the
WHOLE CALL (the plan kernels, the host's wait for the plan record and every launch: a whole-call figure, not a kernel's share of
peak), as a share of 8 TB/s (bandwidth-bound: the least time the hardware could take is the traffic over the peak bandwidth).
A timed window is ONE call: at 2^22 keys (0.05 .. 0.5 ms) it holds as much launch and synchronise overhead as kernel time; the rows
that decide defaults are those at 2^26 keys.

    python tools/segments_probe.py [--log2 26,22] [--rounds 5] [--long-counts 0,8] [--baseline-root DIR] [--out profiles/segments/segments_probe.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12
LONG_ROW = 100000


LONG_COUNTS = (0, 8)


def shapes(log2, cap):
    n = 1 << log2
    out = [("u32 rows of %d" % r, "U32", "uniform", r) for r in (16, 256, 4096, cap)]
    out += [("i32 csr mean 16" + (" + %d long" % k if k else ""), "I32", "csr", k) for k in LONG_COUNTS]
    if n >= 131072:
        out.append(("f32 rows of 131072", "F32", "uniform", 131072))
    return out


def make(torch, rsa, log2, kind, arg, tdt, seed=4242):
    """(keys, offsets int32 or None, rows or None): n is cut to a whole number of rows for uniform shapes"""
    n = 1 << log2
    if kind == "uniform":
        rows = max(1, n // arg)
        keys = torch.empty(rows * arg, dtype=tdt, device="cuda")
        rsa.fill_splitmix(keys, seed)
        return keys, None, rows
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    m = n // 16
    u = torch.rand(m, device="cuda", generator=g).clamp_(1e-9, 1.0)
    lengths = torch.floor(torch.log(u) / torch.log(torch.tensor(1.0 - 1.0 / 17.0, device="cuda"))).to(torch.int64)     # geometric, mean 16
    if arg:
        lengths[torch.arange(arg, device="cuda") * (m // arg)] = LONG_ROW
    offsets = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lengths, 0, out=offsets[1:])
    total = int(offsets[-1])
    keys = torch.empty(total, dtype=tdt, device="cuda")
    rsa.fill_splitmix(keys, seed)
    return keys, offsets.to(torch.int32), None


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def baseline_call(torch, rsa, keys, offsets, rows):
    """the parent's public API: ids by torch, radix_sort_lex, the gathers"""
    n = keys.numel()
    if offsets is None:
        m, length = rows, n // rows
        ids = torch.arange(m, dtype=torch.int32, device="cuda").repeat_interleave(length)
        starts = ids * length
    else:
        m = offsets.numel() - 1
        lengths = (offsets[1:] - offsets[:-1]).to(torch.int64)
        ids = torch.repeat_interleave(torch.arange(m, dtype=torch.int32, device="cuda"), lengths, output_size=n)
        starts = offsets[ids.to(torch.int64)]
    perm, _ = rsa.radix_sort_lex([ids, keys])
    return keys[perm.to(torch.int64)], perm - starts


def run_baseline(log2s, rounds, cap):
    """this process: the baseline alone, one JSON line per shape (used through --baseline-only in the parent's checkout)"""
    import torch
    import radix_sorting_amd as rsa
    rsa.require_gpu()
    TD = {"U32": torch.int32, "I32": torch.int32, "F32": torch.float32}
    for log2 in log2s:
        for name, dname, kind, arg in shapes(log2, cap):
            keys, offsets, rows = make(torch, rsa, log2, kind, arg, TD[dname])
            ts = []
            for r in range(rounds + 1):
                ms, res = timed(torch, lambda: baseline_call(torch, rsa, keys, offsets, rows))
                del res
                ts.append(ms)
            print(json.dumps({"log2": log2, "shape": name, "ms": ts[1:]}), flush=True)
            del keys, offsets
            torch.cuda.empty_cache()


def baseline_in(root, log2s, rounds, cap):
    root = os.path.abspath(root)
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-only", "--log2", ",".join(map(str, log2s)), "--rounds", str(rounds), "--cap", str(cap),
           "--long-counts", ",".join(map(str, LONG_COUNTS))]
    env = dict(os.environ, PYTHONPATH=root)
    env.pop("RSX_LIB", None)
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root, timeout=1500)
    if out.returncode != 0:
        raise SystemExit("the baseline in %s failed:\n%s\n%s" % (root, out.stdout, out.stderr))
    res = {}
    for line in out.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            res[(d["log2"], d["shape"])] = d["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="26,22")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--cap", type=int, default=0)
    ap.add_argument("--long-counts", default="0,8", help="the CSR shape with these many rows of %d keys among the others" % LONG_ROW)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    log2s = [int(x) for x in args.log2.split(",")]
    global LONG_COUNTS
    LONG_COUNTS = tuple(int(x) for x in args.long_counts.split(","))
    if args.baseline_only:
        # (the package comes from PYTHONPATH: the checkout this process was started in)
        return run_baseline(log2s, args.rounds, args.cap)
    sys.path.insert(0, ROOT)
    import torch
    import radix_sorting_amd as rsa
    rsa.require_gpu()
    TD = {"U32": torch.int32, "I32": torch.int32, "F32": torch.float32}
    CODE = {"U32": rsa.U32, "I32": rsa.I32, "F32": rsa.F32}
    ROUTES = ["TRIVIAL", "LDS", "MIXED", "LEX"]
    cap = rsa.SEGMENTS_CAP(rsa.U32, True)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def setenv(force):
        os.environ["RSX_SEGMENTS_FORCE"] = force
        os.environ["RSX_SEGMENTS_MAX_LONG"] = "4096"
        rsa.reload_env()

    def fmt(v):
        return "%8.3f [%8.3f .. %8.3f]" % (statistics.median(v), min(v), max(v))

    before = baseline_in(args.baseline_root, log2s, args.rounds, cap) if args.baseline_root else {}
    own = {}
    for log2 in log2s:
        for name, dname, kind, arg in shapes(log2, cap):
            keys, offsets, rows = make(torch, rsa, log2, kind, arg, TD[dname])
            n = keys.numel()
            keys_out = torch.empty_like(keys)
            idx_out = torch.empty(n, dtype=torch.int32, device="cuda")
            t = {"lds": [], "lex": [], "base": []}
            infos = {}
            for r in range(args.rounds + 1):
                for which, force in (("lds", "1"), ("lex", "2")):
                    setenv(force)
                    ms, out = timed(torch, lambda: rsa.radix_sort_segments(keys, offsets=offsets, rows=rows, dtype=CODE[dname], keys=keys_out, idx=idx_out,
                                                                           local_idx=True))
                    infos[which] = out[0]
                    t[which].append(ms)
                if not args.baseline_root:
                    ms, res = timed(torch, lambda: baseline_call(torch, rsa, keys, offsets, rows))
                    del res
                    t["base"].append(ms)
            own[(log2, name)] = (n, {k: v[1:] for k, v in t.items()}, infos)
            del keys, offsets, keys_out, idx_out
            torch.cuda.empty_cache()
    after = baseline_in(args.baseline_root, log2s, args.rounds, cap) if args.baseline_root else {}

    emit("# tools/segments_probe.py: keys + local 4-byte indices, %d rounds after one warm-up; ms, median [min .. max]" % args.rounds)
    emit("# baseline: torch ids + radix_sort_lex([ids, keys]) + gathers, %s" % (
        "on a build of the parent commit, a block of rounds before and one after this build's" if args.baseline_root
        else "ON THIS BUILD (its radix_sort_lex is the parent's code), alternating with the other two"))
    emit("# %-26s %10s %-6s | %-29s | %-29s | %-29s | %-9s | lds: whole call's share of 8 TB/s" % (
        "shape", "n", "route", "RSX_SEGMENTS_FORCE=1", "RSX_SEGMENTS_FORCE=2", "baseline", "lds wins?"))
    for (log2, name), (n, t, infos) in own.items():
        base = (before.get((log2, name), []) + after.get((log2, name), [])) if args.baseline_root else t["base"]
        spread = max(base) - min(base)
        med_l, med_b = statistics.median(t["lds"]), statistics.median(base)
        wins = med_b - med_l > spread     # beats the baseline by more than the baseline's own run-to-run spread
        kb = 4
        share = n * (2 * kb + 4) / (med_l * 1e-3) / PEAK
        emit("  %-26s %10d %-6s | %s | %s | %s | %-9s | %5.3f" % (name, n, ROUTES[infos["lds"].route], fmt(t["lds"]), fmt(t["lex"]), fmt(base),
                                                                 "yes" if wins else "no", share))
        emit("    classes %s n_long %d max_len %d; baseline spread %.3f ms" % (infos["lds"].classes(), infos["lds"].n_long, infos["lds"].max_len, spread))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
