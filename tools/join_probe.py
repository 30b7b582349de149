"""radix_sort_join's two phases against their own forced routes and against what a caller had to do before them (DESIGN.md 4p;
profiles/join/join_probe.txt).

Phase 1: for every input row four things are timed in ONE process, alternating, after a warm-up round, each between two device
events and ending in a synchronise:
    default   rsx_sort_join_device as it chooses its route (start, count and right_perm wanted, 4-byte indices)
    search    the same with RSX_JOIN_FORCE=2: the right side sorted with an iota, the left keys searched as they come
    merge     the same with RSX_JOIN_FORCE=3: the left side sorted too, the sorted left keys searched, start / count scattered back
    before    the way before the call: radix_sort_rank of the right keys, a gather of them through the permutation, and
              torch.searchsorted of the left keys on both sides (keys are non-negative i32 / i64 so that torch orders them as
              the library does)
The 2-versus-3 rule (join_use_merge, rsx_join_shape.hpp) and the acceptance rule of DESIGN.md 4h / 4l / 4m are read from these
rows: the default may not be slower than the better forced route beyond the row's min .. max spread.

Phase 2: ranges made on the device -- counts all 1, all 16, Zipf-like, one row holding half of all pairs -- are expanded by
rsx_join_pairs_device and by torch (cumsum + repeat_interleave + two gathers); the last columns give the bytes written per
second and that as a fraction of the in-pipeline copy rate of DESIGN.md section 5 (5.1 TB/s).

A run may be cut into pieces that append to one file: `--rows 0,1,2` takes the phase-1 rows of that number only, `--phase 1|2`
one phase only.

    python tools/join_probe.py [--log2 26] [--rounds 5] [--phase 1] [--rows 0,1] [--out profiles/join/join_probe.txt] [--append [--header]]
                               [--no-before] [--idx 4]
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

ROUTES = ["TRIVIAL", "TABLE", "SEARCH", "MERGE"]
COPY_RATE_GBS = 5100.0


def rows(log2):
    """(name, dtype code, carrier, left mask, right mask, log2 of m; None: m = n)"""
    r = [("u8 x u8", rsa.U8, torch.int8, 0x7F, 0x7F, 16)]
    for lm in (12, 16, 20):
        r.append(("u32 dense ids m=2^%d" % lm, rsa.I32, torch.int32, (1 << lm) - 1, (1 << lm) - 1, lm))
    for lm in (20, 24, None):
        r.append(("u32 uniform m=%s" % ("n" if lm is None else "2^%d" % lm), rsa.I32, torch.int32, 0x7FFFFFFF, 0x7FFFFFFF, lm))
    r.append(("u64 < 2^40 m=2^24", rsa.I64, torch.int64, (1 << 40) - 1, (1 << 40) - 1, 24))
    return r


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(force=None):
    if force is None:
        os.environ.pop("RSX_JOIN_FORCE", None)
    else:
        os.environ["RSX_JOIN_FORCE"] = str(force)
    rsa.reload_env()


def fmt(v):
    v = v[1:]
    if not v:
        return "%26s" % "-"
    if len(v) == 1:
        return "%8.3f %17s" % (v[0], "(one round)")
    return "%8.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))


def phase1(args, emit, picked):
    n = 1 << args.log2
    idt = torch.int32 if args.idx == 4 else torch.int64
    emit("# phase 1: n = 2^%d left rows, %d-byte indices, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.idx, args.rounds))
    emit("# %-24s %-7s | %-26s | %-26s | %-26s | %-26s | pairs" % ("input", "route", "default", "RSX_JOIN_FORCE=2 (search)", "RSX_JOIN_FORCE=3 (merge)",
                                                                 "rank + searchsorted x 2"))
    for number, (name, dt, tdt, lmask, rmask, lm) in enumerate(rows(args.log2)):
        if picked is not None and number not in picked:
            continue
        m = n if lm is None else min(n, 1 << lm)
        left, right = torch.empty(n, dtype=tdt, device="cuda"), torch.empty(m, dtype=tdt, device="cuda")
        rsa.fill_splitmix(left, 5151, lmask)
        rsa.fill_splitmix(right, 5252, rmask)
        st, ct, pm = (torch.empty(size, dtype=idt, device="cuda") for size in (n, n, m))
        ibuf = torch.empty(2 * m, dtype=idt, device="cuda")
        torch.cuda.synchronize()

        def call():
            return rsa.radix_sort_join_ranges(left, right, dtype=dt, start=st, count=ct, right_perm=pm)

        def before():
            perm, _ = rsa.radix_sort_rank(right, ibuf, dtype=dt)
            sr = right[perm.long()] if perm.dtype != torch.int64 else right[perm]
            lo = torch.searchsorted(sr, left, out_int32=args.idx == 4)
            hi = torch.searchsorted(sr, left, right=True, out_int32=args.idx == 4)
            return hi - lo

        t = {"default": [], "search": [], "merge": [], "before": []}
        started = time.time()
        route, pairs = None, 0
        for r in range(args.rounds + 1):
            setenv()
            ms, out = timed(call)
            route, pairs = out[4].route, out[0]
            t["default"].append(ms)
            setenv(2)
            ms, out = timed(call)
            assert out[4].route == rsa.JOIN_SEARCH and out[0] == pairs
            t["search"].append(ms)
            setenv(3)
            ms, out = timed(call)
            assert out[4].route == rsa.JOIN_MERGE and out[0] == pairs
            t["merge"].append(ms)
            setenv()
            if not args.no_before and r < 3:
                ms, res = timed(before)
                del res
                t["before"].append(ms)
        emit("  %-24s %-7s | %s | %s | %s | %s | %d" % (name, ROUTES[route], fmt(t["default"]), fmt(t["search"]), fmt(t["merge"]), fmt(t["before"]), pairs))
        print("    (%.1f s of wall time)" % (time.time() - started), flush=True)
        del left, right, st, ct, pm, ibuf
        torch.cuda.empty_cache()


def phase2(args, emit):
    n = 1 << args.log2
    idt = torch.int32 if args.idx == 4 else torch.int64
    emit("# phase 2: %d-byte indices, %d rounds after one warm-up; ms, median [min .. max]; the rows are sized to about 2^%d pairs" % (args.idx, args.rounds, args.log2))
    emit("# %-28s %12s %12s | %-26s | %-26s | GB/s written, of the copy rate" % ("counts", "rows", "pairs", "rsx_join_pairs_device", "torch cumsum + repeat_interleave"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6262)

    def zipf(rows_):
        u = torch.rand(rows_, device="cuda", generator=gen, dtype=torch.float64).clamp_(min=1e-9)
        c = (1.0 / u ** 1.1 - 1.0).clamp_(max=float(1 << 20)).to(torch.int64)
        return c

    shapes = [("all 1", lambda: torch.ones(n, dtype=torch.int64, device="cuda")),
              ("all 16", lambda: torch.full((n // 16,), 16, dtype=torch.int64, device="cuda")),
              ("Zipf-like (many zeros)", lambda: zipf(n // 32)),
              ("one row holds half", None)]
    for name, make in shapes:
        if make is None:
            count = torch.ones(n // 2, dtype=torch.int64, device="cuda")
            count[n // 4] = n // 2
        else:
            count = make()
        rows_ = count.numel()
        m = int(max(int(count.max().item()), 1 << 20))
        start = (torch.rand(rows_, device="cuda", generator=gen, dtype=torch.float64) * (m - count + 1).to(torch.float64)).to(torch.int64).clamp_(min=0)
        start = torch.minimum(start, m - count)
        perm = torch.randperm(m, device="cuda", generator=gen)
        st, ct, pm = start.to(idt), count.to(idt), perm.to(idt)
        total = int(count.sum().item())
        ol_t, or_t = torch.empty(total, dtype=idt, device="cuda"), torch.empty(total, dtype=idt, device="cuda")
        del start, perm
        torch.cuda.synchronize()

        def call():
            return rsa.radix_sort_join_pairs(st, ct, pm, left_idx=ol_t, right_idx=or_t)[2]

        def before():
            c64 = ct.to(torch.int64)
            first = torch.cumsum(c64, 0) - c64
            li = torch.repeat_interleave(torch.arange(rows_, device="cuda"), c64, output_size=total)
            t_ = torch.arange(total, device="cuda") - first[li]
            ri = pm[(st.to(torch.int64)[li] + t_)]
            return li.to(idt), ri

        t = {"call": [], "before": []}
        for r in range(args.rounds + 1):
            ms, got = timed(call)
            assert got == total
            t["call"].append(ms)
            if not args.no_before and r < 3:
                ms, res = timed(before)
                if r == 0:
                    assert torch.equal(res[0], ol_t) and torch.equal(res[1], or_t), name
                del res
                t["before"].append(ms)
        gbs = total * 2 * args.idx / statistics.median(t["call"][1:]) / 1e6
        emit("  %-28s %12d %12d | %s | %s | %6.0f  %4.2f" % (name, rows_, total, fmt(t["call"]), fmt(t["before"]), gbs, gbs / COPY_RATE_GBS))
        del st, ct, pm, ol_t, or_t, count
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--idx", type=int, default=4, choices=(4, 8))
    ap.add_argument("--phase", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-before", action="store_true")
    ap.add_argument("--header", action="store_true", help="write the header line although appending")
    ap.add_argument("--rows", default=None, help="comma-separated numbers of phase-1 rows (default: all)")
    args = ap.parse_args()
    rsa.require_gpu()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out and lines:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a" if (args.append or flush.done) else "w") as f:
                f.write("\n".join(lines) + "\n")
            flush.done = True
            del lines[:]

    flush.done = False
    picked = None if args.rows is None else {int(x) for x in args.rows.split(",")}
    if not args.append or args.header:
        emit("# tools/join_probe.py --log2 %d --idx %d" % (args.log2, args.idx))
    if args.phase in (0, 1):
        phase1(args, emit, picked)
        flush()
    if args.phase in (0, 2):
        phase2(args, emit)
        flush()


if __name__ == "__main__":
    main()
