"""radix_sort_partition against its own sort route and against what a caller had to do before it (DESIGN.md 4q;
profiles/partition/partition_probe.txt).

For every input row, every number of parts, both kinds of edges and each of the three questions -- keys only, idx only, both --
three things are timed in ONE process, alternating, after a warm-up round, each between two device events and ending in a
synchronise:
    scatter   radix_sort_partition with RSX_PARTITION_MAX_EDGES=255: the scatter route for every number of parts up to 256 (the
              library's default cut-off is what these rows say it should be: DESIGN.md 4q)
    forced    the same with RSX_PARTITION_FORCE=2 (the sort route: locate's bins, their rank sort, a gather)
    torch     the way to the same arrays without the call: torch.bucketize over the sorted edges, torch.sort(stable=True) of the
              bins, a gather of the keys through its indices
The keys are signed or float where torch has no unsigned type of their width, so that torch orders them as the library does.  The
source is never written, so nothing is refilled between the calls.  The spread of a column is the run-to-run spread the
acceptance rule of DESIGN.md 4q refers to.  The last column is its algorithmic traffic -- two reads of the
keys and the outputs written -- over the median time, as a share of 8 TB/s.  Last, the two ranking forms against each other:
every number of parts with RSX_PARTITION_BALLOT_PARTS=256 (ballots) and =0 (per-wave cells in LDS).

    python tools/partition_probe.py [--log2 26] [--rounds 3] [--out profiles/partition/partition_probe.txt] [--append]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import radix_sorting_amd as rsa  # noqa: E402

ROUTES = ["TRIVIAL", "SCATTER", "SORT"]
PEAK = 8e12
SWITCHES = ("RSX_PARTITION_FORCE", "RSX_PARTITION_BALLOT_PARTS", "RSX_PARTITION_MAX_EDGES")


def rows():
    # (name, rsx dtype, torch dtype, the integer type of the same width, mask of the random bits, key bytes, low edge, far edge)
    return [("i32 uniform", rsa.I32, torch.int32, torch.int32, 0xFFFFFFFF, 4, 1000, 1 << 30),
            ("f32 in [0, 2)", rsa.F32, torch.float32, torch.int32, 0x3FFFFFFF, 4, 0x3F000000, 0x3FFFFFFF),
            ("u64 < 2^40", rsa.U64, torch.int64, torch.int64, (1 << 40) - 1, 8, 1000, 1 << 39)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def setenv(**values):
    for name in SWITCHES:
        v = values.get(name)
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    rsa.reload_env()


def edge_lists(src, dt, tdt, idt, n, parts, low, far):
    """(name, edges): parts - 1 quantile splitters of the keys; parts - 1 edges of which all but the last lie in one digit of the start table"""
    m = parts - 1
    keys, _, _, _, _ = rsa.radix_sort_nth(src, [(i + 1) * n // parts for i in range(m)], dtype=dt, want_idx=False)
    out = [("quantiles", keys.clone())]
    if m >= 2:
        v = torch.arange(m - 1, dtype=torch.int64, device="cuda") * 3 + low
        out.append(("one digit", torch.cat([v, torch.tensor([far], dtype=torch.int64, device="cuda")]).to(idt).view(tdt)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="2,4,8,16,64,256")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    rsa.require_gpu()
    n = 1 << args.log2
    parts_list = [int(p) for p in args.parts.split(",")]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:     # (kept up to date line by line: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")

    if args.out and not args.append and os.path.exists(args.out):
        os.remove(args.out)

    def fmt(v):
        v = v[1:]
        return "%8.3f [%8.3f .. %8.3f]" % (statistics.median(v), min(v), max(v))

    emit("# tools/partition_probe.py: n = 2^%d keys, 4-byte indices, %d rounds after one warm-up; ms, median [min .. max]" % (args.log2, args.rounds))
    emit("# %-14s %5s %-10s %-5s %-7s f | %-29s | %-29s | %-29s | scatter: share of 8 TB/s" % ("input", "parts", "edges", "out", "route", "RSX_PARTITION_MAX_EDGES=255", "RSX_PARTITION_FORCE=2", "torch bucketize+sort+gather"))
    for name, dt, tdt, idt, mask, kb, low, far in rows():
        src = torch.empty(n, dtype=tdt, device="cuda")
        rsa.fill_splitmix(src, 4242, mask)
        keys_out = torch.empty_like(src)
        idx_out = torch.empty(n, dtype=torch.int32, device="cuda")
        for parts in parts_list:
            for ename, edges in edge_lists(src, dt, tdt, idt, n, parts, low, far):
                sorted_edges = torch.sort(edges).values
                offsets = torch.empty(parts + 1, dtype=torch.int32, device="cuda")

                def torch_way(want_keys):
                    bins = torch.bucketize(src, sorted_edges, out_int32=True, right=True)
                    order = torch.sort(bins, stable=True).indices
                    return (src[order] if want_keys else None), order

                for oname, want_keys, want_idx in (("keys", True, False), ("idx", False, True), ("both", True, True)):
                    t = {"default": [], "forced": [], "torch": []}
                    info = None
                    call = lambda: rsa.radix_sort_partition(src, edges, dtype=dt, keys=keys_out if want_keys else False,
                                                            idx=idx_out if want_idx else False, offsets=offsets)
                    for r in range(args.rounds + 1):
                        setenv(RSX_PARTITION_MAX_EDGES=255)
                        ms, out = timed(call)
                        info = out[0]
                        assert info.route == rsa.PARTITION_SCATTER
                        t["default"].append(ms)
                        setenv(RSX_PARTITION_FORCE=2)
                        ms, out = timed(call)
                        assert out[0].route == rsa.PARTITION_SORT
                        t["forced"].append(ms)
                        setenv()
                        ms, res = timed(lambda: torch_way(want_keys))
                        del res
                        t["torch"].append(ms)
                    traffic = n * (2 * kb + (kb if want_keys else 0) + (4 if want_idx else 0))
                    share = traffic / (statistics.median(t["default"][1:]) * 1e-3) / PEAK if info.route == rsa.PARTITION_SCATTER else 0.0
                    emit("  %-14s %5d %-10s %-5s %-7s %d | %s | %s | %s | %5.3f" % (name, parts, ename, oname, ROUTES[info.route], info.rank_form, fmt(t["default"]),
                                                                                 fmt(t["forced"]), fmt(t["torch"]), share))
                    torch.cuda.empty_cache()
        # the two ranking forms against each other: quantile edges, both outputs
        emit("# %s: the ranking forms, quantile edges, keys + idx: parts | RSX_PARTITION_BALLOT_PARTS=256 (ballots) | =0 (cells in LDS)" % name)
        for parts in sorted(set(parts_list + [3, 5, 6, 7, 12, 32])):
            edges = edge_lists(src, dt, tdt, idt, n, parts, low, far)[0][1]
            t = {256: [], 0: []}
            for r in range(args.rounds + 1):
                for seam in (256, 0):
                    setenv(RSX_PARTITION_BALLOT_PARTS=seam, RSX_PARTITION_MAX_EDGES=255)
                    ms, out = timed(lambda: rsa.radix_sort_partition(src, edges, dtype=dt, keys=keys_out, idx=idx_out, offsets=False))
                    assert out[0].rank_form == (1 if seam else 2)
                    t[seam].append(ms)
            emit("  %-14s %5d | %s | %s" % (name, parts, fmt(t[256]), fmt(t[0])))
        setenv()
        del src, keys_out, idx_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
