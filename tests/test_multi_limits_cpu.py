"""The exchange of radix_sorting_amd/multi.py with pieces over its size limits, on CPU: world_size-2 and -3 gloo runs.

distributed_sort cuts pieces into parts of at most multi.PIECE_LIMIT bytes once the largest piece of the count matrix reaches
multi.WHOLE_PIECE_MAX bytes.  At their defaults (2^30, 2^31) that code needs 24 GiB and a GPU to run at all; here the workers
lower the two module attributes to tens of kilobytes, so that shards of tens of thousands of keys go through
  * the grouped send / receive in parts of one_exchange (chunks = 1, world >= 2),
  * the part loops of the chunk pipeline's exchange() (chunks > 1),
  * the even-digits hint of local_sort (the engine here takes and records it).
Every run is compared bit for bit with the oracle's sort of the whole input, its recv_counts with the count matrix worked
out here from the input, and its sends and receives -- recorded by wrapping torch.distributed in the worker -- with the parts
that matrix asks for.  Every group has a 60 s timeout: ranks that disagree about the exchange fail, they do not hang.
"""
import json
import os
from datetime import timedelta

import numpy as np
import pytest

import oracle_lib as ol
from radix_sorting_amd import multi
from test_multi_cpu import OracleEngine, _free_port, _skew

torch = pytest.importorskip("torch")
import torch.distributed as dist          # noqa: E402
import torch.multiprocessing as mp        # noqa: E402

_CARRIER = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


class HintEngine(OracleEngine):
    """OracleEngine that is told whether the received bins are even, as HipEngine is, and keeps what it was told."""
    takes_even_hint = True

    def __init__(self, dtype, order=0):
        super().__init__(dtype, order)
        self.evens = []

    def sort_inplace_async(self, buf, scratch, even=False):
        self.evens.append([int(buf.numel()), bool(even)])
        super().sort_inplace_async(buf, scratch)


def _worker(rank, world, port, cfg, outdir):
    """One rank: the shard of outdir/whole.npy, cfg["runs"] = [(chunks, split_slices), ...] one after the other in one group."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    calls = {"a2a": 0, "batches": 0, "ops": []}
    real_a2a, real_batch = dist.all_to_all_single, dist.batch_isend_irecv

    def a2a(*args, **kw):
        calls["a2a"] += 1
        return real_a2a(*args, **kw)

    def batch(ops):
        calls["batches"] += 1
        for op in ops:
            calls["ops"].append(["send" if op.op is dist.isend else "recv", int(op.tensor.numel() * op.tensor.element_size()),
                                 int(op.peer)])
        return real_batch(ops)

    dist.all_to_all_single, dist.batch_isend_irecv = a2a, batch
    try:
        if cfg.get("piece_limit") is not None:
            multi.PIECE_LIMIT = cfg["piece_limit"]
            multi.WHOLE_PIECE_MAX = cfg["whole_max"]
        dtype, order, n_per_rank = cfg["dtype"], cfg["order"], cfg["n_per_rank"]
        whole = np.load(os.path.join(outdir, "whole.npy"))
        first = sum(n_per_rank[:rank])
        shard = torch.from_numpy(whole[first:first + n_per_rank[rank]].view(_CARRIER[ol.DTYPE_SIZE[dtype]]).copy())
        report = []
        for i, (chunks, slices) in enumerate(cfg["runs"]):
            calls.update(a2a=0, batches=0, ops=[])
            engine = HintEngine(dtype, order)
            res, stats = multi.distributed_sort(shard, engine, chunks=chunks, split_slices=slices)
            np.save(os.path.join(outdir, "out%d_%d.npy" % (rank, i)), res.numpy().view(ol.NP_BITS[dtype]).copy())
            report.append({"a2a": calls["a2a"], "batches": calls["batches"], "ops": calls["ops"], "evens": engine.evens,
                           "recv_counts": [int(x) for x in stats["recv_counts"]],
                           "send_counts": [int(x) for x in stats["send_counts"]], "chunks": int(stats["chunks"]),
                           "split_slices": int(stats.get("split_slices", 1)), "levels": int(stats["refine_levels"])})
        with open(os.path.join(outdir, "report%d.json" % rank), "w") as f:
            json.dump(report, f)
    finally:
        dist.all_to_all_single, dist.batch_isend_irecv = real_a2a, real_batch
        dist.destroy_process_group()


def plan_from_input(whole, dtype, order, n_per_rank, chunks=1, slices=1):
    """What distributed_sort has to arrive at, worked out from the whole input with numpy: the bins (digits of the highest
    byte that varies, a bin with more than multi.HEAVY_FACTOR fair shares divided by the next byte, level by level), the
    splitters and sub-ranges over them, and from these every piece:
    pieces[s, d, j, i] = keys of rank s's part i of the split that go to rank d in sub-range j; matrix = pieces summed over j, i."""
    world = len(n_per_rank)
    k = ol.kdf_keys(whole, dtype, order).astype(np.uint64)
    rank_of = np.repeat(np.arange(world), n_per_rank)
    column = 0
    for c in range(ol.DTYPE_SIZE[dtype] - 1, -1, -1):
        if np.unique((k >> np.uint64(8 * c)) & np.uint64(0xFF)).size > 1:
            column = c
            break
    below = np.uint64((1 << (8 * (column + 1))) - 1)
    depth = np.zeros(k.size, dtype=np.uint64)         # how many bytes below `column` the key's bin is divided by
    levels = 0
    while True:
        low = np.uint64(8) * (np.uint64(column) - depth)
        _, inv = np.unique(((k & below) >> low) << low, return_inverse=True)      # (bins in key order; the empty ones left out)
        inv = inv.reshape(-1)
        counts = np.zeros((world, int(inv.max()) + 1), dtype=np.uint64)
        np.add.at(counts, (rank_of, inv), 1)
        too = multi.heavy_bins(counts.sum(axis=0), world, column - levels)
        if not too:
            break
        levels += 1
        depth[np.isin(inv, too)] += np.uint64(1)
    total = counts.sum(axis=0)
    lut = multi.choose_splitters(total, world).astype(np.int64)
    if chunks == 1 or levels > 0:
        slices = 1
    chunk_of = multi.choose_chunks(total, lut, world, chunks) if chunks > 1 else np.zeros(total.size, dtype=np.int64)
    slice_of = np.concatenate([np.searchsorted(np.asarray(multi.slice_bounds(n, slices)[1:]), np.arange(n), side="right")
                               for n in n_per_rank])
    pieces = np.zeros((world, world, max(chunks, 1), slices), dtype=np.int64)
    np.add.at(pieces, (rank_of, lut[inv], chunk_of[inv], slice_of), 1)
    return {"matrix": pieces.sum(axis=(2, 3)), "pieces": pieces, "levels": levels, "column": column, "slices": slices}


def parts_of(count, step):
    return -(-int(count) // step)


def run_case(tmp_path, whole, dtype, order, n_per_rank, runs, piece_limit=None, whole_max=None):
    """Spawn the ranks; check every run's output, counts and recorded sends / receives; return the ranks' reports."""
    world = len(n_per_rank)
    np.save(os.path.join(str(tmp_path), "whole.npy"), whole)
    cfg = {"dtype": dtype, "order": order, "n_per_rank": list(n_per_rank), "runs": list(runs), "piece_limit": piece_limit,
           "whole_max": whole_max}
    mp.spawn(_worker, args=(world, _free_port(), cfg, str(tmp_path)), nprocs=world, join=True)
    want = ol.oracle_sort(whole, dtype, order)[0]
    reports = [json.load(open(os.path.join(str(tmp_path), "report%d.json" % r))) for r in range(world)]
    es = ol.DTYPE_SIZE[dtype]
    for i, (chunks, slices) in enumerate(runs):
        got = np.concatenate([np.load(os.path.join(str(tmp_path), "out%d_%d.npy" % (r, i))) for r in range(world)])
        assert got.dtype == want.dtype and np.array_equal(got, want), (chunks, slices)
        plan = plan_from_input(whole, dtype, order, n_per_rank, chunks, slices)
        for r in range(world):
            rep = reports[r][i]
            assert rep["recv_counts"] == [int(x) for x in plan["matrix"][:, r]], (r, chunks, slices)
            assert rep["send_counts"] == [int(x) for x in plan["matrix"][r]], (r, chunks, slices)
            assert rep["chunks"] == chunks and rep["split_slices"] == plan["slices"] and rep["levels"] == plan["levels"]
            if piece_limit is None:
                continue
            # the parts: a rank's own piece is copied, every other piece goes in ceil(count / step) sends against as many receives
            step = piece_limit // es
            big = int(plan["matrix"].max()) * es >= whole_max
            sends = [op for op in rep["ops"] if op[0] == "send"]
            recvs = [op for op in rep["ops"] if op[0] == "recv"]
            assert all(op[2] != r for op in rep["ops"]), "rank %d sends to itself" % r
            assert all(0 < op[1] <= step * es for op in rep["ops"]), (r, step * es, sorted(op[1] for op in rep["ops"])[-3:])
            if chunks == 1 and not big:
                assert rep["a2a"] == 1 and not rep["ops"]
                continue
            assert rep["a2a"] == 0
            for kind, got_ops, mine in (("send", sends, plan["pieces"][r]), ("recv", recvs, plan["pieces"][:, r])):
                for p in range(world):
                    if p != r:
                        want_parts = sum(parts_of(c, step) for c in mine[p].reshape(-1))
                        assert len([op for op in got_ops if op[2] == p]) == want_parts, (kind, r, p, chunks, slices)
                        assert sum(op[1] for op in got_ops if op[2] == p) == int(mine[p].sum()) * es
    return reports


def lopsided(world, seed=61):
    """Rank 0 holds 60000 keys in the lowest 1 / world of the key range, the other ranks 60000 / (world - 1) (two ranks: 20000) over
    the rest of it.  Rank 0 then keeps most of its shard: a piece about twice the size of any other in the matrix."""
    n_per_rank = [60000, 20000] if world == 2 else [60000] + [60000 // (world - 1)] * (world - 1)
    a =ol.splitmix_fill(sum(n_per_rank), ol.U32, seed).astype(np.uint64)
    cut = (1 << 32) // world
    a[:60000] %= np.uint64(cut)
    a[60000:] = np.uint64(cut) + a[60000:] % np.uint64((1 << 32) - cut)
    return a.astype(np.uint32), n_per_rank


def designed(matrix, seed):
    """u32 keys whose count matrix is `matrix` (its column sums must be equal): rank s holds matrix[s][d] keys with a top byte
    in destination d's range of digits [256 d / world, 256 (d + 1) / world), in random order."""
    m = np.asarray(matrix, dtype=np.int64)
    world = m.shape[0]
    assert len(set(int(x) for x in m.sum(axis=0))) == 1
    rng = np.random.default_rng(seed)
    shards = []
    for s in range(world):
        keys = [(rng.integers(256 * d // world, 256 * (d + 1) // world, int(m[s, d])).astype(np.uint32) << np.uint32(24))
                | rng.integers(0, 1 << 24, int(m[s, d])).astype(np.uint32) for d in range(world)]
        shards.append(rng.permutation(np.concatenate(keys)))
    return np.concatenate(shards), [int(x) for x in m.sum(axis=1)]


def sees_big(matrix, r, es, whole_max):
    """What rank r alone can tell from its row and column of the matrix (how `big` was decided before it came from the whole matrix)."""
    return max(int(matrix[r].max()), int(matrix[:, r].max())) * es >= whole_max


# ---- only one rank sees a big piece -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
def test_a_big_piece_that_only_one_rank_sees(tmp_path, world):
    """Rank 0 keeps a piece of exactly WHOLE_PIECE_MAX bytes; no other piece of the matrix reaches it, so ranks 1.. see no big piece
    in their own rows and columns.  Every rank must still cut the pieces in the same parts: `big` comes from the whole matrix.
    (Decided per rank, rank 0 posted sends in parts against the others' all_to_all_single: a gloo timeout, a hang over RCCL.)"""
    whole, n_per_rank = lopsided(world)
    matrix = plan_from_input(whole, ol.U32, 0, n_per_rank)["matrix"]
    whole_max = int(matrix[0, 0]) * 4
    over = matrix * 4 >= whole_max
    assert over.sum() == 1 and over[0, 0], matrix                                  # the precondition: one self-piece, nothing else
    assert sees_big(matrix, 0, 4, whole_max) and not any(sees_big(matrix, r, 4, whole_max) for r in range(1, world)), matrix
    piece_limit = 48002                                                             # 12000 keys a part
    assert int(matrix[0, 1]) > 12000, matrix                                        # rank 0 -> 1 goes in two parts at least
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(1, 1), (3, 1)], piece_limit, whole_max)
    for r in range(world):
        assert reports[r][0]["batches"] == 1 and reports[r][0]["a2a"] == 0


# ---- every rank agrees the pieces are big -------------------------------------------------------------------------------------

_S = 5000       # keys a part in the designed cases: PIECE_LIMIT = 4 _S + 2 bytes (the two odd bytes carry nothing)
_DESIGNED = {
    "world2-a": [[_S, _S - 1], [2 * _S + 1, 2 * _S + 2]],
    "world2-b": [[_S, 2 * _S], [3 * _S, 2 * _S]],
    "world3": [[2 * _S, _S - 1, _S + 1], [2 * _S, 2 * _S + 2, 2 * _S + 1], [3 * _S, 4 * _S - 1, 4 * _S - 2]],
}


@pytest.mark.parametrize("name", sorted(_DESIGNED))
def test_pieces_in_one_two_and_more_parts(tmp_path, name):
    """chunks = 1 with every rank over the limit by its own row and column: the grouped send / receive in parts.  The inputs are
    built for their count matrix, so the pieces between two ranks are cut in 1, 2, 3 and 4 parts, and they include exact
    multiples of a part, multiples plus one key and multiples minus one key (the two world-2 inputs together; world 3 alone).
    (one_exchange used to send a rank its own piece over the group as well: gloo's `Pair is not connected`.)"""
    whole, n_per_rank = designed(_DESIGNED[name], 7)
    world = len(n_per_rank)
    matrix = plan_from_input(whole, ol.U32, 0, n_per_rank)["matrix"]
    assert np.array_equal(matrix, np.asarray(_DESIGNED[name])), matrix             # the splitters fell where the input wants them
    piece_limit, whole_max = 4 * _S + 2, 8 * _S + 4
    assert all(sees_big(matrix, r, 4, whole_max) for r in range(world))
    off = [int(matrix[s, d]) for s in range(world) for d in range(world) if s != d]
    parts = sorted(parts_of(c, _S) for c in off)
    kinds = {(c + 1) % _S for c in off}            # 1: a multiple of a part, 2: a multiple plus one, 0: a multiple minus one
    if world == 3:
        assert parts == [1, 2, 2, 3, 3, 4] and kinds >= {0, 1, 2}
    else:
        assert (parts, kinds) == {"world2-a": ([1, 3], {0, 2}), "world2-b": ([2, 3], {1})}[name]
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(1, 1)], piece_limit, whole_max)
    for r in range(world):
        assert reports[r][0]["batches"] == 1 and len(reports[r][0]["ops"]) == sum(
            parts_of(matrix[r, p], _S) + parts_of(matrix[p, r], _S) for p in range(world) if p != r)


def test_designed_inputs_cover_every_part_count_at_world_two():
    off = [m[s][d] for name, m in _DESIGNED.items() if name.startswith("world2") for s in range(2) for d in range(2) if s != d]
    assert {parts_of(c, _S) for c in off} >= {1, 2, 3} and {(c + 1) % _S for c in off} >= {0, 1, 2}


# ---- key widths ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,order", [(ol.U8, 0), (ol.I16, 0), (ol.F32, 1), (ol.U64, 0)], ids=["u8", "i16", "f32-desc", "u64"])
def test_every_key_width_in_parts(tmp_path, dtype, order):
    """1, 2, 4 and 8 bytes a key (the exchange moves uint8 / uint8 pairs / int32 / int64 units) through the grouped exchange in
    parts and through the chunk pipeline, with a PIECE_LIMIT that is no multiple of the key size: a part is
    PIECE_LIMIT // size whole keys."""
    es = ol.DTYPE_SIZE[dtype]
    n_per_rank = [50000, 45001]
    whole = ol.splitmix_fill(sum(n_per_rank), dtype, 83 + dtype)
    piece_limit, whole_max = 10007, 20014
    assert piece_limit % es != 0 or es == 1
    matrix = plan_from_input(whole, dtype, order, n_per_rank)["matrix"]
    assert all(sees_big(matrix, r, es, whole_max) for r in range(2)), matrix
    assert min(int(matrix[0, 1]), int(matrix[1, 0])) > 2 * (piece_limit // es), matrix        # three parts at least, both ways
    run_case(tmp_path, whole, dtype, order, n_per_rank, [(1, 1), (3, 1)], piece_limit, whole_max)


# ---- pieces of no keys --------------------------------------------------------------------------------------------------------

def test_a_pair_of_ranks_that_exchanges_nothing(tmp_path):
    """World 3, ranks 0 and 2 hold none of each other's keys: no send and no receive is posted between them, in either path."""
    m = [[2 * _S, _S, 0], [_S, _S, _S], [0, _S, 2 * _S]]
    whole, n_per_rank = designed(m, 11)
    matrix = plan_from_input(whole, ol.U32, 0, n_per_rank)["matrix"]
    assert np.array_equal(matrix, np.asarray(m)), matrix
    piece_limit = 4 * (_S // 2) + 1                                                 # every piece that exists: two parts
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(1, 1), (3, 1)], piece_limit, 2 * piece_limit)
    for run in range(2):
        assert all(op[2] != 2 for op in reports[0][run]["ops"]) and all(op[2] != 0 for op in reports[2][run]["ops"])


def test_a_rank_with_an_empty_shard(tmp_path):
    """n_per_rank = [60000, 0]: rank 1 sends nothing and receives its half of rank 0's keys, in parts."""
    n_per_rank = [60000, 0]
    whole = ol.splitmix_fill(60000, ol.U32, 67)
    matrix = plan_from_input(whole, ol.U32, 0, n_per_rank)["matrix"]
    assert int(matrix[1].sum()) == 0 and int(matrix[0, 1]) > 25000, matrix
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(1, 1), (3, 1)], 40001, 80002)
    assert not [op for op in reports[0][0]["ops"] if op[0] == "recv"] and not [op for op in reports[1][0]["ops"] if op[0] == "send"]


# ---- the chunk pipeline's parts -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,n_per_rank", [(2, [70000, 61111]), (3, [50000, 64001, 47000])], ids=["world2", "world3"])
def test_chunk_pipeline_cuts_its_pieces_in_parts(tmp_path, world, n_per_rank):
    """chunks in (2, 4) x split_slices in (1, 3): a piece is (destination, sub-range, part of the split), and PIECE_LIMIT is low
    enough that the largest of them goes in three parts or more in every one of the four runs."""
    whole = ol.splitmix_fill(sum(n_per_rank), ol.U32, 43)
    runs = [(c, s) for c in (2, 4) for s in (1, 3)]
    piece_limit = 4001                                                              # 1000 keys a part
    for chunks, slices in runs:
        plan = plan_from_input(whole, ol.U32, 0, n_per_rank, chunks, slices)
        assert plan["slices"] == slices and plan["levels"] == 0
        off = [int(plan["pieces"][s, d].max()) for s in range(world) for d in range(world) if s != d]
        assert max(off) > 2 * 1000, (chunks, slices, off)
    run_case(tmp_path, whole, ol.U32, 0, n_per_rank, runs, piece_limit, 2 * piece_limit)


def test_chunk_pipeline_parts_meet_the_refined_split(tmp_path):
    """70 % of the keys share one top byte: that digit is divided by the next byte (the sliced split steps aside), the sub-ranges
    are cut over the refined bins, and their pieces go in parts.  Nothing that was refined is called even."""
    n_per_rank = [52000, 47003]
    whole = _skew(ol.splitmix_fill(sum(n_per_rank), ol.U32, 19), ol.U32, 70)
    plan = plan_from_input(whole, ol.U32, 0, n_per_rank, 4, 3)
    assert plan["levels"] == 1 and plan["slices"] == 1
    assert max(int(plan["pieces"][0, 1].max()), int(plan["pieces"][1, 0].max())) > 2 * 1000
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(4, 3), (1, 1)], 4001, 8002)
    for r in range(2):
        for run in range(2):
            assert reports[r][run]["evens"] and not any(even for _, even in reports[r][run]["evens"])


# ---- the defaults -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lopsided", "world3"])
def test_default_limits_leave_small_inputs_to_all_to_all_single(tmp_path, name):
    """PIECE_LIMIT and WHOLE_PIECE_MAX as the module defines them: the inputs of the cases above are exchanged by ONE
    all_to_all_single a rank and no send or receive -- what distributed_sort did before the limits had names."""
    assert multi.PIECE_LIMIT == 1 << 30 and multi.WHOLE_PIECE_MAX == 1 << 31
    whole, n_per_rank = lopsided(2) if name == "lopsided" else designed(_DESIGNED["world3"], 7)
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(1, 1)])
    for rep in reports:
        assert rep[0]["a2a"] == 1 and rep[0]["batches"] == 0 and not rep[0]["ops"]


# ---- the even-digits hint -----------------------------------------------------------------------------------------------------

def slot_cap(mean):
    """slot_cap_for of csrc/rsx_route_levels.hpp: the keys a level-1 slot holds when the mean bucket has `mean` keys -- 1.25 times the mean, at
    least seven standard deviations of an even spread above it, rounded up to 256."""
    r = int(np.floor(np.sqrt(mean)))
    while (r + 1) * (r + 1) <= mean:
        r += 1
    while r * r > mean:
        r -= 1
    need = max(mean + mean // 4, mean + 7 * (r + 1) + 8)
    return (need + 255) // 256 * 256


def test_bins_are_even_stays_below_the_level_one_slot():
    """The hint turns the sample's own level-1 test off, and the counts are exact: a bin above its slot loses the attempt for
    certain.  So it is never granted where a bin exceeds slot_cap_for(mean) -- nor 1.25 times the mean of any number of bins --,
    it is granted for uniform counts, not for a single bin, and not after a refinement."""
    rng = np.random.default_rng(17)
    granted = refused = 0
    for mean in (300, 2000, 65536, 1 << 21):
        for factor in np.r_[np.linspace(1.0, 1.6, 61), 1.2, 1.25, 1.5]:
            for nbins in (256, 128, 86, 2):
                c = rng.poisson(mean, nbins).astype(np.uint64)
                c[int(rng.integers(nbins))] = int(factor * mean)
                even = multi.bins_are_even(c, 0)
                if even:
                    granted += 1
                    assert float(c.max()) <= 1.25 * float(c.mean()), (mean, factor, nbins)
                    if nbins == 256:
                        assert int(c.max()) <= slot_cap(int(c.sum()) >> 8), (mean, factor)
                else:
                    refused += 1
                    assert float(c.max()) > 1.15 * float(c.mean()), (mean, factor, nbins)      # (not refused for nothing either)
                assert not multi.bins_are_even(c, 1)
    assert granted > 100 and refused > 100
    assert multi.bins_are_even(np.full(256, 1000, dtype=np.uint64), 0)
    assert multi.bins_are_even(np.full(2, 7, dtype=np.uint64), 0)
    assert not multi.bins_are_even(np.full(256, 1000, dtype=np.uint64), 1)           # after a refinement
    assert not multi.bins_are_even(np.asarray([123456], dtype=np.uint64), 0)         # a single bin
    assert not multi.bins_are_even(np.zeros(0, dtype=np.uint64), 0)
    c = np.full(256, 1000.0)
    c[9] = 1.3 * c.sum() / 256                                                       # between the old 1.5 and the slot's 1.25
    assert not multi.bins_are_even(c, 0)


@pytest.mark.parametrize("name", ["uniform", "lopsided"])
def test_the_engine_is_told_what_bins_are_even_says(tmp_path, name):
    """Two ranks, one exchange, one local sort a rank: the `even` the engine is given is bins_are_even of the global counts of the
    top digits that rank owns.  Uniform keys: both ranks are told yes; the lopsided input: rank 1 owns digits of two densities."""
    if name == "uniform":
        n_per_rank = [90000, 80001]
        whole = ol.splitmix_fill(sum(n_per_rank), ol.U32, 5)
    else:
        whole, n_per_rank = lopsided(2)
    total = np.bincount((whole >> np.uint32(24)).astype(np.int64), minlength=256).astype(np.uint64)
    lut = multi.choose_splitters(total, 2).astype(np.int64)
    want = [bool(multi.bins_are_even(total[lut == r], 0)) for r in range(2)]
    assert want == ([True, True] if name == "uniform" else [True, False])
    reports = run_case(tmp_path, whole, ol.U32, 0, n_per_rank, [(1, 1)])
    for r in range(2):
        assert reports[r][0]["levels"] == 0
        assert reports[r][0]["evens"] == [[sum(reports[r][0]["recv_counts"]), want[r]]]
