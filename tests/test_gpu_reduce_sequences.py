"""What one call leaves for the next, with rsx_sort_reduce_device among its neighbours on ONE context and stream:
reduce (cells) -> radix_sort_group -> reduce (sort) -> radix_sort_pairs -> radix_sort_unique -> reduce (cells).  The calls share
the context's records of heads and chunks, its copies of the keys and its payload buffers; each step is checked against the
oracle, so that a table, a record or a flag left behind by one step shows in the next."""
import numpy as np
import pytest

import group_lib as gr
import oracle_lib as ol
import radix_sorting_amd as rsa
import reduce_lib as rl
import unique_lib as ul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


def dev(bits, dt):
    a = np.ascontiguousarray(bits, dtype=ol.NP_BITS[dt])
    return torch.from_numpy(a.view(ul.SIGNED[ol.DTYPE_SIZE[dt]]).copy()).cuda()


def reduce_step(k, dt, v, vdt, route, what, order=ol.ASC):
    want = rl.want_reduce(rl.groups(k, dt, order), v, vdt)
    ok, cn, sm, mn, mx, info = rsa.radix_sort_reduce(dev(k, dt), dev(v, vdt), dtype=dt, val_dtype=vdt, order=order, min=True, max=True, counts=True)
    torch.cuda.synchronize()
    assert info.route == route, (what, info.route)
    got = (ok.cpu().numpy().view(ol.NP_BITS[dt]), cn.cpu().numpy().view(np.uint32).astype(np.uint64), sm.cpu().numpy().view(np.uint64),
           mn.cpu().numpy().view(ol.NP_BITS[vdt]), mx.cpu().numpy().view(ol.NP_BITS[vdt]))
    for name, g, w in zip(("keys", "counts", "sum", "min", "max"), got, want):
        assert np.array_equal(g, w), "%s: %s differs from the oracle" % (what, name)


def test_reduce_among_its_neighbours():
    rsa.reload_env()
    torch.cuda.synchronize()
    n = (1 << 18) + 11
    cells = ol.splitmix_fill(n, ol.U32, 9601, 0x00F0F00F)
    wide = ol.splitmix_fill(n, ol.U32, 9602)
    wide[::3] = wide[0]                                  # (a third of the elements in one long run of the sorted array)
    v32, v64 = rl.small_ints(n, ol.F32, 9603), rl.small_ints(n, ol.I64, 9604)
    # 1. reduce on the cells route
    reduce_step(cells, ol.U32, v32, ol.F32, rsa.REDUCE_CELLS_LDS, "step 1, cells")
    # 2. radix_sort_group on the sort route (counts and first indices): the heads' records, the keys' copies, the index halves
    inv, k, cn, fi, info = rsa.radix_sort_group(dev(wide, ol.U32), dtype=ol.U32, keys=True, counts=True, first=True)
    torch.cuda.synchronize()
    assert info.route == rsa.GROUP_SORT
    want = gr.want_group(wide, ol.U32)
    for name, t, w in zip(("inverse", "keys", "counts", "first"), (inv, k, cn, fi), want):
        g = t.cpu().numpy().view(np.uint32)
        assert np.array_equal(g if name == "keys" else g.astype(np.uint64), w), "step 2, group: " + name
    # 3. reduce on the sort route, 8-byte values in the halves that held 4-byte indices
    reduce_step(wide, ol.U32, v64, ol.I64, rsa.REDUCE_SORT, "step 3, sort", order=ol.DESC)
    # 4. a key + payload sort of the caller's own buffers
    pk, pv = dev(wide, ol.U32), dev(v32, ol.F32)
    rk, rv, pinfo = rsa.radix_sort_pairs(pk, torch.zeros_like(pk), pv, torch.zeros_like(pv), dtype=ol.U32)
    torch.cuda.synchronize()
    perm = ol.stable_argsort_by_kdf(wide, ol.U32)
    assert np.array_equal(rk.cpu().numpy().view(np.uint32), wide[perm]) and np.array_equal(rv.cpu().numpy().view(np.uint32), v32[perm])
    # 5. radix_sort_unique over a bitmap: the chunk records where the tile records were
    uk = dev(cells, ol.U32)
    res, ucn, uinfo = rsa.radix_sort_unique(uk, torch.zeros_like(uk), dtype=ol.U32, counts=torch.zeros(n, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    wk, wc = ul.want_unique(cells, ol.U32)
    assert np.array_equal(res.cpu().numpy().view(np.uint32), wk) and np.array_equal(ucn.cpu().numpy().view(np.uint32).astype(np.uint64), wc)
    # 6. reduce on the cells route again, other values and the other order: the table is made anew
    reduce_step(cells, ol.U32, rl.small_ints(n, ol.U64, 9605), ol.U64, rsa.REDUCE_CELLS_LDS, "step 6, cells", order=ol.DESC)
    # ... and once more on the sort route with the keys in order: no copy, the records of the tiles alone
    reduce_step(np.sort(wide), ol.U32, v32, ol.F32, rsa.REDUCE_SORT, "step 7, sorted input")
