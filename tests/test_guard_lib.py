"""CPU checks of tests/guard_lib.py: the guard bands catch a write one byte before and one byte after the buffer, report where,
and the restated slot geometry gives the numbers rsx_route_levels.hpp's comments and tests/test_gpu_bounds.py rely on.  No GPU: the helper
runs on CPU tensors here (the same layout and comparison as on the device)."""
import numpy as np
import pytest

import guard_lib as gl

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("dtype,residue", [(torch.int32, 0), (torch.int32, 4), (torch.int64, 8), (torch.int64, 72),
                                           (torch.float32, 68)])
def test_guard_layout_and_residue(dtype, residue):
    g = gl.guarded(1001, dtype, residue, guard=4096, device="cpu")
    assert g.t.numel() == 1001 and g.t.dtype == dtype and g.t.is_contiguous()
    assert g.t.data_ptr() % 256 == residue
    assert g.start >= 4096 and g.raw.numel() - g.end >= 4096
    assert g.damage() == []
    g.t.fill_(-1)                   # the buffer itself is the caller's to write
    g.check("whole buffer written")
    rows = np.arange(1001 * g.esize, dtype=np.uint8).reshape(1001, g.esize)     # (records: any shape of the buffer's bytes)
    g.load(rows)
    assert np.array_equal(g.raw[g.start:g.end].numpy(), rows.reshape(-1))
    g.check("loaded")


@pytest.mark.parametrize("residue", [0, 8, 72])
def test_guard_catches_one_byte_before_and_one_after(residue):
    g = gl.guarded(4097, torch.int64, residue, guard=1 << 12, device="cpu")
    g.t.fill_(0)
    g.raw[g.start - 1] ^= 1         # one byte before the buffer
    assert g.damage() == [("front", -1, -1)]
    with pytest.raises(gl.GuardDamage, match=r"front guard, bytes -1 \.\. -1"):
        g.check("one before")
    g.raw[g.start - 1] ^= 1
    g.check("restored")
    g.raw[g.end] ^= 0x80            # one byte after it
    assert g.damage() == [("back", 0, 0)]
    with pytest.raises(gl.GuardDamage, match=r"back guard, bytes \+0 \.\. \+0"):
        g.check("one after")
    # a run that starts 40 bytes before the buffer's start and one that ends at the last byte of the back guard
    g.raw[g.start - 40:g.start - 3] = 0
    g.raw[g.raw.numel() - 1] ^= 0xFF
    g.raw[g.end + 5] ^= 0x10
    assert g.damage() == [("front", -40, -4), ("back", 0, g.raw.numel() - 1 - g.end)]


def test_guard_pattern_is_the_seeded_splitmix_stream():
    """Both guards hold the low bytes of the splitmix64 sequence of the guard seed (the device fills the same sequence), never
    a constant a zeroed or copied run could match."""
    import oracle_lib as ol
    g = gl.guarded(100, torch.int32, 4, guard=512, device="cpu")
    want = ol.splitmix_fill(g.raw.numel(), ol.U8, gl.GUARD_SEED)
    assert np.array_equal(g.front.numpy(), want[:g.start])
    assert np.array_equal(g.back.numpy(), want[g.end:])
    assert len(np.unique(g.front.numpy())) > 200


def test_check_all_names_every_damaged_buffer():
    a = gl.guarded(10, torch.int32, 0, guard=64, device="cpu")
    b = gl.guarded(10, torch.int32, 4, guard=64, device="cpu")
    a.check("a")
    a.raw[a.end + 63] ^= 1
    b.raw[0] ^= 1
    with pytest.raises(gl.GuardDamage) as e:
        gl.check_all(("src", a), ("aux", b))
    assert "src:" in str(e.value) and "aux:" in str(e.value) and "+63" in str(e.value)


def test_bad_layouts_are_refused():
    with pytest.raises(ValueError):
        gl.Guarded(10, torch.int32, 0, 64, device="cpu")        # not whole elements
    with pytest.raises(ValueError):
        gl.Guarded(16, torch.int64, 4, 64, device="cpu")        # a residue that is not element-aligned
    with pytest.raises(ValueError):
        gl.Guarded(16, torch.int32, 0, 0, device="cpu")


def test_restated_slot_geometry():
    """The numbers test_gpu_bounds.py sizes its cases and guards by."""
    # u32, 64 Mi - 16 Ki keys: slots of 344064 keys (an odd number of 64 KiB), 195 of them fill aux to its last key
    n = 67092480
    cap1, lo = gl.level1_geometry(n, 4)
    assert (cap1, lo) == (344064, 195) and lo * cap1 == n
    assert gl.level1_slot_overrun(n, 4) == cap1 * 4
    # slot_cap_for at a small mean: mean + 7 sigma wins over 1.25 x
    assert gl.slot_cap_for(200) == 512 and gl.slot_cap_for(65536) == 81920
    # 8-byte keys below 2^40, 3 * 2^23 + 4096: the narrow level-1 form fits aux by default, and RSX_CAP1_PAD_KIB makes it overrun
    n = 3 * (1 << 23) + 4096
    assert gl.narrow1_overrun(n) == 0
    assert gl.narrow1_overrun(n, pad_kib=512) == 8355840            # ~ 8 MiB
    assert gl.narrow1_overrun(n, pad_kib=1024) == 75464704          # ~ 72 MiB
    assert gl.level1_geometry(n, 8, pad_kib=512) == (204800, 122)
    # RSX_NO_ODD_STRIDE=1: 1.25 means rounded to 256 keys only (slots of a MiB and more: 2^25 + 4096 8-byte keys)
    n = (1 << 25) + 4096
    assert gl.level1_geometry(n, 8, odd_stride=False) == (164096, 204)
    assert gl.level1_geometry(n, 8) == (172032, 195)
