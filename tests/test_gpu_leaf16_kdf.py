"""The two-byte leaves' write-out inverts the key derivation ONCE per leaf (kdf_invert_below, csrc/rsx_kernels.hpp): a leaf's
keys share the slot's two MSB digits and everything above them, the top bit among them, so the sign test of kdf_invert has one
outcome per leaf and a key is the leaf's inverted upper part xor its low bits.  That is only true if the top bit really comes
from what the leaf takes as shared -- the slot's level-1 digit, or the first key's bits above it when the keys' top bits are
constant (shift1 + 8 < 32) -- and it is the signed and float derivations, in both orders, that tell a wrong sign from a right
one: for floats the two halves of the leaves invert differently.

Everything goes through rsa.radix_sort at the sizes at which the library itself picks each kernel (nothing lowered), is
compared bit for bit with the oracle and must report route 5 (no histogram, two MSB passes into two-byte slots, leaves):
rsx_leaf16_kernel in both shapes (2560 and 5120 values), rsx_leaf16w_kernel (4 * 10^7 keys), rsx_leaf16q_kernel (10^7 keys) and
the counting leaves (RSX_FORCE_LEAFC, as tests/test_gpu_routes.py sets it).  The u32 cases at 128 Mi + 8 and 160 Mi + 5 keys
(mean slots of 2048 and 2560 values) are there for the leaves' two ways through count and place: a wave whose vectors all lie
inside the slot's front goes without predicates, the vectors at the front's ragged end and in the slot's back go with them --
every slot of a real sort has both.

The oracle needs one to three seconds per case on one host core.
"""
import numpy as np
import pytest

import oracle_lib as ol
import radix_sorting_amd as rsa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MI = 1 << 20
N_2560 = 104 * MI + 77     # slots of 2560 values: rsx_leaf16_kernel<u32, Leaf16Cfg<128, 2560, 8, 11>>
N_5120 = 136 * MI + 31     # slots of 5120 values: rsx_leaf16_kernel<u32, Leaf16Cfg<256, 5120, 8, 12>>, bench.py's instantiation
ORDERS = [ol.ASC, ol.DESC]
ORDER_IDS = ["asc", "desc"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    rsa.require_gpu()


@pytest.fixture(autouse=True)
def _fresh_routes():
    rsa.reload_env()     # (no back-off from an earlier attempt that was called off: the route is asserted)
    yield
    torch.cuda.empty_cache()


_BITS = {}


def _random_bits(n, seed, mask=0xFFFFFFFF):
    """Random 32-bit patterns, generated once per (size, seed, mask) and shared by the cases that reinterpret them (read-only)."""
    key = (n, seed, mask)
    if key not in _BITS:
        _BITS.clear()    # (one array of this size at a time)
        a = ol.splitmix_fill(n, ol.U32, seed, mask)
        a.setflags(write=False)
        _BITS[key] = a
    return _BITS[key]


def _sort_and_compare(a, dt, order, what):
    want, want_aux, winfo = ol.oracle_sort(a, dt, order)
    src = torch.from_numpy(np.array(a, copy=True).view(np.int32)).cuda()
    aux = torch.full_like(src, 0x5A5A5A5A)
    res, info = rsa.radix_sort(src, aux, dtype=dt, order=order)
    torch.cuda.synchronize()
    assert info.hybrid == 5, (what, info.hybrid)
    assert info.result_in_aux == want_aux, what
    assert info.kept_columns() == list(winfo.cols[:winfo.ncols]), what
    got = res.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), what
    return info


@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("dt", [ol.I32, ol.F32], ids=["i32", "f32"])
@pytest.mark.parametrize("n", [N_2560, N_5120], ids=["2560-value shape", "5120-value shape"])
def test_sign_from_the_slots_level1_digit(n, dt, order):
    """Random bit patterns: the top bit is the top bit of the level-1 digit, half of the leaves have it set and half clear."""
    a = _random_bits(n, 7100 + (n >> 20))
    _sort_and_compare(a, dt, order, ("sign in the slot", n, dt, order))


@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("dt", [ol.I32, ol.F32], ids=["i32", "f32"])
@pytest.mark.parametrize("mask,base", [(0x1FFFFFFF, 0xE0000000), (0x07FFFFFF, 0x18000000)], ids=["top bits 111", "top bits 00011"])
def test_sign_from_the_bits_above_the_level1_digit(mask, base, dt, order):
    """Constant top bits: the MSB digits move down (shift1 + 8 < 32) and the top bit every key shares comes from the first key."""
    a = np.ascontiguousarray(_random_bits(N_5120, 7200, mask) | np.uint32(base))
    _sort_and_compare(a, dt, order, ("sign above the digits", hex(base), dt, order))


@pytest.mark.parametrize("dt,order", [(ol.F32, ol.DESC), (ol.I32, ol.ASC)], ids=["f32 desc", "i32 asc"])
@pytest.mark.parametrize("n", [40000000, 10000000], ids=["a wave per leaf", "a row per leaf"])
def test_sign_through_the_wave_and_row_kernels(n, dt, order):
    a = _random_bits(n, 7300 + n // 10000000)
    _sort_and_compare(a, dt, order, ("small slots", n, dt, order))


def test_sign_through_the_counting_leaves(monkeypatch):
    monkeypatch.setenv("RSX_FORCE_LEAFC", "1")
    a = _random_bits(160 * MI + 77, 7400)
    _sort_and_compare(a, ol.F32, ol.DESC, "counting leaves, f32 desc")


@pytest.mark.parametrize("n", [128 * MI + 8, 160 * MI + 5], ids=["mean slot 2048", "mean slot 2560"])
def test_u32_whole_and_straddling_vectors(n):
    a = _random_bits(n, 7500 + (n >> 20))
    _sort_and_compare(a, ol.U32, ol.ASC, ("u32", n))
