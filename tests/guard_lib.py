"""Guard bands around the buffers a test hands to the library: where does the library write?

TEST INFRASTRUCTURE ONLY (tests/test_gpu_bounds.py, tests/test_guard_lib.py).  A result that is right says nothing about the
memory around it: a slot one past the last, a dump area or an atom rounded the wrong way can land in the caller's neighbouring
allocation and every result-only test still passes.  `Guarded` allocates one uint8 tensor laid out as

    front guard | buffer | back guard

fills both guards with a seeded splitmix64 pattern (its own seed, so that a stray copy of keys cannot match it by chance), hands
out a typed view of the buffer that starts at a chosen residue mod 256, and `check()` compares both guards with the copies kept
when they were filled.

Also here: the slot geometry of the sort without a histogram restated from radix_sorting_amd/csrc/rsx_route_levels.hpp (slot_cap_for,
level1_slot_cap, blind_enqueue's `lo`, the condition of the 8-byte narrow level-1 form), so that a test can size its guards
above the largest overrun a wrong slot could make before anything is launched.
"""
import math

import numpy as np

import oracle_lib as ol

GUARD_SEED = 0x6A09E667F3BCC908     # (no test draws keys from this seed)
ALIGN = 256     # residues are taken mod this: the tests use 0, one element, and 64 + one element


def _torch():
    import torch
    return torch


class GuardDamage(AssertionError):
    pass


class Guarded:
    """One allocation: `guard` bytes (at least) | `nbytes` of buffer starting at `residue` mod 256 | `guard` bytes.

    `dtype`: the torch dtype of the view `.t` (a contiguous tensor of nbytes / element size elements).  The buffer's own bytes are
    filled with the pattern too (tests then copy their data in).  `device`: "cuda" fills with rsx_fill_splitmix_device, "cpu"
    with the oracle's host restatement of the same generator (the helper's own tests run on CPU tensors)."""

    def __init__(self, nbytes, dtype, residue=0, guard=1 << 20, device="cuda", seed=GUARD_SEED):
        torch = _torch()
        esize = torch.empty(0, dtype=dtype).element_size()
        if nbytes % esize or residue % esize or not 0 <= residue < ALIGN:
            raise ValueError("buffer of %d bytes at residue %d: not whole %d-byte elements" % (nbytes, residue, esize))
        if guard <= 0:
            raise ValueError("a guard band needs at least one byte")
        self.nbytes, self.residue, self.guard, self.esize = nbytes, residue, guard, esize
        total = guard + ALIGN + nbytes + guard
        self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        self.start = guard + ((residue - (base + guard)) % ALIGN)
        self.end = self.start + nbytes
        assert (base + self.start) % ALIGN == residue
        assert self.start % esize == 0, "the allocation itself is not element-aligned"
        self._fill(seed)
        self.front_saved = self.raw[:self.start].clone()
        self.back_saved = self.raw[self.end:].clone()
        self.t = self.raw[self.start:self.end].view(dtype)

    def _fill(self, seed):
        if self.raw.is_cuda:
            import radix_sorting_amd as rsa
            rsa.fill_splitmix(self.raw, seed)
            _torch().cuda.synchronize()
        else:
            pat = ol.splitmix_fill(self.raw.numel(), ol.U8, seed)
            self.raw.copy_(_torch().from_numpy(pat))

    @property
    def front(self):
        return self.raw[:self.start]

    @property
    def back(self):
        return self.raw[self.end:]

    def load(self, bits):
        """Copy a numpy array of any dtype and shape that holds exactly the buffer's bytes into it."""
        torch = _torch()
        a = np.ascontiguousarray(bits)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        self.raw[self.start:self.end].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        return self.t

    def damage(self):
        """[(guard, first, last)] of each guard that differs from its copy: byte offsets of the first and last differing byte,
        the front guard's relative to the buffer's START (negative), the back guard's relative to its END (0 = the first byte
        behind the buffer).  Empty when both are intact."""
        torch = _torch()
        if self.raw.is_cuda:
            torch.cuda.synchronize()
        out = []
        for name, now, saved, origin in (("front", self.front, self.front_saved, -self.start), ("back", self.back, self.back_saved, 0)):
            if torch.equal(now, saved):
                continue
            idx = torch.nonzero(now != saved).flatten()
            out.append((name, int(idx[0]) + origin, int(idx[-1]) + origin))
        return out

    def check(self, what=""):
        bad = self.damage()
        if bad:
            raise GuardDamage("%s: written outside the buffer of %d bytes (residue %d): %s" % (
                what, self.nbytes, self.residue,
                "; ".join("%s guard, bytes %+d .. %+d from the buffer's %s" % (g, a, b, "start" if g == "front" else "end")
                          for g, a, b in bad)))


def guarded(n, dtype, residue=0, guard=1 << 20, device="cuda"):
    """Guarded buffer of n elements of a torch dtype."""
    torch = _torch()
    return Guarded(n * torch.empty(0, dtype=dtype).element_size(), dtype, residue, guard, device)


def check_all(*pairs):
    """check() every (name, Guarded) pair; one error names every damaged buffer."""
    msgs = []
    for name, g in pairs:
        try:
            g.check(name)
        except GuardDamage as e:
            msgs.append(str(e))
    if msgs:
        raise GuardDamage("\n".join(msgs))


# ---- the slot geometry of a sort without a histogram (rsx_route_levels.hpp), restated ---------------------------------------------------

def slot_cap_for(mean):
    """rsx_route_levels.hpp slot_cap_for: 1.25 x the mean and at least mean + 7 standard deviations + 8, rounded up to 256 keys."""
    r = math.isqrt(mean)
    need = max(mean + mean // 4, mean + 7 * (r + 1) + 8)
    return (need + 255) // 256 * 256


def level1_slot_cap(mean, ksize, pad_kib=0, odd_stride=True):
    """rsx_route_levels.hpp level1_slot_cap<KT>: slots of a MiB and more an odd number of 64 KiB apart; RSX_CAP1_PAD_KIB adds pad_kib KiB."""
    cap1 = slot_cap_for(mean) + pad_kib * (1024 // ksize)
    if odd_stride and cap1 * ksize >= (1 << 20):
        unit = 65536 // ksize
        cap1 = (cap1 + unit - 1) // unit * unit
        if (cap1 // unit) % 2 == 0:
            cap1 += unit
    return cap1


def level1_geometry(n, ksize, pad_kib=0, odd_stride=True):
    """(cap1, lo): the level-1 slot capacity and how many of the 256 slots lie in the caller's second buffer (blind_enqueue,
    keys-only; slot d < lo at aux + d * cap1 keys)."""
    cap1 = level1_slot_cap(n >> 8, ksize, pad_kib, odd_stride)
    return cap1, min(n // cap1, 255)


def pairs_level1_geometry(n):
    """(cap1, lo) of pairs_blind_enqueue (4-byte keys: slot_cap_for without the odd stride)."""
    cap1 = slot_cap_for(n >> 8)
    return cap1, min(n // cap1, 255)


def narrow1_bytes(n, ksize=8, pad_kib=0, odd_stride=True):
    """Bytes the narrow level-1 form of 8-byte keys writes from aux: 256 slots of cap1 four-byte places."""
    cap1, _ = level1_geometry(n, ksize, pad_kib, odd_stride)
    return 256 * cap1 * 4


def narrow1_overrun(n, ksize=8, pad_kib=0, odd_stride=True):
    """How far past the end of aux (n keys) the narrow level-1 form would write if it were chosen: 0 when it fits."""
    return max(0, narrow1_bytes(n, ksize, pad_kib, odd_stride) - n * ksize)


def level1_slot_overrun(n, ksize, pad_kib=0, odd_stride=True):
    """The bytes one slot more than blind_enqueue's `lo` would put past the end of aux: what a guard of a keys-only case of the
    sort without a histogram must exceed (one slot past the last, the largest single misplacement of a slot base)."""
    cap1, lo = level1_geometry(n, ksize, pad_kib, odd_stride)
    return max(0, (lo + 1) * cap1 * ksize - n * ksize)
