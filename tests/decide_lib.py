"""Inputs one key away from the other answer of the library's two decisions (radix_sort.hpp:60-70): is the input sorted already,
and which byte columns vary.

TEST INFRASTRUCTURE ONLY (as oracle_lib.py; numpy, no torch, no GPU): imported by tests/test_decide_lib_cpu.py, which proves with
the reference restatement alone that every input made here does what tests/test_gpu_decisions.py assumes of it, by that module,
and by tests/test_gpu_logroute.py for the Zipf-like generator.

    positions   where a lone descent has to be put so that it falls on every seam of the kernels that look for one: the 16-byte
                vectors (VEC = 16 / key bytes elements), the 64 lanes of a wave, the 1024 and 2048 threads of a sweep, the scalar
                head in front of the first aligned element, the last full vector and the tail behind it, the places a sample reads;
    one_descent a sorted array with exactly ONE descent, and its sorted order in O(n): the sorted base with one element moved;
    one_stray   an array in which one byte column of the derived keys is constant except for one bit of one key.

Everything works on BIT PATTERNS through oracle_lib.kdf_keys / kdf_inverse: float keys include negative values, both zeros and
NaN patterns, and nothing here compares floats.  A case is described by its `patches` ((index, bit pattern) pairs applied to
the base) and its `pieces` (slices of the sorted base and single values whose concatenation is the expected result), so that
the GPU module applies the very description the CPU module has checked -- on the device, without sorting anything itself.
"""
import collections

import numpy as np

import oracle_lib as ol

_M64 = (1 << 64) - 1
SAMPLE_KEYS = 128      # keys a sample reads at each of its 64 places (8 per thread, 16 threads)
SAMPLE_PLACES = 64
RANDOM_POSITIONS = 16


def splitmix64(seed, count):
    """`count` values of the splitmix64 sequence from `seed` (plain Python integers)."""
    out, x = [], seed & _M64
    for _ in range(count):
        x = (x + 0x9E3779B97F4A7C15) & _M64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        out.append(z ^ (z >> 31))
    return out


def head_elems_of(offset_elems, key_bytes):
    """Elements in front of the first 16-byte-aligned one when the array starts `offset_elems` elements behind an aligned address."""
    return ((-offset_elems * key_bytes) % 16) // key_bytes


def _named_positions(n, key_bytes, head_elems, sampled):
    """The boundary positions by name, unclipped (values outside [0, n-2] are out of range for this n)."""
    vec = 16 // key_bytes
    sweep = 2048 * vec
    rel = [0, 1, vec - 2, vec - 1, vec, 64 * vec - 1, 64 * vec, 1024 * vec - 1, 1024 * vec, sweep - 1, sweep]
    m = 1
    while m * sweep < n:          # every power of two below n / (2048 VEC)
        rel.append(m * sweep - 1)
        m *= 2
    named = [head_elems + r for r in rel]                 # counted from the first aligned element
    if head_elems:
        named += rel                                      # ... and the same shifted by -head_elems: counted from the array's start
        named.append(head_elems - 1)                      # the last element of the scalar head against the first aligned one
    full = (n - head_elems) // vec if n > head_elems else 0
    if full:
        named += [head_elems + full * vec - 1, head_elems + full * vec - 2]   # the last full vector's last element: behind it, in front of it
    named += [n - 3, n - 2]
    if sampled:
        step = (n - SAMPLE_KEYS) // (SAMPLE_PLACES - 1) if n >= SAMPLE_KEYS else 0
        named += [6, 7, 8, SAMPLE_KEYS - 1, SAMPLE_KEYS]  # inside thread 0's keys, between threads, behind the first place
        named += [step - 1, step, step + 7, step + 8]     # the second place
    return named


def positions(n, key_bytes, head_elems=0, sampled=False, rand=RANDOM_POSITIONS, seed=None):
    """Sorted descent positions p (a descent between elements p and p + 1) for an array of n keys of `key_bytes` bytes whose first
    16-byte-aligned element has `head_elems` elements in front of it.  `sampled`: also the places of the routes that trust a
    sample.  `rand`: seeded random positions on top (0: the boundary subset alone)."""
    assert n >= 2 and key_bytes in (1, 2, 4, 8) and 0 <= head_elems < 16 // key_bytes
    named = _named_positions(n, key_bytes, head_elems, sampled)
    out = set(min(max(p, 0), n - 2) for p in named)
    if rand:
        s = (0xD0C1DE + 1000003 * n + 31 * key_bytes + head_elems) if seed is None else seed
        out.update(z % (n - 1) for z in splitmix64(s, rand))
    out = sorted(out)
    # nothing named and in range may be missing
    missing = [p for p in _named_positions(n, key_bytes, head_elems, sampled) if 0 <= p <= n - 2 and p not in out]
    assert not missing, missing
    assert out[0] >= 0 and out[-1] <= n - 2
    return out


def stray_positions(n, key_bytes, sampled=False):
    """Sorted element positions for the one key that differs in an otherwise constant column."""
    vec = 16 // key_bytes
    named = [0, 1, 63, 64, 64 * vec - 1, 2048 * vec - 1, 2048 * vec, n // 2, n - 1]
    if sampled:
        step = (n - SAMPLE_KEYS) // (SAMPLE_PLACES - 1) if n >= SAMPLE_KEYS else 0
        named += [6, 7, 8, SAMPLE_KEYS - 1, SAMPLE_KEYS, step - 1, step, step + 7, step + 8]
    out = sorted(set(min(max(p, 0), n - 1) for p in named))
    assert all(p in out for p in named if 0 <= p < n)
    return out


# ---- the derived keys and back ------------------------------------------------------------------------------------------
def kdf_inverse(keys, dtype, order=ol.ASC):
    """The bit patterns whose derived keys (oracle_lib.kdf_keys) are `keys`."""
    ut = ol.NP_BITS[dtype]
    k = np.asarray(keys, dtype=ut)
    if order == ol.DESC:
        k = ~k
    nb = ol.DTYPE_SIZE[dtype] * 8
    top = ut(1 << (nb - 1))
    if dtype in (ol.I8, ol.I16, ol.I32, ol.I64):
        u = k ^ top
    elif dtype in (ol.F32, ol.F64):
        was_neg = (k >> ut(nb - 1)) == 0          # negative floats are complemented: their images have the top bit clear
        u = np.where(was_neg, ~k, k ^ top)
    else:
        u = k.copy()
    return u.astype(ut)


def sort_by_kdf(bits, dtype, order=ol.ASC):
    """The stable sort of `bits` by derived key (equal derived keys are equal bit patterns: the order among them does not show)."""
    return kdf_inverse(np.sort(ol.kdf_keys(bits, dtype, order)), dtype, order)


def zipf_like(n, seed, bmax=40):
    """SURVEY.md 8d cfg 3 (iv), integer-only: key = 2^(b-1) + (r & (2^(b-1) - 1)), b = 1 + (r >> 58) % bmax, r = splitmix64."""
    r = ol.splitmix_fill(n, ol.U64, seed)
    b = np.uint64(1) + ((r >> np.uint64(58)) % np.uint64(bmax))
    one = np.uint64(1)
    return (one << (b - one)) + (r & ((one << (b - one)) - one))


_FLOAT_EDGES = {ol.F32: [0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001],
                ol.F64: [0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000000,
                         0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x8000000000000001]}


def sorted_base(n, dtype, order, seed):
    """n keys sorted in KDF order: splitmix bits over the whole width (every column varies), a quarter of them twice (duplicates,
    no constant halves), floats with both zeros, NaNs of both signs, infinities and denormals; for n < 8 distinct keys."""
    ut = ol.NP_BITS[dtype]
    if n < 8:
        a = ol.splitmix_fill(64, dtype, seed)
        a = a[np.sort(np.unique(a, return_index=True)[1])][:n]      # the first n distinct ones
        assert a.size == n
    else:
        fresh = n - n // 4
        a = ol.splitmix_fill(fresh, dtype, seed)
        a = np.concatenate([a, a[: n // 4]])
        if dtype in _FLOAT_EDGES and n >= 64:
            a[1:9] = np.array(_FLOAT_EDGES[dtype], dtype=ut)
    return sort_by_kdf(a, dtype, order)


# ---- one descent --------------------------------------------------------------------------------------------------------
# patches: [(index, value)] on the base; pieces: [("s", a, b) -> sorted_base[a:b] | ("v", value)] whose concatenation is the result
Case = collections.namedtuple("Case", "p kind patches pieces")


class NoDescent(ValueError):
    pass


def descent_case(sorted_bits, dtype, order, p):
    """The description of one_descent's array, in O(1).  `kind`: "raise" (p < n / 2: element p becomes the array's KDF-maximum)
    or "lower" (element p + 1 becomes the KDF-minimum).  Arrays of two or three keys, where raising element n - 2 would put it
    beside the maximum itself, get both patches (no single patch with the array's own values makes a descent there).
    Raises NoDescent where the base's values do not allow exactly one descent at p."""
    s = np.asarray(sorted_bits)
    n = s.size
    assert 0 <= p <= n - 2
    k = ol.kdf_keys
    key = lambda i: int(k(s[i:i + 1], dtype, order)[0])
    lo, hi = s[0], s[n - 1]
    if 2 * p < n and p == n - 2:                 # n == 2 or 3
        if not key(n - 1) > key(0):
            raise NoDescent((n, p))
        patched = s.copy()
        patched[p], patched[p + 1] = hi, lo
        want = sort_by_kdf(patched, dtype, order)
        return Case(p, "both", [(p, hi), (p + 1, lo)], [("v", v) for v in want])
    if 2 * p < n:
        if not key(n - 1) > key(p + 1):
            raise NoDescent((n, p))
        return Case(p, "raise", [(p, hi)], [("s", 0, p), ("s", p + 1, n), ("s", n - 1, n)])
    if not key(p) > key(0):
        raise NoDescent((n, p))
    return Case(p, "lower", [(p + 1, lo)], [("s", 0, 1), ("s", 0, p + 1), ("s", p + 2, n)])


def apply_patches(base, case):
    out = np.array(base, copy=True)
    for i, v in case.patches:
        out[i] = v
    return out


def assemble(sorted_bits, case):
    s = np.asarray(sorted_bits)
    parts = [s[pc[1]:pc[2]] if pc[0] == "s" else np.array([pc[1]], dtype=s.dtype) for pc in case.pieces]
    return np.concatenate(parts) if parts else s[:0].copy()


def one_descent(sorted_bits, dtype, order, p):
    """(array, expected sorted array): `sorted_bits` (sorted in KDF order) with exactly one descent, between elements p and p + 1,
    and its sorted order derived from the base by moving the one element.  Raises NoDescent if the base does not allow it."""
    case = descent_case(sorted_bits, dtype, order, p)
    return apply_patches(sorted_bits, case), assemble(sorted_bits, case)


def descents(bits, dtype, order):
    """Where the derived keys descend."""
    k = ol.kdf_keys(bits, dtype, order)
    return np.flatnonzero(k[:-1] > k[1:])


# ---- one stray key in a constant column ----------------------------------------------------------------------------------
def force_columns(bits, dtype, order, columns, seed=0):
    """`bits` with the byte columns `columns` of the DERIVED keys made constant (a seeded byte per column, never 0x00 or 0xFF), so
    that the column is constant for signed, float and descending keys alike."""
    ut = ol.NP_BITS[dtype]
    k = ol.kdf_keys(bits, dtype, order)
    for j, c in enumerate(columns):
        byte = 1 + splitmix64(0xC01 + 131 * seed + c, 1)[0] % 254
        k = (k & ~ut(0xFF << (8 * c))) | ut(byte << (8 * c))
    return kdf_inverse(k, dtype, order)


def one_stray(bits, dtype, column, p, bit):
    """`bits` with bit `bit` of byte column `column` of element p's derived key flipped (the same bit in either order)."""
    out = np.array(bits, dtype=ol.NP_BITS[dtype], copy=True)
    k = ol.kdf_keys(out[p:p + 1], dtype)
    k ^= ol.NP_BITS[dtype](1 << (8 * column + bit))
    out[p] = kdf_inverse(k, dtype)[0]
    return out


def stray_case(base, sorted_base_bits, dtype, order, column, p, bit, sorted_keys=None):
    """The Case of one_stray against the base's own sorted order: one key leaves its place and enters another.  `sorted_keys`:
    kdf_keys(sorted_base_bits), for callers that make many cases of one base (O(log n) each then)."""
    new = one_stray(base[p:p + 1], dtype, column, 0, bit)[0]
    s = np.asarray(sorted_base_bits)
    n = s.size
    ks = ol.kdf_keys(s, dtype, order) if sorted_keys is None else sorted_keys
    k_old = ol.kdf_keys(base[p:p + 1], dtype, order)[0]
    k_new = ol.kdf_keys(np.array([new], dtype=s.dtype), dtype, order)[0]
    r = int(np.searchsorted(ks, k_old, side="left"))        # the key that leaves (any of its equals: the same bits)
    assert ks[r] == k_old
    q = int(np.searchsorted(ks, k_new, side="left"))        # where the new key enters, as an index of s
    if q <= r:
        pieces = [("s", 0, q), ("v", new), ("s", q, r), ("s", r + 1, n)]
    else:
        pieces = [("s", 0, r), ("s", r + 1, q), ("v", new), ("s", q, n)]
    return Case(p, "stray", [(p, new)], pieces)


def kept_columns(bits, dtype, order):
    """The byte columns in which some derived key differs from the first (radix_sort.hpp:64-70), lowest first."""
    k = ol.kdf_keys(bits, dtype, order)
    diff = int(np.bitwise_or.reduce(k ^ k[0])) if k.size else 0
    return [c for c in range(ol.DTYPE_SIZE[dtype]) if (diff >> (8 * c)) & 0xFF]


def rank_pieces(sorted_bits, dtype, order, case):
    """The stable ranks (radix_sort_rank.hpp: equal keys in index order) of a descent case as pieces over arange(n): the raised
    element (index p) goes in FRONT of the keys equal to the maximum, which all lie behind it; the lowered one (index p + 1)
    BEHIND the keys equal to the minimum, which all lie in front of it."""
    s = np.asarray(sorted_bits)
    n, p = s.size, case.p
    ks = ol.kdf_keys(s, dtype, order)
    if case.kind == "raise":
        j = int(np.searchsorted(ks, ks[n - 1], side="left"))
        j = max(j, p + 1)
        return [("s", 0, p), ("s", p + 1, j), ("v", p), ("s", j, n)]
    if case.kind == "lower":
        q = min(int(np.searchsorted(ks, ks[0], side="right")), p + 1)
        return [("s", 0, q), ("v", p + 1), ("s", q, p + 1), ("s", p + 2, n)]
    perm = np.argsort(ol.kdf_keys(apply_patches(s, case), dtype, order), kind="stable")
    return [("v", int(i)) for i in perm]


# ---- the cases of tests/test_gpu_decisions.py, listed once: tests/test_decide_lib_cpu.py walks the same lists -------------------
SMALL = 65536                 # arrays up to here: the oracle is asked per case; beyond: per base and construction, and at spot checks
CAP = lambda dt: 65536 // ol.DTYPE_SIZE[dt]       # the one-workgroup kernel's largest array (rsx_small.hpp)
N_B = (70001, (1 << 21) + 12345)
N_C = (1 << 22) + 3
N_D = ((1 << 20) + 1, 1 << 21)
OFFSETS_B = (0, 1, 3)         # elements between a 16-byte-aligned address and the array's start
B_DTYPES = (ol.U8, ol.I16, ol.U32, ol.F32, ol.I64, ol.F64)

# family, dtype, order, n, offsets, sampled (positions of the sample-trusting routes too), rand (random positions), base ("mixed" | "zipf")
Spec = collections.namedtuple("Spec", "family dtype order n offsets sampled rand base")


def spec_id(s):
    return "%s-%s-%s-n%d" % (s.family, ol.DTYPE_NAMES[s.dtype], "desc" if s.order else "asc", s.n)


def presorted_specs(family):
    """The bases of the pre-sorted family, by the issue's letters (E and F name the entry points the GPU module runs them through)."""
    both = (ol.ASC, ol.DESC)
    if family == "A":
        return [Spec("A", dt, o, n, (0,), False, RANDOM_POSITIONS, "mixed")
                for dt in range(10) for o in both for n in (2, 3, 1000, CAP(dt) - 1, CAP(dt))]
    if family == "A-rank-pairs":
        return [Spec("A-rank-pairs", dt, o, 1000, (0,), False, RANDOM_POSITIONS, "mixed") for dt in (ol.U32, ol.F32) for o in both]
    if family == "B":
        return [Spec("B", dt, o, n, OFFSETS_B, False, RANDOM_POSITIONS, "mixed") for dt in B_DTYPES for o in both for n in N_B]
    if family == "C":
        return [Spec("C", dt, o, N_C, (0,), True, RANDOM_POSITIONS, "mixed")
                for dt, o in ((ol.U32, ol.ASC), (ol.U32, ol.DESC), (ol.F32, ol.DESC), (ol.U64, ol.ASC))]
    if family == "D":
        return [Spec("D", ol.U64, ol.ASC, n, (0,), True, RANDOM_POSITIONS, "zipf") for n in N_D]
    if family == "E":
        return [Spec("E", ol.U32, ol.ASC, (1 << 21) + 12345, (0,), False, 0, "mixed"),
                Spec("E", ol.U32, ol.ASC, N_C, (0,), True, 0, "mixed"),
                Spec("E", ol.U64, ol.ASC, (1 << 21) + 7, (0,), False, 0, "mixed")]
    if family == "E-rank-pairs":
        return [Spec("E-rank-pairs", ol.F32, ol.ASC, (1 << 20) + 3, (0,), False, 0, "mixed")]
    if family == "F":
        return [Spec("F", dt, o, 70001, (0,), False, RANDOM_POSITIONS, "mixed") for dt in (ol.U32, ol.F64) for o in both] + \
               [Spec("F", ol.U32, ol.ASC, (1 << 21) + 12345, (0,), False, RANDOM_POSITIONS, "mixed")]
    raise ValueError(family)


PRESORTED_FAMILIES = ("A", "A-rank-pairs", "B", "C", "D", "E", "E-rank-pairs", "F")


def base_seed(spec):
    return 1 + (7 * spec.dtype + 3 * spec.order + spec.n) % 1000003


_bases = collections.OrderedDict()


def spec_base(spec):
    """The sorted base of a spec (the last few are kept: specs that share dtype, order, n and kind share the array)."""
    key = (spec.base, spec.dtype, spec.order, spec.n)
    if key in _bases:
        _bases.move_to_end(key)
        return _bases[key]
    if spec.base == "zipf":
        assert spec.dtype == ol.U64 and spec.order == ol.ASC
        a = np.sort(zipf_like(spec.n, base_seed(spec)))
    else:
        a = sorted_base(spec.n, spec.dtype, spec.order, base_seed(spec))
    a.setflags(write=False)
    _bases[key] = a
    while len(_bases) > 3:
        _bases.popitem(last=False)
    return a


def spec_positions(spec, offset=0):
    kb = ol.DTYPE_SIZE[spec.dtype]
    return positions(spec.n, kb, head_elems_of(offset, kb), sampled=spec.sampled, rand=spec.rand)


def spot_positions(ps, count=8):
    """`count` of the positions `ps`, spread over them, both ends included."""
    if len(ps) <= count:
        return list(ps)
    return sorted(set(ps[(i * (len(ps) - 1)) // (count - 1)] for i in range(count)))


# kept-columns family: dtype, order, the derived keys' constant columns (a stray key is put into each of them in turn)
StraySpec = collections.namedtuple("StraySpec", "dtype order n constant sampled")
STRAY_KEYS = ((ol.U8, ol.ASC, (0,)), (ol.U16, ol.ASC, (1,)), (ol.U32, ol.ASC, (2,)), (ol.U32, ol.ASC, (1, 3)),
              (ol.U32, ol.ASC, (1, 2, 3)), (ol.U64, ol.ASC, (5, 6, 7)), (ol.I64, ol.ASC, (5, 6, 7)), (ol.F32, ol.DESC, (0,)))
STRAY_BITS = (0, 7)
STRAY_BITS_D = (45, 50, 63)          # above the log route's window (rsx_logroute.hpp: at most 44 varying low bits)


def stray_specs(size_class):
    """size_class "A": 1000 and the one-workgroup kernel's largest array; "B": N_B; "C": N_C with the sample's places."""
    out = []
    for dt, o, const in STRAY_KEYS:
        ns = {"A": (1000, CAP(dt)), "B": N_B, "C": (N_C,)}[size_class]
        out += [StraySpec(dt, o, n, const, size_class == "C") for n in ns]
    return out


def stray_id(s):
    return "%s-%s-n%d-const%s" % (ol.DTYPE_NAMES[s.dtype], "desc" if s.order else "asc", s.n, "".join(map(str, s.constant)))


def stray_base(spec):
    """Unsorted splitmix keys with the spec's columns of the derived keys constant."""
    a = ol.splitmix_fill(spec.n, spec.dtype, 11 + spec.n % 97 + 5 * spec.dtype)
    a = force_columns(a, spec.dtype, spec.order, spec.constant, seed=spec.dtype)
    a.setflags(write=False)
    return a


def stray_base_d(n):
    """Unsorted Zipf-like keys below 2^40 (the log route's input)."""
    a = zipf_like(n, 21 + n % 13)
    a.setflags(write=False)
    return a


def stray_decision(base, base_kept, dtype, order, column, case):
    """(kept columns, result_in_aux, early_exit) of `base` with the stray key of `case`, restated: the base's kept columns plus
    the stray's (radix_sort.hpp:64-70: whether the stray is the first key or another one, it and the first key differ there),
    the buffer by their parity (:92).  A base of equal keys (one-byte keys with their column constant) is looked at whole: with
    one other key it may well still be sorted (:60-62).  tests/test_decide_lib_cpu.py pins this against the oracle."""
    if base_kept:
        kept = sorted(set(base_kept) | {column})
        return kept, len(kept) & 1, 0
    a = apply_patches(base, case)
    if descents(a, dtype, order).size == 0:
        return [], 0, 2
    kept = kept_columns(a, dtype, order)
    return kept, len(kept) & 1, 0
