"""Stage model for the as-run stage read-backs (TEST INFRASTRUCTURE; Python integers and NumPy, nothing of the engine).

What the kernels of a G1 MSM must leave behind, written from the geometries' definitions (csrc/common.hpp, the comments of
csrc/kernels/decompose.hpp and wide.hpp), not from their code:

    recode(k, geometry)   digits of one scalar, the flags the kernel must raise, the values it must store
    digit_matrix(...)     the same for a list of scalars, as the digit columns of every window slot
    csr(stored, ...)      per key of a slot: how many entries, and which (entry, sign) pairs
    bucket_sum(...)       the sum a bucket must hold, by pyref's group law (ed=True: Edwards-BLS12 points, pyref.ed_add /
                          ed_neg, the identity (0, 1); such calls take k_decompose, so their recode is even16() / equal16())
    ed_record_affine(...) the affine point an Edwards-BLS12 bucket record stands for

A geometry is a Geometry value from equal16 / even16 / narrow22 / short / wide13 / glv8.  tests/test_stage_model_host.py
pins this module (digits rebuild the scalar, ranges, flag sets, agreement with the oracle's recode and with the short
recode of tests/test_short_scalars_host.py) before tests/test_stage_geometries_gpu.py compares the GPU with it.
"""
import os
import sys
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bits of the device error word a recode may raise (csrc/common.hpp)
ERR_SCALAR, ERR_GLV_RANGE, ERR_RERUN, ERR_SHORT_WIDTH = 1, 2, 128, 256
KEY_TRACKED, KEY_UNSIGNED = 0x80000000, 0x40000000

_GLV = None


def glv_consts():
    """(lambda, beta) of the GLV endomorphism phi(x, y) = (beta x, y) = [lambda](x, y), from tools/gen_consts.py."""
    global _GLV
    if _GLV is None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_consts

        _GLV = (gen_consts.GLV_LAMBDA, gen_consts._find_beta())
    return _GLV


class Slot(NamedTuple):
    offset: int      # bit offset of the slot's field in the scalar (its weight is 2^offset)
    width: int       # bits of the field
    signed: bool     # signed digit with a carry into the next slot of its chain, or unsigned
    bias: int        # stored value = digit + bias
    key_unsigned: bool = False  # the sort reads the stored value itself as the key


class Geometry(NamedTuple):
    name: str
    bucket_log: int
    slots: Tuple[Slot, ...]
    digit_bytes: int = 2
    bits: int = 0    # short scalars: the declared width


def equal16():
    """Sixteen signed 16-bit windows, digits in [-2^15, 2^15), stored d + 2^15; a final carry is the scalar error."""
    return Geometry("equal16", 15, tuple(Slot(16 * w, 16, True, 1 << 15) for w in range(16)))


def even16():
    """Thirteen signed 16-bit windows, then three unsigned 15-bit ones at bits 208, 223, 238 with a carry chain of their own."""
    return Geometry("even16", 15, tuple(Slot(16 * w, 16, True, 1 << 15) for w in range(13)) + tuple(Slot(208 + 15 * j, 15, False, 1 << 15) for j in range(3)))


def narrow22():
    """Eleven signed 12-bit windows, then eleven unsigned 11-bit ones (from bit 132), 2^11 buckets, stored d + 2^11."""
    return Geometry("narrow22", 11, tuple(Slot(12 * w, 12, True, 1 << 11) for w in range(11)) + tuple(Slot(132 + 11 * j, 11, False, 1 << 11) for j in range(11)))


def short(bits, L):
    """floor(bits / (L + 1)) signed digits of L + 1 bits, then the unsigned rest plus the carry (at most 2^L).  On 2^15
    buckets the top slot is stored unbiased and sorted as an unsigned key; on 2^11 buckets it is biased like the others."""
    c = L + 1
    W = bits // c + 1
    top = Slot(c * (W - 1), max(bits - c * (W - 1), 0), False, 0 if L == 15 else 1 << L, L == 15)
    return Geometry("short", L, tuple(Slot(c * w, c, True, 1 << L) for w in range(W - 1)) + (top,), 2, bits)


WIDE_WIDTHS = (20,) * 6 + (19,) * 7


def wide_offset(w):
    return sum(WIDE_WIDTHS[:w])


def wide13():
    """Six 20-bit and seven 19-bit windows into ONE set of 2^19 buckets: windows 0..11 signed (d = v - 2^width when
    v >= 2^(width - 1)), the top one (from bit 234) unsigned; stored d + 2^19 as 32-bit values."""
    return Geometry("wide13", 19, tuple(Slot(wide_offset(w), WIDE_WIDTHS[w], w < 12, 1 << 19) for w in range(13)), 4)


def glv8():
    """k = k1 + lambda k2 with k1 = k mod lambda, k2 = k div lambda, both below 2^127: eight signed 16-bit digits each (the
    top one stays non-negative).  Slot w holds 2n columns: column i = digit w of k1_i, column n + i = digit w of k2_i."""
    return Geometry("glv8", 15, tuple(Slot(16 * w, 16, True, 1 << 15) for w in range(8)))


class Recode(NamedTuple):
    digits: List[int]   # one per slot (GLV: the 8 digits of k1, then the 8 of k2)
    stored: List[int]   # what the kernel writes for them
    flags: int          # ERR_* bits the kernel must raise for this scalar


def _final_carry16(k):
    """The scalar error of every geometry: the sixteen-window signed recode ends with a carry (k >= 2^255 - 2^239)."""
    carry = 0
    for w in range(16):
        carry = 1 if ((k >> (16 * w)) & 0xFFFF) + carry >= 32768 else 0
    return carry


def _signed_chain(k, slots, last_carries=True):
    """Signed digits of consecutive slots: v = field + carry; v >= 2^(width - 1) becomes v - 2^width and carries."""
    digits, carry = [], 0
    for j, s in enumerate(slots):
        v = ((k >> s.offset) & ((1 << s.width) - 1)) + carry
        carry = 1 if v >= (1 << (s.width - 1)) and (last_carries or j + 1 < len(slots)) else 0
        digits.append(v - (carry << s.width))
    return digits, carry


def recode(k: int, g: Geometry) -> Recode:
    assert 0 <= k < (1 << 256)
    flags = 0
    if g.name == "glv8":
        lam, _ = glv_consts()
        k1, k2 = k % lam, k // lam
        digits = []
        for half in (k1, k2):
            d, _ = _signed_chain(half & ((1 << 128) - 1), g.slots, last_carries=False)
            if half >> 128 or d[-1] >= (1 << 15):  # does not fit eight windows with a non-negative top digit
                flags |= ERR_GLV_RANGE
            digits += d
        stored = [(d + (1 << 15)) & 0xFFFF for d in digits]
        return Recode(digits, stored, flags)
    if g.name == "short":
        if k >> g.bits:
            flags |= ERR_SHORT_WIDTH
            k &= (1 << g.bits) - 1  # the excess is dropped before the recode
        digits, carry = _signed_chain(k, g.slots[:-1])
        digits.append((k >> g.slots[-1].offset) + carry)
        return Recode(digits, [d + s.bias for d, s in zip(digits, g.slots)], flags)
    if _final_carry16(k):
        flags |= ERR_SCALAR
    signed = [s for s in g.slots if s.signed]
    digits, carry = _signed_chain(k, signed)
    if g.name == "equal16":
        return Recode(digits, [(d + s.bias) & 0xFFFF for d, s in zip(digits, g.slots)], flags)  # (a flagged scalar wraps)
    if g.name == "wide13":
        top = (k >> g.slots[-1].offset) + carry
        if top > (1 << 19):
            flags |= ERR_RERUN
            top = 0  # the kernel stores digit 0 for it; the call reruns
        digits.append(top)
        return Recode(digits, [d + s.bias for d, s in zip(digits, g.slots)], flags)
    # even16 / narrow22: unsigned L-bit digits with a carry chain of their own (field + carry = 2^L: digit 0, carry on)
    for s in g.slots[len(signed):]:
        v = ((k >> s.offset) & ((1 << s.width) - 1)) + carry
        carry = v >> s.width
        digits.append(v & ((1 << s.width) - 1))
    if carry or k >> 253:
        flags |= ERR_RERUN  # the digits then no longer rebuild k: the call reruns on sixteen equal windows
    return Recode(digits, [d + s.bias for d, s in zip(digits, g.slots)], flags)


def rebuild(digits, g: Geometry) -> int:
    """The scalar a digit vector stands for under the geometry's weights."""
    if g.name == "glv8":
        lam, _ = glv_consts()
        k1 = sum(d << (16 * w) for w, d in enumerate(digits[:8]))
        k2 = sum(d << (16 * w) for w, d in enumerate(digits[8:]))
        return k1 + lam * k2
    return sum(d << s.offset for d, s in zip(digits, g.slots))


def digit_matrix(scalars, g: Geometry):
    """(stored, flags): stored[slot] is the slot's digit column(s) as the kernel writes them -- n values; 2n behind the
    GLV front end; the wide table has ONE slot of 13n values, window-major -- and flags the OR over all scalars."""
    recs = [recode(k, g) for k in scalars]
    flags = 0
    for r in recs:
        flags |= r.flags
    dt = np.uint32 if g.digit_bytes == 4 else np.uint16
    if g.name == "glv8":
        cols = [np.array([r.stored[w] for r in recs] + [r.stored[8 + w] for r in recs], dtype=dt) for w in range(8)]
    elif g.name == "wide13":
        cols = [np.array([r.stored[w] for w in range(13) for r in recs], dtype=dt)]
    else:
        cols = [np.array([r.stored[w] for r in recs], dtype=dt) for w in range(len(g.slots))]
    return cols, flags


def keys_and_signs(stored: np.ndarray, bias: int, key_unsigned: bool):
    """Sort key |d| and sign of every stored digit of a slot."""
    d = stored.astype(np.int64) - (0 if key_unsigned else bias)
    return np.abs(d), (d < 0)


class Csr(NamedTuple):
    counts: np.ndarray  # entries per key 0 .. 2^L
    order: np.ndarray   # entry numbers (positions in the slot's columns) grouped by key
    start: np.ndarray   # start[key] .. start[key + 1] indexes `order`
    sign: np.ndarray    # per entry number

    def row(self, key):
        """The multiset of (entry, sign) of a key, sorted."""
        return sorted((int(e), int(self.sign[e])) for e in self.order[self.start[key] : self.start[key + 1]])


def csr(stored: np.ndarray, L: int, bias: int, key_unsigned: bool = False) -> Csr:
    key, sign = keys_and_signs(stored, bias, key_unsigned)
    assert key.max(initial=0) <= (1 << L), "a digit outside the bucket range"
    counts = np.bincount(key, minlength=(1 << L) + 1)
    order = np.argsort(key, kind="stable")
    start = np.concatenate(([0], np.cumsum(counts)))
    return Csr(counts, order, start, sign)


def phi(pt):
    _, beta = glv_consts()
    return None if pt is None else (beta * pt[0] % R.P, pt[1])


def entry_base(points, entry, g: Geometry, n: int, cache: Optional[dict] = None, ed: bool = False):
    """The point an entry of a slot adds: P_i; behind the GLV front end P_i for entry i and phi(P_i) for entry n + i; on
    the wide table [2^wide_offset(w)] P_i for entry w n + i.  ed: an Edwards-BLS12 call, whose slots all gather P_i."""
    if ed:
        assert g.name in ("even16", "equal16"), "Edwards-BLS12 calls run sixteen windows over their own points"
        return points[entry]
    if g.name == "glv8":
        return points[entry] if entry < n else phi(points[entry - n])
    if g.name == "wide13":
        if cache is not None and entry in cache:
            return cache[entry]
        w, i = divmod(entry, n)
        pt = R.mul(points[i], 1 << wide_offset(w))
        if cache is not None:
            cache[entry] = pt
        return pt
    return points[entry]


def bucket_sum(points, row, g: Geometry, n: int, cache: Optional[dict] = None, ed: bool = False):
    """Sum over a row's (entry, sign) pairs of +-base(entry): what bucket key - 1 of the slot must hold.  The identity is
    None for G1 and (0, 1) for Edwards-BLS12 (ed), whose complete law takes every curve point, low-order ones included."""
    if ed:
        acc = R.ED_ID
        for entry, sign in row:
            pt = entry_base(points, entry, g, n, cache, ed=True)
            acc = R.ed_add(acc, R.ed_neg(pt) if sign else pt)
        return acc
    acc = None
    for entry, sign in row:
        pt = entry_base(points, entry, g, n, cache)
        acc = R.add(acc, R.neg(pt) if sign else pt)
    return acc


def key_max_word(stored: np.ndarray, bias: int, key_unsigned: bool) -> int:
    """The key_max word of a slot whose largest key the decomposition tracks."""
    key, _ = keys_and_signs(stored, bias, key_unsigned)
    return int(key.max(initial=0)) | KEY_TRACKED | (KEY_UNSIGNED if key_unsigned else 0)


_FQ = None


def fq_model():
    """lazy_model.FieldModel("Fq"): modulus, limb count, Montgomery radix 2^261 and the stored-record shapes of the 9-limb field."""
    global _FQ
    if _FQ is None:
        import lazy_model

        _FQ = lazy_model.FieldModel("Fq")
    return _FQ


def ed_record_affine(words):
    """An Edwards-BLS12 bucket record as read back -- X, Y, T, Z of 9 limbs each, lazy residues in Montgomery form -- as the
    affine point (X / Z, Y / Z): limbs to a value, times 2^-261 mod q.  Zero may be stored as 0 or as q; the point (0, 1) is
    the identity whichever it is.  The record must be a point: Z != 0, T Z = X Y, on the curve."""
    fq = fq_model()
    n = fq.N
    X, Y, T, Z = (sum(int(x) << (29 * j) for j, x in enumerate(words[n * c : n * c + n])) * fq.Rinv % fq.P for c in range(4))
    assert Z != 0 and (X * Y - T * Z) % fq.P == 0, "extended-coordinate invariant T Z = X Y violated"
    zi = pow(Z, -1, fq.P)
    pt = (X * zi % fq.P, Y * zi % fq.P)
    assert R.ed_on_curve(pt), "not on the Edwards-BLS12 curve"
    return pt
