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


# ---- the accumulation work list (msm377_g1_read_work_list) ----
# Written from the comments of csrc/kernels/accumulate.hpp and the contract in include/msm377.h: a row of more than SEG
# entries is cut into the fewest equal parts of at most SEG entries.  ceil() is spelled -(-a // b) here, not as the
# kernel spells it.
SEG_BINS = 129            # work items are counted by length 0 .. 128
LONG_ROW_PARTIALS = 32    # k_fold_long_rows folds the rows of its slot with MORE work items than this


class RowSplit(NamedTuple):
    nseg: int
    seglen: int
    lastlen: int


def row_split(length: int, seg: int) -> RowSplit:
    """(work items, entries per item, entries of the last item) of a row: one item up to `seg` entries (also for an empty
    row: an item of length 0); beyond that parts = ceil(len / seg) equal parts of ceil(len / parts) entries -- as many
    of those as the row fills, the last one holding the rest."""
    if length <= seg:
        return RowSplit(1, length, length)
    parts = -(-length // seg)
    seglen = -(-length // parts)
    nseg = -(-length // seglen)
    return RowSplit(nseg, seglen, length - (nseg - 1) * seglen)


def item_range(length: int, seg: int, s: int):
    """Entries [lo, hi) of a row of `length` entries that its work item s adds."""
    sp = row_split(length, seg)
    assert 0 <= s < sp.nseg
    return s * sp.seglen, min((s + 1) * sp.seglen, length)


class WorkList(NamedTuple):
    hist: List[int]            # hist[b]: work items of b entries
    items: int                 # work items in all
    split_rows: List[int]      # rows of more than one item, ascending
    overflow_slots: int        # sum of nseg - 1 over the split rows
    item_set: np.ndarray       # the set of (row, seg, entries) items: an (items, 3) int64 array sorted by (row, seg)
    folded: List[int]          # rows of the fold slot with more than LONG_ROW_PARTIALS items (empty without a fold slot)


def work_list(row_lens, seg: int, fold_slot: int = -1, bucket_log: int = 15) -> WorkList:
    """The work list of a pass from the lengths of its rows (row = slot 2^L + t, in that order).  fold_slot: the window
    slot k_fold_long_rows is launched on, -1: none.  (Rows of one item -- nearly all of half a million -- are listed
    with NumPy, the split rows one by one.)"""
    lens = np.asarray(row_lens, dtype=np.int64)
    one = np.nonzero(lens <= seg)[0]
    items = [np.stack([one, np.zeros_like(one), lens[one]], axis=1)]
    split, folded, ovf = [], [], 0
    for row in np.nonzero(lens > seg)[0]:
        row, length = int(row), int(lens[row])
        sp = row_split(length, seg)
        assert sp.nseg > 1
        ranges = [item_range(length, seg, s) for s in range(sp.nseg)]
        items.append(np.array([(row, s, hi - lo) for s, (lo, hi) in enumerate(ranges)], dtype=np.int64))
        split.append(row)
        ovf += sp.nseg - 1
        if fold_slot >= 0 and row >> bucket_log == fold_slot and sp.nseg > LONG_ROW_PARTIALS:
            folded.append(row)
    item_set = np.concatenate(items)
    item_set = item_set[np.lexsort((item_set[:, 1], item_set[:, 0]))]
    hist = [int(x) for x in np.bincount(item_set[:, 2], minlength=SEG_BINS)]
    assert len(hist) == SEG_BINS, "a work item of more than 128 entries"
    return WorkList(hist, len(item_set), split, ovf, item_set, folded)


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


# ---- the window records (msm377_g1_read_partials): what the bucket reduction must hand to the host tail ----
# csrc/kernels/reduce.hpp lines 10-22: per record, point 0 = the sum of all 2^L buckets and point 1 + b = the sum of the
# buckets whose INDEX has bit b set, b < L; bucket index t holds key t + 1.  Written from that definition, not from the tree.
FORM_XYZZ, FORM_TE, FORM_ED = 0, 1, 2  # MSM377_STAGE_FORM_*
RECORD_TAG = 0x80000000  # TE_RECORD_TAG: bit 31 of the last word of coordinate 0 of point 0 of a FORM_TE record


def group(ed=False):
    """(add, neg, mul, identity, generator, order of the generator) of the curve of a call."""
    if ed:
        return R.ed_add, R.ed_neg, R.ed_mul, R.ED_ID, R.ED_G, R.ED_SUBGROUP
    return R.add, R.neg, R.mul, None, R.G, R.R_ORDER


def record_slots(g: Geometry, fold=False):
    """Window slots that go into each record: one each, or all of them into ONE record behind the 16-bit table (fold)."""
    count = 1 if g.name == "wide13" else len(g.slots)
    return [list(range(count))] if fold else [[s] for s in range(count)]


def entry_weight(entry, slot, g: Geometry, n: int, fold=False):
    """(index of the point, factor) of an entry of a slot: the base it adds is [factor] points[index].  lambda behind the
    GLV front end for entry n + i; 2^wide_offset(w) on the wide table; 2^(16 slot) on the folded 16-bit table, whose window
    `slot` holds [2^(16 slot)] P_i."""
    if g.name == "glv8":
        return (entry, 1) if entry < n else (entry - n, glv_consts()[0])
    if g.name == "wide13":
        w, i = divmod(entry, n)
        return i, 1 << wide_offset(w)
    return entry, (1 << g.slots[slot].offset) if fold else 1


def partial_points(points, cols, g: Geometry, n: int, logs=None, ed=False, fold=False):
    """For every record of a call (one per slot; ONE with fold, the sixteen slots of the 16-bit table added together; one on
    the wide table, whose 13 digit columns share a bucket set): [total, plane_0, .., plane_(L-1)] as affine points (the
    identity: None on G1, (0, 1) on Edwards-BLS12).  total = the sum of all buckets, plane_b = the sum of the buckets whose
    index t = key - 1 has bit b set.
    logs[i]: the discrete logarithm of points[i] to the curve's generator, or None where it is not known (low-order points,
    points outside the subgroup): entries with a known logarithm are summed as integers and cost ONE scalar multiplication
    per point of a record; the others are added one by one with the group law."""
    add, neg, mul, ident, gen, order = group(ed)
    L = g.bucket_log
    out = []
    for slots in record_slots(g, fold):
        log_sum = [0] * (L + 1)
        rest = [ident] * (L + 1)
        for slot in slots:
            s = g.slots[-1] if g.name == "wide13" else g.slots[slot]
            key, sign = keys_and_signs(cols[slot], s.bias, s.key_unsigned)
            for entry in np.nonzero(key)[0]:
                t = int(key[entry]) - 1
                i, factor = entry_weight(int(entry), slot, g, n, fold)
                where = [0] + [1 + b for b in range(L) if (t >> b) & 1]
                if logs is not None and logs[i] is not None:
                    v = -factor * logs[i] if sign[entry] else factor * logs[i]
                    for p in where:
                        log_sum[p] += v
                else:
                    assert not ed or factor == 1
                    pt = mul(points[i], factor) if factor != 1 else points[i]
                    pt = neg(pt) if sign[entry] else pt
                    for p in where:
                        rest[p] = add(rest[p], pt)
        out.append([add(mul(gen, v % order) if v % order else ident, q) for v, q in zip(log_sum, rest)])
    return out


def record_weights(g: Geometry, fold=False):
    """Bit offset of every record in the result: the slot's; 0 for the one record behind a table."""
    return [0 if (fold or g.name == "wide13") else g.slots[slots[0]].offset for slots in record_slots(g, fold)]


def weighted_sum(records, g: Geometry, ed=False, fold=False):
    """sum_records 2^offset (total + sum_b 2^b plane_b) = sum_t (t + 1) B[t] over every window: the call's result."""
    add, _, mul, ident, _, _ = group(ed)
    acc = ident
    for rec, off in zip(records, record_weights(g, fold)):
        w = rec[0]
        for b, pl in enumerate(rec[1:]):
            w = add(w, mul(pl, 1 << b))
        acc = add(acc, mul(w, 1 << off))
    return acc


def meetings(x, y, L):
    """Where the reduction tree first adds what started in bucket x to what started in bucket y: a list of (level r, array)
    with array 0 = the running block, 1 + r' = the list that level r' left behind.  reduce.hpp: level r folds
    B[lo + k + half] onto B[lo + k] for k < half = 2^L >> (r + 1), in the running block (lo = 0) and in the list of every
    earlier level r' (lo = 2^L >> (r' + 1)); the upper half is only read, so the block's upper half stays behind as the
    list of level r.  Replayed on the occupied bucket indices alone; two buckets can meet in more than one array (a pair in
    the block's upper half meets again in the list that half becomes)."""
    NB = 1 << L
    held = {x: {"x"}, y: {"y"}} if x != y else {x: {"x", "y"}}
    out = []
    for r in range(L):
        half = NB >> (r + 1)
        step = {}
        for arr in range(r + 1):
            lo = 0 if arr == 0 else NB >> arr
            for at, labels in held.items():
                if lo + half <= at < lo + 2 * half:
                    step[at - half] = (set(labels), arr)
        for to, (labels, arr) in sorted(step.items()):
            have = held.setdefault(to, set())
            if have and labels and len(have) == 1 and len(labels) == 1 and have != labels:
                out.append((r, arr))
            have |= labels
    return sorted(out)


def record_point_contract(words, form, first_point):
    """The contract of one point of a window record (include/msm377.h): four coordinates of 12 (8: Edwards-BLS12) u32
    words, each CANONICAL -- below the modulus -- once the tag is taken off; the tag (bit 31 of the last word of
    coordinate 0) set on point 0 of a FORM_TE record and nowhere else.  Returns the four coordinates as Montgomery
    residues (radix 2^(32 words))."""
    cw = 8 if form == FORM_ED else 12
    mod = R.Q if form == FORM_ED else R.P
    w = [int(x) for x in words]
    assert len(w) == 4 * cw
    tagged = form == FORM_TE and first_point
    assert bool(w[cw - 1] & RECORD_TAG) == tagged, "the tag bit of coordinate 0 is %s" % ("missing" if tagged else "set where it must not be")
    w[cw - 1] &= ~RECORD_TAG
    vals = [sum(w[cw * c + i] << (32 * i) for i in range(cw)) for c in range(4)]
    for c, v in enumerate(vals):
        assert v < mod, "coordinate %d is not canonical (at or above the modulus%s)" % (c, "; bit 31 of its last word set" if w[cw * c + cw - 1] >> 31 else "")
    return vals


def record_point_affine(words, form, first_point=False):
    """Contract, invariant and value of one point of a window record: ZZ^3 = ZZZ^2 (FORM_XYZZ; the identity is ZZ = ZZZ =
    0), T Z = X Y and the curve equation (both Edwards forms; the identity is (0 : c : 0 : c), c != 0).  FORM_XYZZ and
    FORM_TE give the Weierstrass affine point or None, FORM_ED the Edwards-BLS12 affine point ((0, 1): the identity)."""
    import util

    vals = record_point_contract(words, form, first_point)
    if form == FORM_ED:
        ri = pow(1 << 256, -1, R.Q)
        X, Y, T, Z = (v * ri % R.Q for v in vals)
        assert Z != 0 and (X * Y - T * Z) % R.Q == 0, "extended-coordinate invariant T Z = X Y violated"
        zi = pow(Z, -1, R.Q)
        pt = (X * zi % R.Q, Y * zi % R.Q)
        assert R.ed_on_curve(pt), "not on the Edwards-BLS12 curve"
        return pt
    plain = [x for v in vals for x in util._words12(v)]
    if form == FORM_TE:
        return util.affine_from_te_record_words(plain)
    ri = pow(util.R64, -1, R.P)
    if vals[2] == 0:
        assert vals[3] == 0, "the Weierstrass identity stores ZZ = ZZZ = 0"
    else:
        assert vals[3] * ri % R.P != 0
    return util.affine_from_record_words(plain)


def is_stored_identity(words, form):
    """The identity AS STORED: (0 : c : 0 : c) with c != 0 in the Edwards forms, ZZ = ZZZ = 0 in the Weierstrass form."""
    cw = 8 if form == FORM_ED else 12
    w = [int(x) for x in words]
    w[cw - 1] &= ~RECORD_TAG
    c = [w[cw * k : cw * k + cw] for k in range(4)]
    if form == FORM_XYZZ:
        return not any(c[2]) and not any(c[3])
    return not any(c[0]) and not any(c[2]) and c[1] == c[3] and any(c[1])


def ed_record_point_words(pt, z=1):
    """An Edwards-BLS12 affine point -> one point of a window record: X, Y, T, Z as 8 u32 words each, radix 2^256."""
    X, Y, T, Z = pt[0] * z % R.Q, pt[1] * z % R.Q, pt[0] * pt[1] * z % R.Q, z % R.Q
    return [((v << 256) % R.Q >> (32 * i)) & 0xFFFFFFFF for v in (X, Y, T, Z) for i in range(8)]


def encode_records(records, form, points_per_record=16, z=lambda: 1, filler=None):
    """The model's points as the window records the host tail reads: `points_per_record` points each, the model's
    L + 1 first, then `filler` words (points beyond `planes` are unspecified: a tail that read them would show)."""
    import util

    out = []
    for rec in records:
        for i in range(points_per_record):
            if i < len(rec):
                if form == FORM_ED:
                    out += ed_record_point_words(rec[i], z())
                elif form == FORM_TE:
                    out += util.te_record_point_words(rec[i], z(), tag=(i == 0))
                else:
                    out += util.record_point_words(rec[i], z())
            else:
                out += list(filler) if filler is not None else [0xFFFFFFFF] * (32 if form == FORM_ED else 48)
    return np.array(out, dtype=np.uint32)
