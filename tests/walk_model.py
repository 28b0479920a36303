"""Model of what the batch calls' walk kernels leave in the stash (TEST INFRASTRUCTURE, pure Python integers).

k_bm_accumulate, k_bmm_accumulate, k_cr_accumulate / k_cr_fold, k_bmv_table / k_bmv_accumulate, k_bl2_accumulate and
k_edbm_accumulate (csrc/kernels/) each store one projective point per output; k_bm_up / k_edbm_up put the exclusive running
products beside them.  msm377_read_walk_stash and msm377_g1_read_walk_tables copy both out; this module says what they must
hold:
    signed_digits      the digit list of a scalar at width c, from the scalar's integer value alone
    check_g1_stash     box, identity form, invariant and the decoded affine point of every XYZZ stash row
    check_ed_stash     the same for the extended Edwards rows
    check_products     the running products of a pass
    entry_words        the record [e]P_i of a per-point table, bit for bit
    walk_events        which exceptional events the walk of a case meets, from the model alone
The boxes are tools/check_lazy_bounds.py's, through lazy_model.FieldModel and normalise_model.stash_shapes -- the table
tests/test_normalise_gpu.py draws its corner operands from.  tests/test_walk_model_host.py pins everything here on the CPU.
"""
import functools

import numpy as np

import lazy_model as M
import normalise_model as NM
import pyref as R
import record_model as RM

r = R.R_ORDER
THREADS, PER_THREAD, BLOCK = NM.THREADS, NM.PER_THREAD, NM.BLOCK
VAR_WIDTH, VAR_ENTRIES = 4, 8  # BMV_WIDTH, BMV_ENTRIES

EVENTS = (
    "O from a zero scalar",
    "O from a non-zero scalar on a base of small order",
    "acc = O in mid-walk, then a non-zero digit",
    "acc = +entry",
    "acc = -entry",
    "a flagged table entry skipped",
    "the carry row taken",
    "the digit +2^(c-1)",
)
(EV_ZERO_O, EV_SMALL_O, EV_MID_O, EV_EQUAL, EV_OPPOSITE, EV_FLAGGED, EV_CARRY, EV_HALF) = EVENTS


# ------------------------------------------------------------------ digits ----

def windows(c):
    return (256 + c - 1) // c


def signed_digits(s, c):
    """(digits, carry) of s in [0, 2^256) at width c: W = ceil(256 / c) digits in -(2^(c-1) - 1) .. 2^(c-1), low window
    first, with s = sum_w d_w 2^(c w) + carry 2^(c W).  d_w is THE residue of what is left mod 2^c in that range -- no carry
    variable, no window extraction: nothing of bm_digit (csrc/batch_mul_recode.hpp) is restated here."""
    assert 0 <= s < 1 << 256
    half, full = 1 << (c - 1), 1 << c
    digits, rest = [], s
    for _ in range(windows(c)):
        d = rest % full
        if d > half:
            d -= full
        digits.append(d)
        rest = (rest - d) // full  # exact
    assert rest in (0, 1)
    return digits, rest


def var_digits(s):
    """The 64 signed 4-bit digits -7 .. 8 and the carry of the variable-base and pairwise walks."""
    return signed_digits(s, VAR_WIDTH)


def crafted_scalars(c):
    """[(label, s)]: the scalars every walk case is given, at width c."""
    half = 1 << (c - 1)
    out = [("0", 0), ("1", 1), ("2^(c-1)", half), ("2^(c-1) + 1", half + 1), ("2^c - 1", (1 << c) - 1), ("2^c", 1 << c),
           ("2^256 - 1", 2**256 - 1), ("2^256 - 2^(c-1)", 2**256 - half), ("2^255", 2**255),
           ("r - 1", r - 1), ("r", r), ("r + 1", r + 1), ("a 64-bit value", 0xF123456789ABCDE7)]
    return out


# ------------------------------------------------------------------ fields and boxes ----

@functools.lru_cache(maxsize=None)
def field(name):
    return M.FieldModel(name)


@functools.lru_cache(maxsize=None)
def stash_boxes(name):
    """[(coordinate, record_model.Box)] in stash order: NORMALISATION_OPERANDS of tools/check_lazy_bounds.py over its
    shapes() -- the table normalise_model.stash_shapes reads (whose "canonical" is the generator's strict sub-box; the
    contract is the proof's own: every limb carry-normalised, the value below the modulus)."""
    B = M.B
    B.use_field(name)
    try:
        t = B.shapes()
        out = [(c, RM.Box(s, tuple(t[s].limbs), t[s].hi)) for c, s in B.NORMALISATION_OPERANDS[name].items()]
    finally:
        B.use_field("Fp")
    assert [c for c, _ in out] == [c for c, _ in NM.stash_shapes(field(name))]
    return out


def one_limbs(name):
    fm = field(name)
    return M.nform_limbs(fm.R % fm.P, fm.N)


def g1_identity_words():
    """G1::identity() as the stash holds it: X = 0, Y = the Montgomery 1, ZZ = ZZZ = 0."""
    return [0] * 13 + one_limbs("Fp") + [0] * 26


def _fail(where, i, text):
    raise AssertionError("%sstash point %d: %s" % (where, i, text))


def _check_boxes(name, rows, where):
    fm = field(name)
    rows = np.asarray(rows, dtype=np.uint32)
    for c, (coord, box) in enumerate(stash_boxes(name)):
        arr = rows[:, fm.N * c : fm.N * c + fm.N]
        bad = np.flatnonzero(~box.accepts(arr))
        if bad.size:
            _fail(where, int(bad[0]), "%s outside the %s box (limbs %s); %d of %d points are" % (coord, box.name, [hex(int(x)) for x in arr[bad[0]]], bad.size, len(rows)))


def check_g1_stash(rows, where=""):
    """rows: (m, 52) u32.  Every limb and value of X inside stored_x, of Y, ZZ, ZZZ inside stored; an identity is the words
    of G1::identity() exactly; a live point has ZZ and ZZZ non-zero mod p, ZZ^3 = ZZZ^2 and lies on the curve.  Returns the
    affine point (or None) of every row."""
    fp = field("Fp")
    assert [c for c, _ in stash_boxes("Fp")] == ["X", "Y", "ZZ", "ZZZ"] and [b.name for _, b in stash_boxes("Fp")] == ["stored_x", "stored", "stored", "stored"]
    rows = np.asarray(rows, dtype=np.uint32)
    assert rows.ndim == 2 and rows.shape[1] == 52
    _check_boxes("Fp", rows, where)
    p, ident = fp.P, g1_identity_words()
    out = []
    for i, row in enumerate(rows.tolist()):
        X, Y, ZZ, ZZZ = (M.value(row[13 * c : 13 * c + 13]) for c in range(4))
        if not any(row[26:39]) or not any(row[39:52]) or ZZ % p == 0 or ZZZ % p == 0:
            if row != ident:
                _fail(where, i, "ZZ or ZZZ is zero (limb by limb or mod p) but the words are not G1::identity(): X %#x Y %#x ZZ %#x ZZZ %#x" % (X, Y, ZZ, ZZZ))
            out.append(None)
            continue
        if (ZZ * ZZ * ZZ * fp.Rinv - ZZZ * ZZZ) % p:  # ((ZZ / R)^3 = (ZZZ / R)^2) R^2
            _fail(where, i, "ZZ^3 != ZZZ^2")
        pt = (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)
        if not R.on_curve(pt):
            _fail(where, i, "the decoded point is not on the curve")
        out.append(pt)
    return out


def check_ed_stash(rows, where=""):
    """rows: (m, 36) u32.  X, Y, T, Z canonical, Z non-zero, T Z = X Y; returns (x, y) = (X / Z, Y / Z) of every row."""
    fq = field("Fq")
    assert [b.name for _, b in stash_boxes("Fq")] == ["canonical"] * 4
    rows = np.asarray(rows, dtype=np.uint32)
    assert rows.ndim == 2 and rows.shape[1] == 36
    _check_boxes("Fq", rows, where)
    q = fq.P
    out = []
    for i, row in enumerate(rows.tolist()):
        X, Y, T, Z = (M.value(row[9 * c : 9 * c + 9]) for c in range(4))
        if max(X, Y, T, Z) >= q:
            _fail(where, i, "a coordinate is not below q")
        if Z == 0:
            _fail(where, i, "Z = 0")
        if (T * Z - X * Y) % q:
            _fail(where, i, "T Z != X Y")
        zi = pow(Z, -1, q)
        pt = (X * zi % q, Y * zi % q)
        if not R.ed_on_curve(pt):
            _fail(where, i, "the decoded point is not on the curve")
        out.append(pt)
    return out


def check_products(name, rows, products, where=""):
    """The exclusive running products of a pass.  rows: the (m, 4 N) stash points; products: (m, N + 3).  For thread tid of
    workgroup blk, with outputs blk * 1024 + j * 256 + tid, j < 4: C_0 is the words of one() exactly; C_(j+1) = C_j z_j / R
    mod p with z_j the stored ZZZ (Z) of output j, or one for an identity (ZZZ zero limb by limb: the one test k_bm_up makes);
    every C inside `stored` (Fq::mul: canonical); the pad words zero."""
    fm = field(name)
    n = fm.N
    rows, products = np.asarray(rows, dtype=np.uint32), np.asarray(products, dtype=np.uint32)
    m = len(rows)
    assert products.shape == (m, n + 3) and rows.shape == (m, 4 * n)
    bad = np.flatnonzero(products[:, n:].any(axis=1))
    if bad.size:
        _fail(where, int(bad[0]), "running product: pad words not zero")
    box = RM.boxes(name)["stored" if name == "Fp" else "canonical"]
    bad = np.flatnonzero(~box.accepts(products[:, :n]))
    if bad.size:
        _fail(where, int(bad[0]), "running product outside the %s box (limbs %s)" % (box.name, [hex(int(x)) for x in products[bad[0], :n]]))
    one = one_limbs(name)
    z, c = rows[:, 3 * n :].tolist(), products[:, :n].tolist()
    for i in range(m):
        if (i % BLOCK) // THREADS == 0:
            if c[i] != one:
                _fail(where, i, "running product of a thread's first output is not one(): %s" % [hex(x) for x in c[i]])
            continue
        prev = i - THREADS
        zv = M.value(z[prev]) if any(z[prev]) else fm.R
        if (M.value(c[prev]) * zv * fm.Rinv - M.value(c[i])) % fm.P:
            _fail(where, i, "running product is not C z / R of output %d" % prev)


# ------------------------------------------------------------------ per-point tables ----

def entry_words(pt, e):
    """The record [e]P of a per-point table: canonical x, canonical y, flag 0; x = y = 0 with flag 1 where [e]P = O or the
    input was flagged (pt None); pad words zero."""
    return RM.table_record_words(None if pt is None else R.mul(pt, e))


def check_table(words, points, where=""):
    """words: (8, m, 32) u32 of one per-point table; points: the m input points (None: flagged).  Every record, bit for bit;
    a failure names the entry."""
    words = np.asarray(words, dtype=np.uint32)
    assert words.shape == (VAR_ENTRIES, len(points), 32)
    RM.check_table_boxes(words.reshape(-1, 32), where)
    for i, pt in enumerate(points):
        acc = None
        for e in range(1, VAR_ENTRIES + 1):
            acc = None if pt is None else R.add(acc, pt)
            got, exp = words[e - 1, i].tolist(), RM.table_record_words(acc)
            if got != exp:
                raise AssertionError("%sentry [%d]P of point %d: %s, model %s" % (where, e, i, [hex(x) for x in got[:27]], [hex(x) for x in exp[:27]]))


# ------------------------------------------------------------------ the walks, on affine points ----

@functools.lru_cache(maxsize=None)
def _row_bases(base, c):
    return tuple(RM.window_points(base, [c] * (windows(c) + 1)))


@functools.lru_cache(maxsize=1 << 16)
def _entry(base, c, w, d):
    rb = _row_bases(base, c)[w]
    return None if rb is None else R.mul(rb, d)


def _madd(acc, entry, negative, events, started):
    """One step of a walk on affine points: the events madd's exits stand for.  (acc, an addition was made)."""
    if entry is None:
        events.add(EV_FLAGGED)
        return acc, started
    if negative:
        entry = R.neg(entry)
    if acc is None:
        if started:
            events.add(EV_MID_O)
    elif acc == entry:
        events.add(EV_EQUAL)
    elif acc == R.neg(entry):
        events.add(EV_OPPOSITE)
    return R.add(acc, entry), True


def walk_fixed(bases, scalars, c, acc=None):
    """The low-to-high walk of k_bm_accumulate / k_bmm_accumulate / k_cr_accumulate over the tables of `bases` in order into
    one accumulator: (point, events)."""
    events, started = set(), False
    for base, s in zip(bases, scalars):
        digits, carry = signed_digits(s, c)
        for w, d in enumerate(digits + [carry]):
            if d == 0:
                continue
            if w == windows(c):
                events.add(EV_CARRY)
            if d == 1 << (c - 1):
                events.add(EV_HALF)
            acc, started = _madd(acc, _entry(base, c, w, abs(d)), d < 0, events, started)
    return acc, events


def walk_var(terms):
    """The high-to-low walk of k_bmv_accumulate (one term) and k_bl2_accumulate (two): terms = [(point or None, scalar)];
    a final carry is a leading digit 1.  (point, events)."""
    events, started, acc = set(), False, None
    lists = []
    for pt, s in terms:
        digits, carry = var_digits(s)
        if carry:
            events.add(EV_CARRY)
        lists.append([carry] + digits[::-1])
    for step in range(windows(VAR_WIDTH) + 1):
        for _ in range(VAR_WIDTH):
            acc = R.add(acc, acc)
        for (pt, _), digits in zip(terms, lists):
            d = digits[step]
            if d == 0:
                continue
            if d == 1 << (VAR_WIDTH - 1):
                events.add(EV_HALF)
            acc, started = _madd(acc, None if pt is None else R.mul(pt, abs(d)), d < 0, events, started)
    return acc, events


def small_order(pt):
    return pt is not None and R.mul(pt, 12) is None


@functools.lru_cache(maxsize=None)
def lane_events(kind, c, bases, scalars):
    """(expected output point, events) of one crafted lane.  kind: "fixed" (bases: the k bases; scalars: the k scalars of
    the row) or "var" (bases: the lane's one or two points, None for a flagged one).  Tuples in, kept: the cases share lanes."""
    if kind == "fixed":
        pt, ev = walk_fixed(bases, scalars, c)
        direct = None
        for b, s in zip(bases, scalars):
            direct = R.add(direct, R.mul(b, s))
    else:
        pt, ev = walk_var(list(zip(bases, scalars)))
        direct = None
        for b, s in zip(bases, scalars):
            direct = R.add(direct, None if b is None else R.mul(b, s))
    assert pt == direct, "the digit walk and the direct sum disagree: a mistake in the model"
    if pt is None:
        if not any(scalars):
            ev.add(EV_ZERO_O)
        elif any(s and small_order(b) for b, s in zip(bases, scalars)):
            ev.add(EV_SMALL_O)
    return pt, frozenset(ev)


def walk_events(case):
    """The union of the events over the crafted lanes of a case: {"kind", "c", "lanes": [(bases, scalars)]}
    (tests/walk_cases.py events_of builds it from a case; a row commitment: one lane per segment of a row)."""
    out = set()
    for bases, scalars in case["lanes"]:
        out |= lane_events(case["kind"], case["c"], tuple(bases), tuple(scalars))[1]
    return out


# ------------------------------------------------------------------ Edwards-BLS12 ----

def ed_expected(bases, scalars):
    acc = R.ED_ID
    for b, s in zip(bases, scalars):
        acc = R.ed_add(acc, R.ed_mul(b, s))
    return acc


def ed_events(scalars, c):
    """The complete law has no exits; what a lane can still meet is the recode's: the carry row and the digit +2^(c-1)."""
    out = set()
    for s in scalars:
        digits, carry = signed_digits(s, c)
        if carry:
            out.add(EV_CARRY)
        if 1 << (c - 1) in digits:
            out.add(EV_HALF)
    return out
