"""Model of what a pass of the Edwards-BLS12 variable-base call leaves behind (TEST INFRASTRUCTURE): the per-point tables
[1..8]P_i as exact MSM377_BASES_ED words and the walk's stash as projective points.  Big integers and tests/pyref.py only;
the digits are walk_model.var_digits (the residue definition, nothing of bm_digit restated), the record words
record_model.ed_make_base, the stash checks walk_model.check_ed_stash / check_products.  Nothing here calls the engine.

The walk itself is modelled the way the kernel is specified, not the way the twin multiplies: acc = carry ? P : O, then for
the 64 digits from the top acc = 16 acc + d_w P with |d_w| P taken from the table -- so a wrong table index, sign or carry
start shows as a wrong point even where the call's output bytes would be compared elsewhere."""
import numpy as np

import pyref as R
import record_model as RM
import walk_model as WM

ENTRIES = 8
REC_WORDS = 32


def check_tables(words, points, where=""):
    """words: (8, m, 32) u32; points: the m input points.  Record [e]P: (y - x)[9], (y + x)[9], (2 d x y)[9] canonical
    Montgomery limbs, 5 zero words; the identity is the ordinary record (1, 1, 0).  Every record, bit for bit; a failure
    names the entry."""
    words = np.asarray(words, dtype=np.uint32)
    assert words.shape == (ENTRIES, len(points), REC_WORDS), words.shape
    for i, pt in enumerate(points):
        acc = R.ED_ID
        for e in range(1, ENTRIES + 1):
            acc = R.ed_add(acc, pt)
            ymx, ypx, kt = RM.ed_make_base(acc)
            got, exp = words[e - 1, i].tolist(), ymx + ypx + kt + [0] * 5
            if got != exp:
                raise AssertionError("%sentry [%d]P of point %d: %s, model %s" % (where, e, i, [hex(x) for x in got[:27]], [hex(x) for x in exp[:27]]))


def walk(pt, s):
    """The point the walk of scalar s over the table of pt ends at."""
    digits, carry = WM.var_digits(s)
    table = [None]
    for e in range(1, ENTRIES + 1):
        table.append(R.ed_add(table[-1], pt) if e > 1 else pt)
    acc = pt if carry else R.ED_ID
    for d in reversed(digits):
        for _ in range(4):
            acc = R.ed_add(acc, acc)
        if d:
            entry = table[abs(d)]
            acc = R.ed_add(acc, R.ed_neg(entry) if d < 0 else entry)
    return acc


def check_stash(rows, products, points, scalars, lanes, where=""):
    """rows: (m, 36) u32 X, Y, T, Z; products: (m, 12).  Every row canonical with Z != 0, T Z = X Y and on the curve, the
    running products those of the rows; the rows at `lanes` decode to walk(point, scalar)."""
    decoded = WM.check_ed_stash(rows, where)
    WM.check_products("Fq", rows, products, where)
    for i in lanes:
        exp = walk(points[i], scalars[i])
        assert decoded[i] == exp, "%slane %d: the stash holds %s, the model %s" % (where, i, decoded[i], exp)
    return decoded
