"""Model of what a pass of the Edwards-BLS12 k-term linear combination leaves behind (TEST INFRASTRUCTURE): the k per-point
tables [1..8]P_ti as exact MSM377_BASES_ED words and the walk's stash as projective points.  Big integers and
tests/pyref.py only, on tests/ed_walk_var_model.py (the table records) and tests/walk_model.py (the digits, the stash
checks).  Nothing here calls the engine.

The walk is modelled the way the kernel is specified, not the way the twin computes: the k final carries first
(acc = sum_t carry_t P_t on acc = O), then for the 64 steps from the top acc = 16 acc + sum_t d_tw P_t, the terms in order,
with |d| P_t taken from table t -- so a wrong table, index, sign or carry shows as a wrong point."""
import pyref as R
import ed_walk_var_model as WVM
import walk_model as WM

ENTRIES = WVM.ENTRIES


def check_tables(words, points, where=""):
    """words[t]: the (8, m, 32) read-back of table t; points[t]: term t's m input points.  Every record bit for bit."""
    assert len(words) == len(points)
    for t, (w, pts) in enumerate(zip(words, points)):
        WVM.check_tables(w, pts, "%stable %d: " % (where, t))


def _table(pt):
    table = [None, pt]
    for _ in range(2, ENTRIES + 1):
        table.append(R.ed_add(table[-1], pt))
    return table


def walk(pts, scs):
    """The point the joint walk of the scalars scs over the tables of the points pts ends at."""
    terms = [(_table(p),) + WM.var_digits(s) for p, s in zip(pts, scs)]
    acc = R.ED_ID
    for table, _, carry in terms:  # step 64: the carries, no doublings
        if carry:
            acc = R.ed_add(acc, table[1])
    for w in reversed(range(64)):
        for _ in range(4):
            acc = R.ed_add(acc, acc)
        for table, digits, _ in terms:
            d = digits[w]
            if d:
                acc = R.ed_add(acc, R.ed_neg(table[-d]) if d < 0 else table[d])
    return acc


def check_stash(rows, products, points, scalars, lanes, where=""):
    """rows: (m, 36) u32 X, Y, T, Z; products: (m, 12).  Every row canonical with Z != 0, T Z = X Y and on the curve, the
    running products those of the rows; the rows at `lanes` decode to walk() of that output's k terms."""
    decoded = WM.check_ed_stash(rows, where)
    WM.check_products("Fq", rows, products, where)
    for i in lanes:
        exp = walk([p[i] for p in points], [s[i] for s in scalars])
        assert decoded[i] == exp, "%slane %d: the stash holds %s, the model %s" % (where, i, decoded[i], exp)
    return decoded
