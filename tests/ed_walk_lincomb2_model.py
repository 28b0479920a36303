"""Model of what a pass of the Edwards-BLS12 pairwise linear combination leaves behind (TEST INFRASTRUCTURE): both per-point
tables [1..8]P_i and [1..8]Q_i as exact MSM377_BASES_ED words and the walk's stash as projective points.  Big integers and
tests/pyref.py only, on tests/ed_walk_var_model.py (the table records) and tests/walk_model.py (the digits, the stash
checks).  Nothing here calls the engine.

The walk is modelled the way the kernel is specified, not the way the twin computes: the two final carries first
(acc = carry_a P + carry_b Q on acc = O), then for the 64 digit pairs from the top acc = 16 acc + da_w P + db_w Q with
|d| P and |d| Q taken from the two tables -- so a wrong table half, index, sign or carry shows as a wrong point."""
import pyref as R
import ed_walk_var_model as WVM
import walk_model as WM

ENTRIES = WVM.ENTRIES


def check_tables(words_p, words_q, ps, qs, where=""):
    """Table 0 against the P_i and table 1 against the Q_i, every record bit for bit."""
    WVM.check_tables(words_p, ps, where + "table 0 (p): ")
    WVM.check_tables(words_q, qs, where + "table 1 (q): ")


def _table(pt):
    table = [None, pt]
    for _ in range(2, ENTRIES + 1):
        table.append(R.ed_add(table[-1], pt))
    return table


def walk(p, q, a, b):
    """The point the joint walk of (a, b) over the tables of (p, q) ends at."""
    terms = [(_table(p),) + WM.var_digits(a), (_table(q),) + WM.var_digits(b)]
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


def check_stash(rows, products, ps, qs, as_, bs, lanes, where=""):
    """rows: (m, 36) u32 X, Y, T, Z; products: (m, 12).  Every row canonical with Z != 0, T Z = X Y and on the curve, the
    running products those of the rows; the rows at `lanes` decode to walk(P, Q, a, b)."""
    decoded = WM.check_ed_stash(rows, where)
    WM.check_products("Fq", rows, products, where)
    for i in lanes:
        exp = walk(ps[i], qs[i], as_[i], bs[i])
        assert decoded[i] == exp, "%slane %d: the stash holds %s, the model %s" % (where, i, decoded[i], exp)
    return decoded
