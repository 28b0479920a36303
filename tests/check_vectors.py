"""Crafted inputs of the point-validation tests (TEST INFRASTRUCTURE): wire records with known verdicts.

Every expected value comes from tests/pyref.py alone (``on_curve``, ``mul(pt, R_ORDER) is None``, ``ed_on_curve``,
``ed_mul(pt, ED_SUBGROUP) == ED_ID``); nothing here calls the engine."""
import os
import sys

import pyref as R
import util

CANONICAL, CURVE, SUBGROUP, ALL = 1, 2, 4, 7
NONE = 2**64 - 1  # first_bad of a clean report in the C struct


def _gen_consts():
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import gen_consts

    return gen_consts


def g1_verdict(x, y):
    """0 = valid, else the CHECK_* bit of the first class the pair fails."""
    if x >= R.P or y >= R.P:
        return CANONICAL
    if not R.on_curve((x, y)):
        return CURVE
    return 0 if R.mul((x, y), R.R_ORDER) is None else SUBGROUP


def ed_verdict(x, y):
    if x >= R.Q or y >= R.Q:
        return CANONICAL
    if not R.ed_on_curve((x, y)):
        return CURVE
    return 0 if R.ed_mul((x, y), R.ED_SUBGROUP) == R.ED_ID else SUBGROUP


def g1_small_order_points():
    """The three points of order 2, the two of order 3 (x = 0), one of order 4 and one of order 6."""
    gc = _gen_consts()
    tp = util.t_prime()
    omega = (-tp[0]) % R.P
    t2 = [(R.P - 1, 0), tp, ((-omega * omega) % R.P, 0)]
    t3 = [(0, 1), (0, R.P - 1)]
    te = util.te_params()
    x4 = (-1 - pow(te["s"], -1, R.P)) % R.P
    t4 = (x4, gc._sqrt_p((x4**3 + 1) % R.P))
    assert R.add(t4, t4) == (R.P - 1, 0)
    t6 = R.add(t2[0], t3[0])
    for t in t2:
        assert R.on_curve(t) and R.add(t, t) is None
    for t in t3:
        assert R.on_curve(t) and R.mul(t, 3) is None
    return t2 + t3 + [t4, t6]


def g1_lifted_points(count, seed=0x11F7):
    """Curve points lifted from x: outside the subgroup with overwhelming probability (the cofactor is ~2^125)."""
    gc = _gen_consts()
    out, g = [], R.splitmix64(seed)
    while len(out) < count:
        x = 0
        for k in range(6):
            x |= next(g) << (64 * k)
        x %= R.P
        rhs = (x**3 + 1) % R.P
        if pow(rhs, (R.P - 1) // 2, R.P) == 1:
            out.append((x, gc._sqrt_p(rhs)))
    return out


def g1_crafted():
    """(wire bytes, list of verdicts): ~64 G1 records."""
    recs = []
    valid = [R.G, R.FIXED_BASE] + [R.mul(R.G, k) for k in (2, 3, 0xDEADBEEF, R.R_ORDER - 1, 0x1234567890ABCDEF1234567890ABCDEF)]
    gx, gy = R.G
    recs += [(R.P, gy), (gx, R.P + 5), (2**384 - 1, gy), (gx, 2**384 - 1), (2**377, 2**377), (R.P + gx, gy)]  # non-canonical (the last: a valid point plus p)
    recs += [(R.P + 1, 1)]  # non-canonical AND, reduced mod p, off the curve: counted once, as non-canonical
    recs += [(1, 1), (gx, gy ^ 1), (gx, gy ^ (1 << 200)), (gx ^ (1 << 376), gy), (0, 0), (gx, 0), (R.P - 1, R.P - 1)]  # off the curve
    small = g1_small_order_points()
    recs += small
    lifted = g1_lifted_points(6)
    recs += lifted
    for i, t in enumerate(small):  # P + T, P in the subgroup
        recs.append(R.add(valid[i % len(valid)], t))
    recs.append(R.add(R.mul(R.G, 77), lifted[0]))
    recs += valid
    recs += [R.neg(v) for v in valid]
    recs += [R.mul(R.G, k) for k in R.rand_scalars(0xC4EC, 12)]
    # interleave: a bad point first and last would hide ordering mistakes, so rotate a valid one to the front
    recs = [valid[0]] + recs
    verdicts = [g1_verdict(x, y) for x, y in recs]
    blob = b"".join(x.to_bytes(48, "little") + y.to_bytes(48, "little") for x, y in recs)
    return blob, verdicts


def ed_low_order_points():
    i = R._sqrt_mod_q(R.Q - 1)
    pts = [(0, R.Q - 1), (i, 0), (R.Q - i, 0)]
    for t in pts:
        assert R.ed_on_curve(t) and R.ed_mul(t, 4) == R.ED_ID and t != R.ED_ID
    return pts


def ed_lifted_points(count, seed=0xED17):
    """Curve points lifted from x, either root of y: about three in four are outside the prime-order subgroup."""
    out, g = [], R.splitmix64(seed)
    while len(out) < count:
        x = 0
        for k in range(4):
            x |= next(g) << (64 * k)
        x %= R.Q
        xx = x * x % R.Q
        y2 = (R.ED_A * xx - 1) * pow(R.ED_D * xx - 1, -1, R.Q) % R.Q
        y = R._sqrt_mod_q(y2)
        if y is not None:
            out.append((x, y if len(out) % 2 else (-y) % R.Q))
    return out


def ed_crafted():
    gx, gy = R.ED_G
    valid = [R.ED_G] + [R.ed_mul(R.ED_G, k) for k in (2, 3, 0xDEADBEEF, R.ED_SUBGROUP - 1)] + [R.ed_point_from_x(R.ed_mul(R.ED_G, 5)[0])]
    recs = [valid[0]]
    recs += [(R.Q, gy), (gx, R.Q + 5), (2**256 - 1, gy), (gx, 2**256 - 1), (R.Q + gx, gy)]
    recs += [(R.Q + 1, 1)]  # non-canonical and off the curve
    recs += [(1, 1), (gx, gy ^ 1), (gx ^ (1 << 250), gy), (0, 0), (gx, 0), (gy, gx)]
    low = ed_low_order_points()
    recs += [R.ED_ID] + low  # the wire format CAN write the Edwards identity: (0, 1) is in the subgroup
    recs += ed_lifted_points(8)
    for i, t in enumerate(low):
        recs.append(R.ed_add(valid[i % len(valid)], t))
    recs += valid[1:]
    recs += [R.ed_neg(v) for v in valid]
    recs += [R.ed_mul(R.ED_G, k) for k in R.rand_scalars(0xEDC4, 10, R.ED_SUBGROUP)]
    verdicts = [ed_verdict(x, y) for x, y in recs]
    blob = b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in recs)
    return blob, verdicts


def expected_report(verdicts, flags):
    """(checked, noncanonical, off_curve, outside_subgroup, first_bad or None, first_bad_reason) under ``flags``
    (normalised: 1, 3 or 7): a class that is not asked for does not count."""
    norm = ALL if flags & SUBGROUP else (CANONICAL | CURVE) if flags & CURVE else CANONICAL
    seen = [v if (v & norm) else 0 for v in verdicts]
    first = next((i for i, v in enumerate(seen) if v), None)
    return (len(verdicts), seen.count(CANONICAL), seen.count(CURVE), seen.count(SUBGROUP), first, seen[first] if first is not None else 0)


def as_tuple(report):
    """A host.engine.CheckReport as the tuple expected_report builds."""
    return (report.checked, report.noncanonical, report.off_curve, report.outside_subgroup, report.first_bad, report.first_bad_reason)
