"""Inputs and expected values of the Edwards-BLS12 k-term linear combination tests (TEST INFRASTRUCTURE), shared by
tests/test_ed_batch_lincomb_host.py, tests/test_ed_batch_lincomb_gpu.py and tests/test_ed_batch_lincomb_node_gpu.py.

Term t of a case is draw t of tests/ed_curve_points.py (every class of curve point, planted at the lanes where a wave or a
block begins and ends; seeds differ from term to term) under the edge scalars of tests/ed_batch_mul_var_vectors.py, which
move SHIFT places on from term to term; a block of relations among the k points of one output is planted at REL_LANES.
Every expected value comes from tests/pyref.py (``R.ed_mul``, ``R.ed_add``, ``R.ed_neg``: the affine law, complete on the
curve).  Nothing here calls the engine's batch code."""
import functools
import random

import ed_batch_mul_var_vectors as VV
import ed_curve_points as EP
import pyref as R
from check_vectors import ed_low_order_points

ORD = R.ED_SUBGROUP
MASK256 = VV.MASK256
PASS = 1 << 16  # EDBL_PASS: the outputs of one pass, whatever k
MAX_TERMS = 8  # MSM377_LINCOMB_MAX_TERMS
IDENTITY_WIRE = VV.IDENTITY_WIRE
LANES = EP.LANES
SHIFT = 5  # term t's edge scalars run this many places ahead of term t - 1's
# First and last lane of the first waves, then lanes inside them: entry e of the relations block at REL_LANES[e], as far as
# n reaches.  The block has 6 + k entries (relations(k)): all of them fit from n = 256 on for every k.
REL_LANES = (0, 63, 64, 127, 128, 191, 192, 255, 32, 96, 160, 224, 31, 95, 159, 223, 256, 319, 320, 383)
FIXED = ("all terms the same point", "term j = -term 0, equal scalars", "multiples of one base, scalars sum to 0", "order 4 beside P + T", "all the identity", "all scalars 0")
SUM_IS_IDENTITY = ("multiples of one base, scalars sum to 0", "all the identity", "all scalars 0")


def relations(k):
    """The names of the block's entries for k terms: the fixed ones, then "scalar t = 0" for every term."""
    return FIXED + tuple("scalar %d = 0" % t for t in range(k))


def relate(e, rnd, pts, scs):
    """(points, scalars) of entry e of the block on one output's k terms: only what the relation dictates is replaced."""
    k = len(pts)
    pts, scs = list(pts), list(scs)
    t2, t4a, _ = ed_low_order_points()
    if e == 0:
        pts = [pts[0]] * k
    elif e == 1:  # a pair that cancels inside the sum (k = 1: nothing to pair with)
        j = 1 + rnd.randrange(k - 1) if k > 1 else 0
        if j:
            pts[j], scs[j] = R.ed_neg(pts[0]), scs[0]
    elif e == 2:  # O from k terms none of which is O (k = 1: [ORD]B)
        base = R.ed_mul(R.ED_G, rnd.randrange(2, ORD))
        mults = [1] + [rnd.randrange(2, 1 << 64) for _ in range(k - 1)]
        scs = [0] + [rnd.randrange(1, ORD) for _ in range(k - 1)]
        scs[0] = (-sum(s * m for s, m in zip(scs, mults))) % ORD or ORD
        pts = [R.ed_mul(base, m) for m in mults]
    elif e == 3:
        pts[0] = t4a
        if k > 1:
            pts[1] = R.ed_add(t4a, t2)
    elif e == 4:
        pts = [R.ED_ID] * k
    elif e == 5:
        scs = [0] * k
    else:
        scs[e - len(FIXED)] = 0
    return pts, scs


@functools.lru_cache(maxsize=None)
def case(n, k, seed=0):
    """(points, scalars, relations) of n outputs of k terms: points[t] and scalars[t] are term t's n-tuples -- draw
    MAX_TERMS * seed + t of every_curve_point, the edge scalars over LANES and the free indices behind them, moved SHIFT * t
    places on -- then the relations block at REL_LANES.  relations: lane -> name.  Cached: do not change the tuples."""
    points, scalars = [], []
    edges = VV.edge_scalars()
    for t in range(k):
        p, s = VV.case(n, MAX_TERMS * seed + t)
        p, s = list(p), list(s)
        _, _, planted, _ = EP.every_curve_point(n, MAX_TERMS * seed + t)
        at = [i for i in LANES if i < n] + [i for i in range(1, n) if i not in LANES and i not in planted]
        for j, i in enumerate(at[: len(edges)]):
            s[i] = edges[(j + SHIFT * t) % len(edges)]
        points.append(p), scalars.append(s)
    rnd = random.Random("ed batch lincomb relations/%d/%d/%d" % (n, k, seed))
    names, rel = relations(k), {}
    for e, lane in enumerate(REL_LANES[: len(names)]):
        if lane < n:
            pts, scs = relate(e, rnd, [p[lane] for p in points], [s[lane] for s in scalars])
            for t in range(k):
                points[t][lane], scalars[t][lane] = pts[t], scs[t]
            rel[lane] = names[e]
    return tuple(tuple(p) for p in points), tuple(tuple(s) for s in scalars), rel


def combine(pts, scs):
    """sum_t [s_t]P_t by pyref, the terms added in order."""
    acc = VV._mul(pts[0], scs[0])
    for p, s in zip(pts[1:], scs[1:]):
        acc = R.ed_add(acc, VV._mul(p, s))
    return acc


def expected(points, scalars, lanes=None):
    """Wire records by pyref, k R.ed_mul per output (about 20 ms each at full width), of all outputs or of `lanes`."""
    lanes = range(len(points[0])) if lanes is None else lanes
    return b"".join(R.ed_encode_result(combine([p[i] for p in points], [s[i] for s in scalars])) for i in lanes)


def encode(points, scalars):
    """(k point buffers, k scalar buffers)."""
    return [R.ed_encode_points(list(p)) for p in points], [R.encode_scalars(list(s)) for s in scalars]


def decode(record):
    """(x, y) of one 64-byte wire record."""
    return int.from_bytes(record[:32], "little"), int.from_bytes(record[32:64], "little")


def special_lanes(n, k):
    """The lanes of the case that hold a relation, a planted class at LANES or a low-order point in any term."""
    points, _, rel = case(n, k)
    low = [i for i in range(n) if any(0 in p[i] for p in points)]
    return sorted(set(rel) | {i for i in LANES if i < n} | set(low[:24]))


def boundary_case(n, k, progression=None):
    """(k point buffers, k scalar buffers, relations) around the pass boundary, n = PASS - 1, PASS or PASS + 1, on the scheme
    of ed_batch_lincomb2_vectors.boundary_case: k progressions of subgroup points, special_classes laid around index PASS in
    term t from PASS - 4 + t on; the relations block at PASS - 20 .. and again from PASS + 12 on (as far as n reaches);
    scalars below 2^16 everywhere except at LANES and at the two outputs either side of index PASS (full width: the
    one-thread twin stays at seconds).  progression(n, a0, d): the wire bytes of ed_curve_points.subgroup_points(n, a0, d)
    from a faster source; default: subgroup_points itself."""
    rnd = random.Random("ed batch lincomb boundary/%d/%d" % (n, k))
    gen = progression if progression else (lambda m, a0, d: R.ed_encode_points(EP.subgroup_points(m, a0, d)))
    arrays = [bytearray(gen(n, rnd.randrange(1, ORD), rnd.randrange(1, ORD))) for _ in range(k)]
    classes, _, _ = EP.special_classes(rnd)
    for t, arr in enumerate(arrays):
        for j, c in enumerate(classes):
            i = PASS - 4 + j + t
            if i < n:
                arr[64 * i : 64 * i + 64] = R.ed_encode_points([c])
    scalars = [[rnd.getrandbits(16) for _ in range(n)] for _ in range(k)]
    wide = [i for i in LANES + (PASS - 2, PASS - 1, PASS, PASS + 1) if i < n]
    fixed = [MASK256, ORD + 1, VV.nibbles(9), 2**255]
    for t in range(k):
        for i, s in zip(wide, fixed[t % 4 :] + VV.random_scalars("lk boundary %d" % t, len(wide))):
            scalars[t][i] = s
    names, rel = relations(k), {}
    for e, lane in enumerate(list(range(PASS - 20, PASS - 20 + len(names))) + list(range(PASS + 12, PASS + 12 + len(names)))):
        if lane < n:
            pts, scs = relate(e % len(names), rnd, [decode(arr[64 * lane : 64 * lane + 64]) for arr in arrays], [s[lane] | 1 for s in scalars])
            for t in range(k):
                arrays[t][64 * lane : 64 * lane + 64] = R.ed_encode_points([pts[t]])
                scalars[t][lane] = scs[t]
            rel[lane] = names[e % len(names)]
    return [bytes(a) for a in arrays], [R.encode_scalars(s) for s in scalars], rel


def off_curve_point():
    return VV.off_curve_point()


def expand(buf, size, n):
    """One element repeated n times: the expanded form of a stride-0 argument."""
    return buf[:size] * n
