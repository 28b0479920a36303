"""Inputs and expected values of the Edwards-BLS12 pairwise linear combination tests (TEST INFRASTRUCTURE), shared by
tests/test_ed_batch_lincomb2_host.py, tests/test_ed_batch_lincomb2_gpu.py and tests/test_ed_batch_lincomb2_node_gpu.py.

Both point arrays are those of tests/ed_curve_points.py (every class of curve point, planted at the lanes where a wave or a
block begins and ends), drawn with different seeds; both scalar arrays carry the edge scalars of
tests/ed_batch_mul_var_vectors.py, shifted against each other; a block of relations between the two arrays is planted at the
lanes where a wave begins and ends.  Every expected value comes from tests/pyref.py (``R.ed_mul``, ``R.ed_add``,
``R.ed_neg``: the affine law, complete on the curve).  Nothing here calls the engine's batch code."""
import functools
import random

import ed_batch_mul_var_vectors as VV
import ed_curve_points as EP
import pyref as R
from check_vectors import ed_low_order_points

ORD = R.ED_SUBGROUP
MASK256 = VV.MASK256
PASS = 1 << 16  # EDBL2_PASS: the pairs of one pass
IDENTITY_WIRE = VV.IDENTITY_WIRE
LANES = EP.LANES
SHIFT = 5  # b's edge scalars run this many places ahead of a's
# first and last lane of the first waves: relation j % 8 at REL_LANES[j], as far as n reaches (all eight from n = 256)
REL_LANES = (0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511)
RELATIONS = ("Q = P", "Q = -P, a = b", "Q = [m]P, a + b m = 0", "P of order 4, Q = P + T", "both the identity", "a = 0", "b = 0", "a = b = 0")


def relate(j, rnd, p, q, a, b):
    """(P, Q, a, b) of relation j on the pair (p, q, a, b): only what the relation dictates is replaced."""
    t2, t4a, _ = ed_low_order_points()
    if j == 0:
        return p, p, a, b
    if j == 1:
        return p, R.ed_neg(p), a, a
    if j == 2:  # O from two terms that are not O
        base, m, bb = R.ed_mul(R.ED_G, rnd.randrange(2, ORD)), rnd.randrange(2, 1 << 64), rnd.randrange(1, ORD)
        return base, R.ed_mul(base, m), (-bb * m) % ORD, bb
    if j == 3:
        return t4a, R.ed_add(t4a, t2), a, b
    if j == 4:
        return R.ED_ID, R.ED_ID, a, b
    return p, q, (0 if j in (5, 7) else a), (0 if j in (6, 7) else b)


@functools.lru_cache(maxsize=None)
def case(n, seed=0):
    """(P, Q, a, b, relations) of n pairs: two draws of every_curve_point, the edge scalars over LANES and the free indices
    behind them in both scalar arrays (b's SHIFT places ahead of a's), then the relations block at REL_LANES.  relations:
    lane -> name.  Cached: do not change the tuples."""
    p, a = VV.case(n, 2 * seed)
    q, b = VV.case(n, 2 * seed + 1)
    p, q, a, b = list(p), list(q), list(a), list(b)
    _, _, planted, _ = EP.every_curve_point(n, 2 * seed + 1)
    edges = VV.edge_scalars()
    at = [i for i in LANES if i < n] + [i for i in range(1, n) if i not in LANES and i not in planted]
    for k, i in enumerate(at[: len(edges)]):
        b[i] = edges[(k + SHIFT) % len(edges)]
    rnd = random.Random("ed batch lincomb2 relations/%d/%d" % (n, seed))
    relations = {}
    for j, lane in enumerate(REL_LANES):
        if lane < n:
            p[lane], q[lane], a[lane], b[lane] = relate(j % 8, rnd, p[lane], q[lane], a[lane], b[lane])
            relations[lane] = RELATIONS[j % 8]
    return tuple(p), tuple(q), tuple(a), tuple(b), relations


def combine(p, q, a, b):
    """[a]P + [b]Q by pyref."""
    return R.ed_add(VV._mul(p, a), VV._mul(q, b))


def expected(ps, qs, as_, bs):
    """Wire records by pyref, two R.ed_mul and one R.ed_add per output (about 40 ms each at full width)."""
    return b"".join(R.ed_encode_result(combine(*t)) for t in zip(ps, qs, as_, bs))


def encode(ps, qs, as_, bs):
    return R.ed_encode_points(list(ps)), R.ed_encode_points(list(qs)), R.encode_scalars(list(as_)), R.encode_scalars(list(bs))


def decode(record):
    """(x, y) of one 64-byte wire record."""
    return int.from_bytes(record[:32], "little"), int.from_bytes(record[32:64], "little")


def special_lanes(n):
    """The lanes of the n-pair case that hold a relation, a planted class at LANES or a low-order point in either array."""
    p, q, _, _, relations = case(n)
    low = [i for i in range(n) if 0 in p[i] or 0 in q[i]]
    return sorted(set(relations) | {i for i in LANES if i < n} | set(low[:24]))


def boundary_case(n, progression=None):
    """(p, q, a, b bytes, relations) around the pass boundary, n = PASS - 1, PASS or PASS + 1, on the scheme of
    ed_batch_mul_var_vectors.boundary_case with PASS = 2^16: two progressions of subgroup points, special_classes laid around
    index PASS in p and, one place on, in q; the relations block at PASS - 12 .. PASS - 5 and again at PASS + 3 .. (as far as n
    reaches); scalars below 2^16 everywhere except at LANES and at the two pairs either side of index PASS (full width: the
    one-thread twin stays at seconds).  progression(n, a0, d): the wire bytes of ed_curve_points.subgroup_points(n, a0, d)
    from a faster source; default: subgroup_points itself."""
    rnd = random.Random("ed batch lincomb2 boundary/%d" % n)
    gen = progression if progression else (lambda m, a0, d: R.ed_encode_points(EP.subgroup_points(m, a0, d)))
    arrays = [bytearray(gen(n, rnd.randrange(1, ORD), rnd.randrange(1, ORD))) for _ in range(2)]
    classes, _, _ = EP.special_classes(rnd)
    for t, arr in enumerate(arrays):
        for j, c in enumerate(classes):
            i = PASS - 4 + j + t  # PASS - 4 .. PASS + 3
            if i < n:
                arr[64 * i : 64 * i + 64] = R.ed_encode_points([c])
    a, b = [rnd.getrandbits(16) for _ in range(n)], [rnd.getrandbits(16) for _ in range(n)]
    wide = [i for i in LANES + (PASS - 2, PASS - 1, PASS, PASS + 1) if i < n]
    fixed = [MASK256, ORD + 1, VV.nibbles(9), 2**255]
    for i, s, t in zip(wide, fixed + VV.random_scalars("l2 boundary a", len(wide)), fixed[2:] + VV.random_scalars("l2 boundary b", len(wide))):
        a[i], b[i] = s, t
    relations = {}
    for j, lane in enumerate(list(range(PASS - 12, PASS - 4)) + list(range(PASS + 4, PASS + 12))):
        if lane < n:
            pq = [decode(arr[64 * lane : 64 * lane + 64]) for arr in arrays]
            pp, qq, a[lane], b[lane] = relate(j % 8, rnd, pq[0], pq[1], a[lane] | 1, b[lane] | 1)
            arrays[0][64 * lane : 64 * lane + 64] = R.ed_encode_points([pp])
            arrays[1][64 * lane : 64 * lane + 64] = R.ed_encode_points([qq])
            relations[lane] = RELATIONS[j % 8]
    return bytes(arrays[0]), bytes(arrays[1]), R.encode_scalars(a), R.encode_scalars(b), relations


def off_curve_point():
    return VV.off_curve_point()


def expand(buf, size, n):
    """One element repeated n times: the expanded form of a stride-0 argument."""
    return buf[:size] * n
