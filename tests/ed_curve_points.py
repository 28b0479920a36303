"""Edwards-BLS12 inputs beyond the prime-order subgroup (TEST INFRASTRUCTURE; pyref and check_vectors only, nothing of the
engine).  The curve has cofactor 4 and a complete addition law, so every curve point is a legal input of an MSM: the
identity (0, 1), the point of order 2 (0, -1), the two points of order 4 (+-i, 0) and P + T for each low-order T.  With
x = 0 a base record has ymx == ypx and kt = 0, and the lazy forms may store that zero as 0 or as q.

    every_curve_point(n, seed)   n points and scalars: subgroup points in arithmetic progression, with the special points
                                 planted where the kernels' lanes, rows and sums can go wrong (below)
    only_low_order(n, seed)      a call made of the four low-order points alone
    total_is_identity(n, seed)   every point with its negative under the same scalar

tests/test_ed_stages_gpu.py reads the stages of such calls, tests/test_ed_parity_gpu.py their results;
tests/test_stage_model_host.py pins the C oracle to pyref on them."""
import functools
import random

import pyref as R
import stage_model as M
from check_vectors import ed_low_order_points

# first and last lane of a wave (64) and of a 256-thread block, in the first blocks of a launch over the points
LANES = (0, 63, 64, 127, 255, 256, 511, 512)
SMALL_SCALARS = (0, 1, 2, 3, 4)


def fitting_scalar(rnd):
    """Uniform in [0, 2^253), drawn again while the even geometry would refuse it (2^253 - 2^238 and more: a rerun)."""
    while True:
        k = rnd.getrandbits(253)
        if M.recode(k, M.even16()).flags == 0:
            return k


def subgroup_points(n, a0, d):
    """P_i = [a0 + i d]G, one addition per point."""
    pt, step, out = R.ed_mul(R.ED_G, a0), R.ed_mul(R.ED_G, d), []
    for _ in range(n):
        out.append(pt)
        pt = R.ed_add(pt, step)
    return out


def progression_msm(a0, d, scalars, skip=()):
    """sum k_i [a0 + i d]G = [sum k_i (a0 + i d) mod ED_SUBGROUP]G over the indices not in `skip`: ONE pyref.ed_mul, because
    G has order ED_SUBGROUP.  pyref.ed_msm_naive takes 20 ms per point; tests/test_stage_model_host.py pins the two to each
    other (and util.oracle_ed_gen_points to this progression)."""
    total = sum(k * (a0 + i * d) for i, k in enumerate(scalars) if i not in skip) % R.ED_SUBGROUP
    return R.ed_mul(R.ED_G, total)


def special_classes(rnd):
    """One point of every class outside "a subgroup point other than the identity": the identity, order 2, order 4 (both),
    and P + T for each low-order T."""
    t2, t4a, t4b = ed_low_order_points()
    p = [R.ed_mul(R.ED_G, rnd.randrange(2, R.ED_SUBGROUP)) for _ in range(3)]
    classes = [t4a, t2, R.ED_ID, t4b, R.ed_add(p[0], t2), R.ed_add(p[1], t4a), R.ed_add(p[2], t4b)]
    for c in classes:
        assert R.ed_on_curve(c)
    return classes, p, (t2, t4a, t4b)


@functools.lru_cache(maxsize=None)
def every_curve_point(n, seed=0):
    """(points, scalars, planted, expected): subgroup points under scalars uniform in [0, 2^253), and planted on top of them, as far
    as n reaches (planted: index -> what was put there):
      - a special point at the first and last lane of a wave and of a 256-thread block and at index n - 1, each under a
        full-width scalar of its own: alone in its rows;
      - every special point next to its own negative under one scalar: rows whose sum is the identity;
      - every special point twice under one scalar: rows that double it (order 4 -> order 2 -> the identity);
      - P + T next to -P under one scalar, and P, T, -P: rows whose sum is the low-order point T;
      - every special point under each of the scalars 0, 1, 2, 3, 4: rows of slot 0 that hold all of them together.
    expected: pyref.ed_msm_naive over the planted points plus progression_msm over the others.  Cached: callers must not
    change the lists."""
    rnd = random.Random("ed every curve point/%d/%d" % (n, seed))
    a0, d = rnd.randrange(1, R.ED_SUBGROUP), rnd.randrange(1, R.ED_SUBGROUP)
    points = subgroup_points(n, a0, d)
    scalars = [fitting_scalar(rnd) for _ in range(n)]
    classes, p, low = special_classes(rnd)
    planted = {}

    def put(i, pt, k, what):
        if i < n and i not in planted:
            points[i], scalars[i], planted[i] = pt, k, what
            return True
        return False

    for j, lane in enumerate(LANES + (n - 1,)):
        put(lane, classes[j % len(classes)], fitting_scalar(rnd), "alone at lane %d" % lane)
    free = (i for i in range(1, n) if i not in LANES and i != n - 1)

    def group(members, what):
        k = fitting_scalar(rnd)
        for pt in members:
            i = next(free, None)
            if i is None:
                return
            put(i, pt, k, what)

    for c in classes:
        group([c, R.ed_neg(c)], "with its own negative")
    for c in classes:
        group([c, c], "twice under one scalar")
    for q, t in zip(p, low):
        group([R.ed_add(q, t), R.ed_neg(q)], "P + T with -P: the row sums to T")
    group([p[0], low[1], R.ed_neg(p[0])], "P, T, -P: the row sums to T")
    for k in SMALL_SCALARS:
        for c in classes:
            i = next(free, None)
            if i is not None:
                put(i, c, k, "scalar %d" % k)
    at = sorted(planted)
    expected = R.ed_add(R.ed_msm_naive([points[i] for i in at], [scalars[i] for i in at]), progression_msm(a0, d, scalars, skip=planted))
    return points, scalars, planted, expected


def only_low_order(n, seed=0):
    rnd = random.Random("ed only low order/%d/%d" % (n, seed))
    low = [R.ED_ID] + ed_low_order_points()
    points = [low[rnd.randrange(4)] for _ in range(n)]
    scalars = [fitting_scalar(rnd) for _ in range(n)]
    scalars[: len(SMALL_SCALARS)] = SMALL_SCALARS[:n]
    return points, scalars


def total_is_identity(n, seed=0):
    """n / 2 points of every_curve_point and, interleaved, their negatives under the same scalars."""
    pts, ks, _, _ = every_curve_point(n // 2, seed)
    points, scalars = [], []
    for pt, k in zip(pts, ks):
        points += [pt, R.ed_neg(pt)]
        scalars += [k, k]
    return points, scalars


# ---- scalars of the stage cases (tests/test_ed_stages_gpu.py); tests/test_stage_model_host.py checks on the CPU that they
# ---- meet the floors that make the decode cap of the stage tests a cap ----
def even_edge_scalars():
    """The even geometry at its edges: 15-bit digits of the top three windows at their boundaries, carries into and through
    them, the first scalars that do not fit (2^253 and more: the call reruns on sixteen equal windows), 0, 1, the order - 1."""
    s15 = 0x7FFF
    return [
        s15 << 208, s15 << 223, s15 << 238, (s15 << 208) + (0x8000 << 192), (s15 << 208) + (s15 << 223) + (0x8000 << 192),
        (s15 << 208) + (s15 << 223) + (s15 << 238) + (0x8000 << 192), (s15 << 238) + (s15 << 223) + (s15 << 208) + 0x7FFF,
        (1 << 253) - 1, 1 << 253, (1 << 254) + 5, (1 << 223) - 1, 1 << 223, (1 << 238) - 1, 1 << 238, 0, 1, R.ED_SUBGROUP - 1,
    ]


def uniform_scalars(n, seed):
    """Uniform in [0, 2^253) as far as the even geometry takes them: every one of its sixteen windows at full width.  (Drawn
    below ED_SUBGROUP only, window 15 would hold about 2^12 keys.)"""
    rnd = random.Random("ed uniform/%d/%d" % (n, seed))
    return [fitting_scalar(rnd) for _ in range(n)]


def few_distinct_scalars(n, distinct, seed):
    """n scalars over `distinct` values: rows of about n / distinct entries in every slot."""
    rnd = random.Random("ed few/%d/%d/%d" % (n, distinct, seed))
    values = [fitting_scalar(rnd) for _ in range(distinct)]
    return [values[rnd.randrange(distinct)] for _ in range(n)]


def one_long_row_scalars(n, length, seed):
    """`length` of the n scalars equal (one row of `length` entries in every slot), the others uniform."""
    rnd = random.Random("ed long row/%d/%d/%d" % (n, length, seed))
    same = fitting_scalar(rnd)
    ks = [same] * length + [fitting_scalar(rnd) for _ in range(n - length)]
    rnd.shuffle(ks)
    return ks
