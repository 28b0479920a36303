"""Inputs and expected values of the Edwards-BLS12 variable-base batch multiplication tests (TEST INFRASTRUCTURE), shared
by tests/test_ed_batch_mul_var_host.py, tests/test_ed_batch_mul_var_gpu.py and tests/test_ed_batch_mul_var_node_gpu.py.

The points are those of tests/ed_curve_points.py (every class of curve point, planted at the lanes where a wave or a block
begins and ends) and the reference's own vectors of tests/ed_vectors.py; every expected value comes from tests/pyref.py
(``R.ed_mul``: the affine law, complete on the curve).  Nothing here calls the engine's batch code."""
import functools
import random

import ed_curve_points as EP
import ed_vectors as V
import pyref as R

ORD = R.ED_SUBGROUP
MASK256 = 2**256 - 1
WINDOWS = 64  # signed 4-bit digits of the walk (csrc/batch_mul_var_recode.hpp)
PASS = 1 << 17  # BMV_PASS: the points of one pass
IDENTITY_WIRE = R.ed_encode_result(R.ED_ID)
LANES = EP.LANES


def nibbles(v):
    return sum(v << (4 * w) for w in range(WINDOWS))


def digit_scalars():
    """One scalar per possible digit value at window 0 and at window 63: the nibbles 0 .. 15 there (digits 0 .. 8 and,
    with a carry into the next window -- out of the top one -- -7 .. -1), everything else zero."""
    return [v << (4 * w) for w in (0, WINDOWS - 1) for v in range(16)]


def edge_scalars():
    """Small values around the table's end, the subgroup order and its neighbours (an output of O from a point that is
    not O), values whose recode ends in a final carry of 1, every nibble 8 / 9 / 0 but the top one, and digit_scalars."""
    out = [0, 1, 2, 7, 8, 9, 15, 16, ORD - 1, ORD, ORD + 1, 2**252, 2**253 - 1, 2**255, MASK256, nibbles(8), nibbles(9), 0xF << 252, 0x8 << 252, 0x1 << 252]
    return out + digit_scalars()


def final_carry(s):
    """The carry out of the top window of the signed 4-bit recode of s."""
    carry = 0
    for w in range(WINDOWS):
        f = ((s >> (4 * w)) & 15) + carry
        carry = 1 if f > 8 else 0
    return carry


def random_scalars(seed, n, bits=256):
    rnd = random.Random("ed batch mul var/%s/%d/%d" % (seed, n, bits))
    return [rnd.getrandbits(bits) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def case(n, seed=0):
    """(points, scalars) of n outputs: every_curve_point's points -- subgroup points with every special class planted at
    LANES, in cancelling pairs and under small scalars -- and its scalars, with the edge scalars laid over LANES first and
    then over the indices from 1 on that hold no planted point, as far as n reaches.  Cached: do not change the lists."""
    points, scalars, planted, _ = EP.every_curve_point(n, seed)
    points, scalars = list(points), list(scalars)
    edges = edge_scalars()
    at = [i for i in LANES if i < n] + [i for i in range(1, n) if i not in LANES and i not in planted]
    for i, s in zip(at, edges):
        scalars[i] = s
    return tuple(points), tuple(scalars)


@functools.lru_cache(maxsize=None)
def _mul(pt, s):
    return R.ed_mul(pt, s)


def expected(points, scalars):
    """Wire records by pyref, one R.ed_mul per output (about 20 ms each at full width)."""
    return b"".join(R.ed_encode_result(_mul(p, s)) for p, s in zip(points, scalars))


def encode(points, scalars):
    return R.ed_encode_points(list(points)), R.encode_scalars(list(scalars))


def reference_cases():
    """((x, y), k, (x', y')) of the reference's MULTIPLY vectors, and (x, k, x') of its x-only GROUP_SCALAR_MUL vectors."""
    return list(V.MULTIPLY), list(V.GROUP_SCALAR_MUL)


def off_curve_point():
    gx, gy = R.ED_G
    bad = (gx, gy ^ 1)
    assert not R.ed_on_curve(bad)
    return bad


def boundary_case(n, progression=None):
    """(point bytes, scalar bytes) around the pass boundary, n = PASS - 1, PASS or PASS + 1: subgroup points from a
    progression with special_classes laid around index PASS, scalars below 2^16 everywhere except at LANES, the last 2 points
    of pass 0 and the first 2 of pass 1 (full width: the one-thread twin stays at seconds).  progression(n, a0, d): the wire
    bytes of ed_curve_points.subgroup_points(n, a0, d) from a faster source (util.oracle_ed_gen_points, which
    tests/test_stage_model_host.py pins to it); default: subgroup_points itself."""
    rnd = random.Random("ed batch mul var boundary/%d" % n)
    a0, d = rnd.randrange(1, ORD), rnd.randrange(1, ORD)
    points = bytearray(progression(n, a0, d) if progression else R.ed_encode_points(EP.subgroup_points(n, a0, d)))
    classes, _, _ = EP.special_classes(rnd)
    for j, c in enumerate(classes):
        i = PASS - 4 + j  # PASS - 4 .. PASS + 2
        if i < n:
            points[64 * i : 64 * i + 64] = R.ed_encode_points([c])
    scalars = [rnd.getrandbits(16) for _ in range(n)]
    wide = [i for i in LANES + (PASS - 2, PASS - 1, PASS, PASS + 1) if i < n]
    for i, s in zip(wide, [MASK256, ORD + 1, nibbles(9), 2**255] + random_scalars("boundary", len(wide))):
        scalars[i] = s
    return bytes(points), R.encode_scalars(scalars)
