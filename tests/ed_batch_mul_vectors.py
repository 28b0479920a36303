"""Inputs and expected values of the Edwards-BLS12 batch multiplication tests (TEST INFRASTRUCTURE), shared by
tests/test_ed_batch_mul_host.py, tests/test_ed_batch_mul_gpu.py and tests/test_ed_batch_mul_node_gpu.py.

Every expected value comes from tests/pyref.py (``R.ed_mul`` and ``R.ed_add``: the affine law, complete on the curve);
the base classes are those of tests/ed_curve_points.py.  Nothing here calls the engine's batch code."""
import functools
import random

import ed_curve_points as EP
import pyref as R

ORD = R.ED_SUBGROUP
WIDTHS = (8, 16)  # the device call's window widths (csrc/batch_mul_recode.hpp)
MAX_BASES = 16
M = 0xCAFE  # the known multiple of the (G, [M]G) tuple
PAD = b"\xa5" * 32  # what padded rows hold between the scalars of two outputs: never read
IDENTITY_WIRE = R.ed_encode_result(R.ED_ID)
MASK256 = 2**256 - 1

# 0, 1, 2, the subgroup order and its neighbours, 4 x order (the curve's group order), the top bit, all ones
EDGE = [0, 1, 2, ORD - 1, ORD, ORD + 1, 4 * ORD, 2**255, MASK256]


def windows(c):
    return (256 + c - 1) // c


def digit_scalars(c):
    """For every window w of width c: the field 2^(c-1) (the largest digit, +2^(c-1)) and the field 2^(c-1) + 1 (the most
    negative digit, -(2^(c-1) - 1), with a carry into window w + 1; -2^(c-1) is not a digit of the recode), cut to 256
    bits: in the top window the carry goes into the table's last record."""
    half = 1 << (c - 1)
    out = []
    for w in range(windows(c)):
        out += [(half << (c * w)) & MASK256, ((half + 1) << (c * w)) & MASK256]
    return [s for s in out if s]


def pattern_scalars(c):
    """Every field at 2^(c-1), at 2^(c-1) + 1 and at 2^c - 1: the last one is a carry that ripples through all windows
    and out of the top one."""
    return [sum(f << (c * w) for w in range(windows(c))) & MASK256 for f in (1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1)]


def all_scalars():
    """The scalar set of the recode test: edges, every window's extreme digits and the rippling carries, both widths."""
    out = list(EDGE)
    for c in WIDTHS:
        out += digit_scalars(c) + pattern_scalars(c)
    return out


def random_scalars(seed, n, bits=256):
    g = R.splitmix64(seed)
    out = []
    for _ in range(n):
        v = 0
        for k in range(4):
            v |= next(g) << (64 * k)
        out.append(v & ((1 << bits) - 1))
    return out


@functools.lru_cache(maxsize=None)
def bases():
    """(name, point) pairs: the generator and one point of every class of ed_curve_points.special_classes -- an order-4
    point, the order-2 point, the identity, the other order-4 point, P + T for each low-order T."""
    classes, p, low = EP.special_classes(random.Random("ed batch mul bases"))
    names = ("order4_a", "order2", "identity", "order4_b", "P_plus_order2", "P_plus_order4_a", "P_plus_order4_b")
    return (("G", R.ED_G),) + tuple(zip(names, classes))


@functools.lru_cache(maxsize=None)
def tuples():
    """(name, bases) for k = 2 and 3: every relation between bases the call promises to follow."""
    b = dict(bases())
    g = R.ED_G
    return (
        ("G_G", (g, g)),
        ("G_negG", (g, R.ed_neg(g))),
        ("G_mG", (g, R.ed_mul(g, M))),
        ("order4_pair", (b["order4_a"], b["order4_b"])),
        ("order2_PplusT", (b["order2"], b["P_plus_order2"])),
        ("identity_G", (b["identity"], g)),
        ("PplusT4_T4", (b["P_plus_order4_a"], b["order4_a"])),
        ("G_mG_order4", (g, R.ed_mul(g, M), b["order4_b"])),
    )


def single_scalars():
    """The k = 1 scalars of the host test: small multiples (a low-order base runs through the identity), the order's
    neighbours, the curve's group order, full width."""
    return [0, 1, 2, 3, 4, ORD - 1, ORD + 1, 4 * ORD, 2**255 + 12345, MASK256]


def relation_rows(k):
    """Rows for the relation tuples: sums that cancel with no term the identity (s_0 = s_1 over (G, -G); (M t, ORD - t)
    over (G, [M]G); (1, 1) over the two points of order 4), each beside a neighbour that differs in one scalar, the zero
    row, and full-width rows."""
    t = random_scalars(0xEDCA9C, 1, bits=200)[0]
    rows = [(t, t), (t, t + 1), (M * t % ORD, ORD - t), (M * t % ORD, ORD - t + 1), (1, 1), (1, 2), (0, 0), (MASK256, 2**255 + 7)]
    return [row + (3,) * (k - 2) for row in rows]


def bases_bytes(points):
    return R.ed_encode_points(list(points))


def pack(rows, layout="rows"):
    """(scalar bytes, out_stride, base_stride) of the k x n matrix in one of the three layouts."""
    n, k = len(rows), len(rows[0]) if rows else 1
    if layout == "rows":
        return b"".join(R.encode_scalars(list(row)) for row in rows), 32 * k, 32
    if layout == "padded":
        return b"".join(R.encode_scalars(list(row)) + PAD for row in rows), 32 * (k + 1), 32
    assert layout == "columns"
    return b"".join(R.encode_scalars([row[j] for row in rows]) for j in range(k)), 32, 32 * max(n, 1)


@functools.lru_cache(maxsize=None)
def _mul(pt, s):
    return R.ed_mul(pt, s)


def expected(points, rows):
    """(wire records, list of points) by pyref: each term by R.ed_mul, the sum by R.ed_add."""
    pts = []
    for row in rows:
        acc = R.ED_ID
        for b, s in zip(points, row):
            acc = R.ed_add(acc, _mul(b, s))
        pts.append(acc)
    return b"".join(R.ed_encode_result(p) for p in pts), pts


def many_rows(k, count, seed, bits=256):
    """count rows of k scalars: the edge list down the diagonal, then seeded values."""
    flat = random_scalars(seed, k * count, bits)
    rows = [tuple(flat[k * i : k * i + k]) for i in range(count)]
    for i, e in enumerate(EDGE[:count]):
        row = list(rows[i])
        row[i % k] = e
        rows[i] = tuple(row)
    return rows
