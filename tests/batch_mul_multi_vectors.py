"""Inputs and expected values of the multi-base batch multiplication tests (TEST INFRASTRUCTURE), shared by
tests/test_batch_mul_multi_host.py, tests/test_batch_mul_multi_gpu.py and tests/test_batch_mul_multi_node_gpu.py.

Every expected value comes from tests/pyref.py (``R.mul`` and ``R.add``, which follow every exceptional case); scalars,
bases and the record forms are those of tests/batch_mul_vectors.py.  Nothing here calls the engine's batch_mul code."""
import functools

import batch_mul_vectors as V
import pyref as R

r = R.R_ORDER
MAX_BASES = 16
M = 0xCAFE  # the known multiple of the (G, [M]G) tuple
PAD = b"\xa5" * 32  # what padded rows hold between the scalars of two outputs: never read


@functools.lru_cache(maxsize=None)
def tuples():
    """(name, (B_0, B_1)) pairs: every relation between two bases the call promises to follow -- equal, opposite, a known
    multiple, two equal points of order 3, a point of order 2 beside a point outside the subgroup, a torsion point of
    large order beside the generator."""
    b = dict(V.bases())
    return (
        ("G_G", (R.G, R.G)),
        ("G_negG", (R.G, R.neg(R.G))),
        ("G_mG", (R.G, R.mul(R.G, M))),
        ("small3_small3", (b["small_3"], b["small_3"])),
        ("order2_GplusT", (b["small_0"], b["G_plus_torsion"])),
        ("torsion_G", (b["torsion"], R.G)),
    )


def bases_bytes(points):
    return R.encode_points(list(points))


def cancelling_rows():
    """Rows whose sum is O over one of the tuples with NEITHER term O, each beside an ordinary neighbour that differs in
    one scalar: (G, [M]G): s_0 = M t, s_1 = r - t; (G, -G): s_0 = s_1; (G, G): s_1 = r - s_0; two equal points of
    order 3: s_0 + s_1 = 0 mod 3."""
    t1, t2 = V.random_scalars(0xCA9CE1, 2, bits=200)
    out = []
    for t in (1, t1, t2):
        out += [(M * t, r - t), (M * t, r - t + 1)]
        out += [(t, t), (t, t + 1)]
        out += [(t % r, r - t % r), (t % r + 1, r - t % r)]
    out += [(1, 2), (2, 4), (2, 2), (5, 1), (r + 1, 2 * r + 2)]
    return out


ZERO_ROWS = [(0, 0), (0, r), (2, 0)]  # an identity output over every tuple: both terms O, or [2] of a point of order 2


def host_rows():
    """The host test's rows for k = 2: the zero rows, the edge list against itself shifted by one, 2r, the window sums of widths 4, 8
    and 16 in both columns, the cancelling pairs, 8 random full-width rows."""
    col = V.EDGE + [2 * r, 2 * r + 1]
    for c in (V.HOST_WIDTH,) + V.WIDTHS:
        col += V.window_scalars(c)
    rows = ZERO_ROWS + list(zip(col, col[1:] + col[:1]))
    rows += cancelling_rows()
    rnd = V.random_scalars(0xBA7C5, 16)
    return rows + list(zip(rnd[:8], rnd[8:]))


def gpu_rows(n=130):
    """n rows for the relation cases on the GPU: the cancelling pairs and the zero rows in front, full-width edges and window sums, then
    scalars short enough that pyref checks all n rows of every tuple in a few seconds (V.gpu_base_scalars)."""
    col = V.gpu_base_scalars(n)
    front = cancelling_rows()
    rows = front + ZERO_ROWS + list(zip(col, col[3:] + col[:3]))
    return rows[:n]


def many_rows(k, count, seed, bits=256):
    """count rows of k scalars: the edge list down the diagonal, then seeded values."""
    flat = V.random_scalars(seed, k * count, bits)
    rows = [tuple(flat[k * i : k * i + k]) for i in range(count)]
    for i, e in enumerate(V.EDGE[:count]):
        row = list(rows[i])
        row[i % k] = e
        rows[i] = tuple(row)
    return rows


def pack(rows, layout="rows"):
    """(scalar bytes, out_stride, base_stride) of the k x n matrix in one of the three layouts."""
    n, k = len(rows), len(rows[0]) if rows else 1
    if layout == "rows":
        return b"".join(R.encode_scalars(list(row)) for row in rows), 32 * k, 32
    if layout == "padded":
        return b"".join(R.encode_scalars(list(row)) + PAD for row in rows), 32 * (k + 1), 32
    assert layout == "columns"
    return b"".join(R.encode_scalars([row[j] for row in rows]) for j in range(k)), 32, 32 * max(n, 1)


def expected(points, rows):
    """(wire records, flag bytes, list of points or None) by pyref: each term by R.mul, the sum by R.add."""
    pts = []
    for row in rows:
        acc = None
        for b, s in zip(points, row):
            acc = R.add(acc, R.mul(b, s))
        pts.append(acc)
    return b"".join(R.encode_result(p) for p in pts), bytes(1 if p is None else 0 for p in pts), pts
