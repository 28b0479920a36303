"""Inputs and expected values of the row-commitment tests (TEST INFRASTRUCTURE), shared by
tests/test_commit_rows_host.py, tests/test_commit_rows_gpu.py and tests/test_commit_rows_node_gpu.py.

Expected values come from tests/pyref.py (``R.mul`` and ``R.add``, which follow every exceptional case) or, for large k,
from generators with KNOWN LOGARITHMS: G_j = [g_j]G is made by the single-base host twin (msm.batch_mul_host, pinned to
pyref by tests/test_batch_mul_host.py) and out[i] = [sum_j s_ij g_j mod r]G by Python integers and the same twin --
valid for every 32-byte scalar because G has order r.  Nothing here calls the engine's commit_rows code."""
import functools

import batch_mul_multi_vectors as MV
import batch_mul_vectors as V
import pyref as R
import webgpu_msm_bls12_377_amd as msm

r = R.R_ORDER
GEN_MAX, GEN_WIDE_MAX = 4096, 64
SEGMENT = 16  # generators a thread walks at most (csrc/commit_rows_plan.hpp)
THREADS = 256
M = 0xCAFE
pack = MV.pack  # (bytes, out_stride, base_stride) of a list of rows in "rows" / "columns" / "padded"


def plan(k):
    """The three formulas of the issue, restated: (segments, generators per segment, rows per pass)."""
    if not 1 <= k <= GEN_MAX:
        return (0, 0, 0)
    s = -(-k // SEGMENT)
    return (s, -(-k // s), (2**20 // s) // THREADS * THREADS)


# ---- generators with known logarithms ----
@functools.lru_cache(maxsize=None)
def known_logs(k, seed=0x10C5):
    """(logarithms g_j in [1, r), the k generators [g_j]G as 96-byte wire records)."""
    logs = [v % (r - 1) + 1 for v in V.random_scalars(seed + k, k)]
    wire, flags = msm.batch_mul_host(V.base_bytes(R.G), R.encode_scalars(logs))
    assert not any(flags)
    return tuple(logs), wire


def multiples_of_g(values):
    """[v mod r]G for every v, as (wire records, flags), by the single-base host twin."""
    return msm.batch_mul_host(V.base_bytes(R.G), R.encode_scalars([v % r for v in values]))


def closed_rows(logs, rows):
    """Expected (records, flags) of dense rows over generators with the logarithms ``logs``."""
    return multiples_of_g([sum(s * g for s, g in zip(row, logs)) for row in rows])


# ---- sliding rows: out_stride = base_stride = 32 over ONE buffer, row i = buf[i : i + k] ----
def sliding_rows(buf, n, k):
    assert len(buf) >= n + k - 1
    return [tuple(buf[i : i + k]) for i in range(n)]


def sliding_bytes(buf):
    return R.encode_scalars(list(buf))


def sparse_sliding(n, k, seed, gap=None, bits=256):
    """A buffer of n + k scalars, zero but for one full-width value every ``gap`` positions.  With gap = k // 3 every row
    meets three non-zero scalars (four when one sits at both ends of its window) that fall into different segments, and
    the windows of all other tables are skipped wave-uniformly."""
    gap = gap or max(1, k // 3)
    buf = [0] * (n + k)
    vals = V.random_scalars(seed, (n + k) // gap + 1, bits)
    where = list(range(gap // 2, n + k, gap))
    for t, pos in enumerate(where):
        buf[pos] = vals[t] | 1
    return buf, where


def closed_sliding(logs, buf, where, rows_wanted, k):
    """Logarithm of out[i] for each i in rows_wanted: sum over the non-zero positions inside row i's window."""
    out = []
    for i in rows_wanted:
        out.append(sum(buf[p] * logs[p - i] for p in where if i <= p < i + k) % r)
    return out


# ---- the relations set: k = 48 = three segments of 16 ----
REL_K = 48
A, B, W33 = 0xA11CE5, 0xB0B0B0B, 0x77E33


@functools.lru_cache(maxsize=None)
def relation_generators():
    """48 generators (points) laid out so that the FOLD meets every case across a segment boundary (segments: 0..15,
    16..31, 32..47):  G_16 = -G_0, G_17 = G_1, G_18 = [M]G_2; a point of order 2, 3, 4 and 6 in segment 0 (3..6) and the
    same four in segment 1 (19..22); P + T outside the subgroup at 7 and 23; G_32 = G_0, G_33 = [W33]G; every other
    position a known multiple [100 + j]G."""
    b = dict(V.bases())
    small = [b["small_0"], b["small_3"], b["small_5"], b["small_6"]]  # orders 2, 3, 4, 6
    g = [R.mul(R.G, 100 + j) for j in range(REL_K)]
    g[0], g[1], g[2] = R.G, R.mul(R.G, A), R.mul(R.G, B)
    g[3:7] = small
    g[7] = b["G_plus_torsion"]
    g[16], g[17], g[18] = R.neg(R.G), g[1], R.mul(g[2], M)
    g[19:23] = small
    g[23] = b["G_plus_torsion"]
    g[32], g[33] = R.G, R.mul(R.G, W33)
    return tuple(g)


def _row(**at):
    row = [0] * REL_K
    for name, v in at.items():
        row[int(name[1:])] = v
    return tuple(row)


@functools.lru_cache(maxsize=None)
def relation_rows():
    """(name, row) pairs, sparse so that pyref prices a row at a handful of multiplications."""
    t, u, v = (x | 1 for x in V.random_scalars(0xF01D, 3, bits=250))
    s, = V.random_scalars(0xF01E, 1, bits=40)
    three = (-(t + u * A) * pow(W33, -1, r)) % r  # [t]G_0 + [u]G_17 + [three]G_33 = O, no two of them opposite
    rows = [
        ("zero", _row()),
        ("zero_multiples_of_r", _row(s0=r, s17=r, s34=r)),
        ("equal_partials", _row(s1=t, s17=t)),                     # [t]G_1 twice: the fold doubles
        ("opposite_partials", _row(s0=t, s16=t)),                  # [t]G - [t]G = O from two partials that are not O
        ("opposite_neighbour", _row(s0=t, s16=t + 1)),
        ("multiple_cancels", _row(s2=M * u % r, s18=r - u)),       # [M u]G_2 + [r - u][M]G_2 = O
        ("multiple_neighbour", _row(s2=M * u % r, s18=r - u + 1)),
        ("first_partial_zero", _row(s17=t, s40=u)),
        ("middle_partial_zero", _row(s1=t, s40=u)),
        ("last_partial_zero", _row(s1=t, s24=u)),
        ("only_last", _row(s47=v)),
        ("three_cancel", _row(s0=t, s17=u, s33=three)),            # O from three partials, none O, no pair opposite
        ("three_neighbour", _row(s0=t, s17=u, s33=(three + 1) % r)),
        ("two_then_opposite", _row(s0=t, s32=t, s16=2 * t)),        # p0 + p1 = -p2: the LAST addition meets its opposite
        ("order2_twice", _row(s3=1, s19=1)),                       # equal partials of order 2: the doubling gives O
        ("order2_inside_and_across", _row(s3=3, s19=2)),           # partial 1 is O by its own walk
        ("order3_cancel", _row(s4=1, s20=2)),
        ("order3_equal", _row(s4=1, s20=1)),                       # doubling a point of order 3: its negative
        ("order4_double", _row(s5=1, s21=1)),                      # doubling lands on the point of order 2
        ("order4_cancel", _row(s5=1, s21=3)),
        ("order6_mix", _row(s6=s, s22=5 * s + 1)),
        ("order6_cancel", _row(s6=1, s22=5)),
        ("small_orders_together", _row(s3=1, s4=2, s5=3, s6=5, s19=1, s20=1, s21=1, s22=2)),
        ("torsion_equal", _row(s7=s, s23=s)),
        ("torsion_opposite_mod_r_only", _row(s7=s, s23=r - s)),    # cancels in the subgroup part only: not O
        ("torsion_full_width", _row(s7=v, s23=t, s0=2**256 - 1)),
        ("full_width_edges", _row(s0=2**256 - 1, s16=2**255, s32=r + 1, s47=r - 1)),
    ]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def relation_expected():
    """(wire records, flags) of relation_rows over relation_generators by pyref, zero scalars skipped (R.mul(P, 0) is O)."""
    gens = relation_generators()
    pts = []
    for _, row in relation_rows():
        acc = None
        for gen, s in zip(gens, row):
            if s:
                acc = R.add(acc, R.mul(gen, s))
        pts.append(acc)
    flags = bytes(1 if p is None else 0 for p in pts)
    names = [name for name, _ in relation_rows()]
    must_be_o = ("zero", "zero_multiples_of_r", "opposite_partials", "multiple_cancels", "three_cancel", "two_then_opposite", "order2_twice", "order3_cancel", "order4_cancel", "order6_cancel")
    for name in names:
        assert flags[names.index(name)] == (1 if name in must_be_o else 0), name
    return b"".join(R.encode_result(p) for p in pts), flags


# ---- dense cases against pyref ----
@functools.lru_cache(maxsize=None)
def mixed_generators(k):
    """k generators for the pyref cases: subgroup points with a point of order 3, a point outside the subgroup, a torsion
    point and a repeat among them wherever k has room."""
    b = dict(V.bases())
    g = [R.mul(R.G, 0x51 + 7 * j) for j in range(k)]
    for pos, name in ((1, "G_plus_torsion"), (3, "small_3"), (16, "torsion"), (20, "small_6")):
        if pos < k:
            g[pos] = b[name]
    if k > 18:
        g[18] = g[0]
    return tuple(g)


def sliding_buffer(n, k, seed):
    """n + k - 1 scalars for dense sliding rows: the edges in front, one zero, then seeded full-width values."""
    vals = V.EDGE[2:] + [0] + V.random_scalars(seed, n + k)
    return vals[: n + k - 1]


def expected(points, rows):
    return MV.expected(points, rows)[:2]
