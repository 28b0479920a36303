"""Inputs and expected values of the Edwards-BLS12 row-commitment tests (TEST INFRASTRUCTURE), shared by
tests/test_ed_commit_rows_host.py, tests/test_ed_commit_rows_gpu.py, tests/test_ed_commit_rows_stash_gpu.py and
tests/test_ed_commit_rows_node_gpu.py.

Expected values come from tests/pyref.py (``R.ed_mul`` and ``R.ed_add``: the complete law, no cases) or, for large k, from
generators with KNOWN LOGARITHMS: G_j = [g_j]G is made by the k = 1 host twin (msm.ed_batch_mul_multi_host, pinned to pyref
by tests/test_ed_batch_mul_host.py) and out[i] = [sum_j s_ij g_j mod l]G by Python integers and the same twin -- valid for
every 32-byte scalar because G has order l = ED_SUBGROUP.  Nothing here calls the engine's ed_commit_rows code.  The
shapes -- the plan, the sliding rows, the sparse sliding buffer -- are tests/commit_rows_vectors.py's."""
import functools

import commit_rows_vectors as CR
import ed_batch_mul_vectors as EV
import ed_curve_points as EP
import pyref as R
import webgpu_msm_bls12_377_amd as msm

ORD = R.ED_SUBGROUP
MASK256 = EV.MASK256
GEN_MAX, GEN_WIDE_MAX = CR.GEN_MAX, CR.GEN_WIDE_MAX
SEGMENT, THREADS = CR.SEGMENT, CR.THREADS
FOLD_GROUP = 16  # partial sums one fold thread adds (csrc/kernels/ed_commit_rows.hpp CR_FOLD_GROUP)
IDENTITY_WIRE = EV.IDENTITY_WIRE
M = 0xCAFE
plan = CR.plan
pack = EV.pack  # (bytes, out_stride, base_stride) of a list of rows in "rows" / "columns" / "padded"
sliding_rows, sliding_bytes, sparse_sliding = CR.sliding_rows, CR.sliding_bytes, CR.sparse_sliding
G_WIRE = R.ed_encode_points([R.ED_G])


def segment_of(j, k):
    """The segment whose thread walks generator j of a call over k generators."""
    return j // plan(k)[1]


# ---- generators with known logarithms ----
def multiples_of_g(values):
    """[v mod l]G for every v, as wire records, by the k = 1 host twin."""
    return msm.ed_batch_mul_multi_host(G_WIRE, R.encode_scalars([v % ORD for v in values]))


@functools.lru_cache(maxsize=None)
def known_logs(k, seed=0xED10C5):
    """(logarithms g_j in [1, l), the k generators [g_j]G as 64-byte wire records)."""
    logs = tuple(v % (ORD - 1) + 1 for v in EV.random_scalars(seed + k, k))
    return logs, multiples_of_g(logs)


def closed_rows(logs, rows):
    """Expected records of dense rows over generators with the logarithms ``logs``."""
    return multiples_of_g([sum(s * g for s, g in zip(row, logs)) for row in rows])


def closed_sliding(logs, buf, where, rows_wanted, k):
    """Logarithm of out[i] for each i in rows_wanted: the sum over the non-zero positions inside row i's window."""
    return [sum(buf[p] * logs[p - i] for p in where if i <= p < i + k) % ORD for i in rows_wanted]


# ---- buffers for sliding rows: row i = buf[i : i + k] ----
def mixed_buffer(count, seed, every=8):
    """count scalars a reference prices cheaply: the edge values in front, then one full-width value in ``every``, one zero
    in eight and 20-bit values between them (double-and-add and pyref both cost by the bit)."""
    full = EV.random_scalars(seed, count)
    short = EV.random_scalars(seed ^ 0x5A5A, count, bits=20)
    vals = list(EV.EDGE)
    for t in range(count):
        vals.append(full[t] if t % every == 0 else 0 if t % 8 == 3 else short[t] | 1)
    return vals[:count]


# ---- dense cases against pyref ----
@functools.lru_cache(maxsize=None)
def mixed_generators(k):
    """k generators for the pyref cases: subgroup points [0x51 + 7 j]G with the point of order 2, a point of order 4, the
    identity, a point outside the subgroup and a repeat among them wherever k has room."""
    b = dict(EV.bases())
    g = EP.subgroup_points(k, 0x51, 7)
    for pos, name in ((1, "P_plus_order4_a"), (3, "order2"), (5, "identity"), (16, "order4_b"), (20, "P_plus_order2")):
        if pos < k:
            g[pos] = b[name]
    if k > 18:
        g[18] = g[0]
    return tuple(g)


def expected(points, rows):
    """Wire records by pyref, zero scalars skipped ([0]P is the identity, which adds nothing)."""
    out = []
    for row in rows:
        acc = R.ED_ID
        for pt, s in zip(points, row):
            if s:
                acc = R.ed_add(acc, EV._mul(pt, s))
        out.append(acc)
    return b"".join(R.ed_encode_result(p) for p in out)


# ---- the relations set: k = 273 = 18 segments: one full fold group (segments 0..15, generators 0..255) and a group of
# ---- two (segments 16 and 17, generators 256..271 and 272)
REL_K = 273
A, B, W272 = 0xA11CE5, 0xB0B0B0B, 0x77E33


@functools.lru_cache(maxsize=None)
def relation_generators():
    """273 generators, [100 + j]G but for:
      0, 1, 2          G, [A]G, [B]G
      3 .. 8           the identity, the point of order 2, both points of order 4, P + T4, P + T2   (segment 0)
      9, 10            -G_1, G_1                                   pairs WITHIN segment 0
      20, 21, 22       -G_0, G_1, [M]G_2                           pairs across segments 0 and 1 of group 0
      35 .. 38         the identity, order 2, both of order 4      again, in segment 2
      256 .. 259       -G_0, G_1, [M]G_2, the first point of order 4     pairs across the two GROUPS (segment 16)
      272              [W272]G                                     alone in segment 17, the last"""
    b = dict(EV.bases())
    low = [b["identity"], b["order2"], b["order4_a"], b["order4_b"]]
    g = EP.subgroup_points(REL_K, 100, 1)
    g[0], g[1], g[2] = R.ED_G, R.ed_mul(R.ED_G, A), R.ed_mul(R.ED_G, B)
    g[3:7] = low
    g[7], g[8] = b["P_plus_order4_a"], b["P_plus_order2"]
    g[9], g[10] = R.ed_neg(g[1]), g[1]
    g[20], g[21], g[22] = R.ed_neg(R.ED_G), g[1], R.ed_mul(g[2], M)
    g[35:39] = low
    g[256], g[257], g[258], g[259] = R.ed_neg(R.ED_G), g[1], R.ed_mul(g[2], M), b["order4_a"]
    g[272] = R.ed_mul(R.ED_G, W272)
    assert len(g) == REL_K and plan(REL_K)[:2] == (18, 16)
    return tuple(g)


def _row(**at):
    row = [0] * REL_K
    for name, v in at.items():
        row[int(name[1:])] = v
    return tuple(row)


@functools.lru_cache(maxsize=None)
def relation_rows():
    """(name, row) pairs, sparse so that pyref prices a row at a handful of multiplications."""
    t, u, v = (x | 1 for x in EV.random_scalars(0xEDF01D, 3, bits=250))
    s, = EV.random_scalars(0xEDF01E, 1, bits=40)
    # [t]G_0 + [u]G_17 in group 0, [t]G_256 + [x]G_272 in group 1: the group sums are [t + 117 u]G and its negative
    x = (-(117 * u) * pow(W272, -1, ORD)) % ORD
    rows = [
        ("zero", _row()),
        ("zero_multiples_of_l", _row(s0=ORD, s20=ORD, s272=ORD)),
        ("opposite_within_segment", _row(s1=t, s9=t)),                    # the walk itself meets its opposite
        ("equal_within_segment", _row(s1=t, s10=t)),
        ("opposite_partials_in_group", _row(s0=t, s20=t)),                # O from two partials of ONE group that are not O
        ("opposite_neighbour_in_group", _row(s0=t, s20=t + 1)),
        ("multiple_cancels_in_group", _row(s2=M * u % ORD, s22=ORD - u)),
        ("equal_partials_in_group", _row(s1=t, s21=t)),                   # the fold adds a point to itself
        ("opposite_group_sums", _row(s0=t, s256=t)),                      # O from two GROUP sums that are not O
        ("opposite_group_sums_of_two_partials", _row(s0=t, s17=u, s256=t, s272=x)),
        ("group_sums_neighbour", _row(s0=t, s17=u, s256=t, s272=(x + 1) % ORD)),
        ("multiple_cancels_across_groups", _row(s2=M * u % ORD, s258=ORD - u)),
        ("equal_group_sums", _row(s1=t, s257=t)),
        ("only_last", _row(s272=v)),                                      # a single non-zero scalar in the last generator
        ("first_group_zero", _row(s260=t, s272=u)),
        ("second_group_zero", _row(s1=t, s40=u)),
        ("identity_generators", _row(s3=v, s35=t, s0=s)),
        ("order2_twice", _row(s4=1, s36=1)),
        ("order2_odd_and_even", _row(s4=3, s36=2, s0=s)),
        ("order4_double", _row(s5=1, s259=1)),                            # lands on the point of order 2, across the groups
        ("order4_cancel", _row(s5=1, s259=3)),
        ("order4_pair", _row(s5=1, s6=1)),                                # T + (-T) inside segment 0
        ("order4_other_segment", _row(s6=2, s37=1, s38=1)),
        ("torsion_mix", _row(s7=s, s8=5 * s + 1)),
        ("torsion_cancels_mod_l_only", _row(s7=s, s8=ORD - s, s0=1)),
        ("torsion_full_width", _row(s7=v, s8=t, s0=MASK256)),
        ("full_width_edges", _row(s0=MASK256, s20=2**255, s256=ORD + 1, s272=ORD - 1)),
    ]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def relation_expected():
    """Wire records of relation_rows over relation_generators by pyref."""
    wire = expected(relation_generators(), [row for _, row in relation_rows()])
    names = [name for name, _ in relation_rows()]
    must_be_o = ("zero", "zero_multiples_of_l", "opposite_within_segment", "opposite_partials_in_group", "multiple_cancels_in_group", "opposite_group_sums",
                 "opposite_group_sums_of_two_partials", "multiple_cancels_across_groups", "order2_twice", "order4_cancel", "order4_pair")
    for i, name in enumerate(names):
        assert (wire[64 * i : 64 * i + 64] == IDENTITY_WIRE) == (name in must_be_o), name
    return wire


def off_curve_point():
    gx, gy = R.ED_G
    bad = (gx, gy ^ 1)
    assert not R.ed_on_curve(bad)
    return bad
