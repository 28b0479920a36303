"""Inputs and expected values of the pairwise linear combination tests (TEST INFRASTRUCTURE), shared by
tests/test_batch_lincomb2_host.py, tests/test_batch_lincomb2_gpu.py and tests/test_batch_lincomb2_node_gpu.py: what
tests/batch_mul_vectors.py and tests/batch_mul_var_vectors.py (imported, not copied) do not already hold -- pairs of
arrays with relations between them, expected values of two terms.

Every expected value comes from tests/pyref.py: ``R.add(R.mul(P, a), R.mul(Q, b))``, whose ``add`` handles P + P, P + (-P)
and O; nothing here calls the engine's batch_lincomb2 code."""
import functools

import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import check_vectors as CV
import pyref as R

r = R.R_ORDER
FULL = 2**256 - 1
BLOCK = 1024  # outputs per workgroup product tree of the normalisation (4 per thread, 256 threads)


def expected_points(p, q, a, b, flagged_p=(), flagged_q=()):
    """[a_i]P_i + [b_i]Q_i by pyref as points (None: the identity); a flagged index makes its term the identity.  One
    scalar in a or b: for all pairs."""
    n = len(p)
    a = list(a) * n if len(a) == 1 else a
    b = list(b) * n if len(b) == 1 else b
    fp, fq = set(flagged_p), set(flagged_q)
    assert len(q) == n and len(a) == n and len(b) == n
    return [R.add(None if i in fp else R.mul(p[i], a[i]), None if i in fq else R.mul(q[i], b[i])) for i in range(n)]


def records(points):
    """(wire records, flag bytes) of a list of points."""
    return b"".join(R.encode_result(pt) for pt in points), bytes(1 if pt is None else 0 for pt in points)


def expected(p, q, a, b, flagged_p=(), flagged_q=()):
    return records(expected_points(p, q, a, b, flagged_p, flagged_q))


def out_records(wire, flags, out_form):
    """What the call must return in out_form (V.WIRE / V.MONT_FLAG, or their names)."""
    return wire if out_form in (V.WIRE, "wire") else V.mont_flag_records(wire, flags)


def host_scalars():
    """The host test's scalars: the full-width edges, 2r, 2r + 1, scalars that carry out of the top, then short ones (a
    full-width pyref multiplication costs about 1.5 ms; two terms per output)."""
    return V.EDGE + [2 * r, 2 * r + 1, FULL - 1, 0x9 << 252] + list(range(2, 8)) + V.random_scalars(0xBA7C5, 24, bits=40) + V.random_scalars(0xBA7C6, 6)


@functools.lru_cache(maxsize=None)
def relations(n=3 * BLOCK + 7):
    """n pairs and their scalars for the GPU test of relations and exceptional points, mixed within waves; everything the
    lanes of a wave can do differently sits in neighbouring lanes.  Returns (p, q, a, b, flagged_p, flagged_q) with
    points as tuples; the flagged indices matter to the mont_flag point form only (expected_points takes them)."""
    p = list(VV.random_subgroup_points(0x11C0B2, n))
    q = list(VV.random_subgroup_points(0x22C0B2, n))
    short_a = V.random_scalars(0xA5A1, n, bits=40)
    short_b = V.random_scalars(0xB5B1, n, bits=40)
    a, b = list(short_a), list(short_b)
    special = [pt for _, pt in V.bases()]
    small = CV.g1_small_order_points()
    edge = V.EDGE + [2 * r, 2 * r + 1]
    k_mul = 0x1D3F
    flagged_p, flagged_q = [], []
    for i in range(n):
        kind = i % 16
        if BLOCK <= i < BLOCK + 64:  # a whole wave of a small-order point in P ...
            p[i] = small[(i // 16) % len(small)]
            a[i] = (i - BLOCK) % 9
        elif BLOCK + 64 <= i < BLOCK + 128:  # ... and in Q
            q[i] = small[(i // 16) % len(small)]
            b[i] = (i - BLOCK) % 7
        elif kind == 0:  # Q = P: equal digits hit madd's doubling exit
            q[i] = p[i]
            b[i] = a[i] if i % 32 else short_b[i]
        elif kind == 1:  # Q = -P: with a = b the identity mid-walk and at the end; with a != b at single steps
            q[i] = R.neg(p[i])
            b[i] = a[i] if i % 32 == 1 else a[i] ^ 0x30
        elif kind == 2:  # Q = [k]P and a = -k b (mod r): O with P != +-Q
            q[i] = R.mul(p[i], k_mul)
            a[i] = (-k_mul * b[i]) % r
        elif kind == 3:
            (flagged_q, flagged_p, flagged_p)[(i // 16) % 3].append(i)
            if (i // 16) % 3 == 2:
                flagged_q.append(i)  # both flagged
        elif kind == 4:  # small orders, torsion, G + T in P, in Q, in both
            which = (i // 16) % 3
            if which != 1:
                p[i] = special[(i // 48) % len(special)]
            if which != 0:
                q[i] = special[(i // 48 + 3) % len(special)]
            a[i], b[i] = 2 + (i // 16) % 11, 1 + (i // 16) % 13
        elif kind == 5:
            a[i], b[i] = ((0, short_b[i]), (short_a[i], 0), (0, 0))[(i // 16) % 3]
        elif kind == 6 and i % 64 == 6:  # both carries; a carry in one scalar only
            a[i], b[i] = ((FULL, FULL), (FULL, short_b[i]), (short_a[i], 0x9 << 252))[(i // 64) % 3]
        elif kind == 7 and i % 128 == 7:  # full-width edges against each other
            a[i], b[i] = edge[(i // 128) % len(edge)], edge[(i // 128 + 4) % len(edge)]
    three = 2 * BLOCK + 77  # (0, 1): a real point of order 3 and the wire encoding of the identity
    p[three], a[three], b[three] = (0, 1), 1, 0
    return tuple(p), tuple(q), tuple(a), tuple(b), tuple(flagged_p), tuple(flagged_q)


@functools.lru_cache(maxsize=None)
def relations_expected(with_flags=False):
    p, q, a, b, fp, fq = relations()
    return expected(p, q, a, b, fp if with_flags else (), fq if with_flags else ())


@functools.lru_cache(maxsize=None)
def relations_sum():
    """P_i + Q_i over the same fixture: what a = b = 1 must give."""
    p, q, _, _, _, _ = relations()
    return records([R.add(x, y) for x, y in zip(p, q)])
