"""Inputs and expected values of the variable-base batch multiplication tests (TEST INFRASTRUCTURE), shared by
tests/test_batch_mul_var_host.py, tests/test_batch_mul_var_gpu.py and tests/test_batch_mul_var_node_gpu.py: what
tests/batch_mul_vectors.py (imported, not copied) does not already hold -- native point forms built by integer
arithmetic, arrays that mix exceptional points with subgroup points, per-point expected values.

Every expected value comes from tests/pyref.py (``R.mul``); nothing here calls the engine's batch_mul_var code."""
import functools

import batch_mul_vectors as V
import pyref as R

r = R.R_ORDER
MONT_R = 1 << 384  # the callers' Montgomery radix of Fp
GARBAGE = bytes((0xC3 ^ (7 * k)) & 0xFF for k in range(96))  # coordinate bytes of a flagged record: p or more, never read


def random_subgroup_points(seed, n):
    """n points [k]G: a chain of additions from a seeded start (one pyref multiplication, then n additions)."""
    g = R.splitmix64(seed)
    start = R.mul(R.G, (next(g) << 64 | next(g)) % r or 1)
    step = R.mul(R.G, next(g) | 1)
    out = [start]
    for _ in range(n - 1):
        out.append(R.add(out[-1], step))
    return out


@functools.lru_cache(maxsize=None)
def mixed_points(n, seed=0x3A12ED, period=7):
    """n points: the points of V.bases() in turn at every `period`-th index among random subgroup points."""
    special = [pt for _, pt in V.bases()]
    out = random_subgroup_points(seed, n)
    for k, i in enumerate(range(0, n, period)):
        out[i] = special[k % len(special)]
    return tuple(out)


def mont_records(points, flag=False, flagged=()):
    """Wire points as MSM377_POINTS_MONT (96-byte) or MSM377_POINTS_MONT_FLAG (104-byte) records, by integer arithmetic.
    The indices in `flagged` become identity records whose coordinate bytes are garbage."""
    flagged = set(flagged)
    out = bytearray()
    for i, (x, y) in enumerate(points):
        if i in flagged:
            assert flag
            out += GARBAGE + b"\x01" + bytes(7)
            continue
        out += (x * MONT_R % R.P).to_bytes(48, "little") + (y * MONT_R % R.P).to_bytes(48, "little")
        if flag:
            out += bytes(8)
    return bytes(out)


def expected(points, scalars, flagged=()):
    """(wire records, flag bytes) of [s_i]P_i by pyref; a flagged index is the identity.  One scalar: for all points."""
    flagged = set(flagged)
    if len(scalars) == 1:
        scalars = list(scalars) * len(points)
    pts = [None if i in flagged else R.mul(p, s) for i, (p, s) in enumerate(zip(points, scalars))]
    return b"".join(R.encode_result(p) for p in pts), bytes(1 if p is None else 0 for p in pts)


def mont_scalars(values):
    """What 32-byte Montgomery values mean: v 2^-256 mod r, fully reduced."""
    inv = pow(1 << 256, -1, r)
    return [v * inv % r for v in values]


MONT_SCALAR_VALUES = [0, 1, r - 1, r, r + 1, 2**256 - 1, 2**255]
