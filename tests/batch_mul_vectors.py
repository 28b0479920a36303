"""Inputs and expected values of the fixed-base batch multiplication tests (TEST INFRASTRUCTURE), shared by
tests/test_batch_mul_host.py, tests/test_batch_mul_gpu.py and tests/test_batch_mul_node_gpu.py.

Every expected value comes from tests/pyref.py (``R.mul``, which follows every exceptional case) or, in the GPU tests'
bulk cases, from the C oracle; nothing here calls the engine's batch_mul code."""
import functools

import check_vectors as CV
import pyref as R
import webgpu_msm_bls12_377_amd as msm

r = R.R_ORDER
WIDTHS = (8, 16)  # the device call's window widths (csrc/batch_mul_recode.hpp)
HOST_WIDTH = 4    # the host twin's
WIRE, MONT, MONT_FLAG = 0, 1, 2
IDENTITY_WIRE = R.encode_result(None)

EDGE = [0, 1, 2**256 - 1, 2**255, r, r - 1, r + 1]


def pattern_scalars(c):
    """Every c-bit field at 2^(c-1) (the largest positive digit), at 2^(c-1) - 1, and at 2^c - 1 (a carry that ripples
    through every window), cut to 256 bits."""
    out = []
    for field in (1 << (c - 1), (1 << (c - 1)) - 1, (1 << c) - 1):
        out.append(sum(field << (c * w) for w in range((256 + c - 1) // c)) & (2**256 - 1))
    return out


def window_scalars(c, windows=(0, 1, 7), digits=(1, 3)):
    """d 2^(c w) and r + d 2^(c w): sums that meet a table entry exactly (the equal- and opposite-point cases of an
    addition), for the digits d and d = 2^(c-1)."""
    out = []
    W = (256 + c - 1) // c
    for w in windows:
        w = min(w, W - 1)
        for d in list(digits) + [1 << (c - 1)]:
            v = d << (c * w)
            out += [v, (r + v) & (2**256 - 1)]
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
    """(name, point) pairs: the generator, the harness's fixed base, every small-order point, a torsion point of large
    order ([r] of a point lifted from x: it lies in the cofactor group) and a subgroup point plus that torsion point."""
    lifted = CV.g1_lifted_points(1)[0]
    torsion = R.mul(lifted, r)
    assert torsion is not None and R.on_curve(torsion) and R.mul(torsion, r) is not None  # outside the subgroup
    out = [("G", R.G), ("fixed_base", R.FIXED_BASE)]
    out += [("small_%d" % i, t) for i, t in enumerate(CV.g1_small_order_points())]
    out += [("torsion", torsion), ("G_plus_torsion", R.add(R.G, torsion))]
    return tuple(out)


def base_bytes(pt):
    return R.encode_points([pt])


def expected(base, scalars):
    """(wire records, flag bytes, list of points or None) by pyref."""
    pts = [R.mul(base, s) for s in scalars]
    return b"".join(R.encode_result(p) for p in pts), bytes(1 if p is None else 0 for p in pts), pts


def mont_flag_records(wire: bytes, flags: bytes) -> bytes:
    """What the MONT_FLAG form must hold: msm377_g1_result_to_native of each wire record, with the flag byte taken from
    `flags` (the converter sets it for the wire identity (0, 1), which is also a real point of order 3)."""
    out = bytearray()
    for i in range(len(flags)):
        rec = bytearray(msm.result_to_native(wire[96 * i : 96 * i + 96]))
        rec[96] = flags[i]
        out += rec
    return bytes(out)


def host_scalars():
    """The host test's scalar list: edges, 2r, 2r + 1, the window sums of every width, 40 random."""
    out = EDGE + [2 * r, 2 * r + 1]
    for c in (HOST_WIDTH,) + WIDTHS:
        out += window_scalars(c)
    return out + random_scalars(0xBA7C4, 40)


def gpu_base_scalars(n=130):
    """n scalars for the exceptional-base cases: the full-width edges and window sums in front, then scalars short enough
    that pyref checks all n of them for every base in a few seconds."""
    out = EDGE + [2 * r, 2 * r + 1]
    for c in WIDTHS:
        out += window_scalars(c, windows=(0, 1, 15))
    out += pattern_scalars(8)[:1] + pattern_scalars(16)[2:]
    out += list(range(2, 14))  # small multiples: the partial sums of a small-order base run through O again and again
    out += random_scalars(0x5A11, n, bits=40)
    return out[:n]
