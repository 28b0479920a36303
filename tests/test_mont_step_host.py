"""The reduction step of the lazy Montgomery products (csrc/field29.hpp mul_lz, mul_add_mul_lz, sqr_lz: biased columns,
q = ~t0' & LMASK, carry = t0' >> 29) against the form it replaced, which tests/native/mont_step_host.cpp keeps verbatim:
the same limbs, every one, on 10^5 random operands per allowed shape and on the corners of the shapes.  CPU only.

The shapes are tools/check_lazy_bounds.py's table (the proof that no column overflows -- with the bias -- runs over
the same boxes).  The q = 0 case, where t0 is a multiple of 2^29 and ceil(t0 / 2^29) = t0 / 2^29, is forced by operands
whose column 0 is 0 or a multiple of 2^29; an operand 0 makes EVERY digit of the product 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import util

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "mont_step_host.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
SO = os.path.join(BUILD, "libmont_step_host.so")
EXE = os.path.join(BUILD, "mont_step_sanitized")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_lazy_bounds as B  # noqa: E402

LB, MASK = 29, (1 << 29) - 1
RANDOM_CASES = 100000


def _stale(target):
    deps = [SRC, os.path.join(CSRC, "field29.hpp"), os.path.join(CSRC, "consts_gen.hpp")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def load_lib():
    if _stale(SO):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", CSRC, "-o", SO, SRC])
    so = ctypes.CDLL(SO)
    so.mont_step_compare.restype = ctypes.c_uint32
    return so


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def limbs_of(v, n):
    """Carry-normalised limbs of an integer (the top limb takes the rest)."""
    return [(v >> (LB * j)) & MASK for j in range(n - 1)] + [v >> (LB * (n - 1))]


def value_of(limbs):
    return sum(int(x) << (LB * j) for j, x in enumerate(limbs))


class FieldCase:
    def __init__(self, name):
        B.use_field(name)
        self.name, self.id, self.N, self.RS, self.P, self.E = name, 0 if name == "Fp" else 1, B.N, B.RS, B.P, B.E
        self.box = {k: list(v.limbs) for k, v in B.shapes().items()}
        self.box["canonical"][-1] -= 1  # strictly below p whatever the lower limbs are
        # operand shapes of each product, as field29.hpp's comment and the proof's replay allow them
        self.mul_pairs = [("canonical", "canonical"), ("stored", "stored"), ("wide", "wide"), ("lazy", "narrow"), ("narrow", "lazy")]
        self.sqr_shapes = ["canonical", "stored", "wide"]
        if name == "Fp":  # Y3 = R D + (2p - Y1) PPP of the Weierstrass formulas
            self.mam_quads = [("canonical",) * 4, ("diff3", "diff7", "kp2_sub", "stored")]
        else:
            self.mam_quads = [("canonical",) * 4]

    def random(self, shape, n, seed):
        rng = np.random.default_rng(seed)
        return np.stack([rng.integers(0, b + 1, size=n, dtype=np.uint64) for b in self.box[shape]], axis=1).astype(np.uint32)

    def extremes(self, shape):
        """The corners of the shape and the values the issue names, as far as they lie inside the shape."""
        box = self.box[shape]
        out = [list(box), [0] * self.N, [box[0]] + [0] * (self.N - 1), [0] * (self.N - 1) + [box[-1]], list(box[:-1]) + [0]]
        for v in (1, 2, self.P - 1, self.P, self.P + self.E - 1, 1 << 28, 1 << LB, (1 << LB) - 1):
            l = limbs_of(v, self.N)
            if all(x <= b for x, b in zip(l, box)):
                out.append(l)
        # column 0 = a.l[0] * b.l[0] a multiple of 2^29 (q = 0 in the first step), the other limbs at the corner
        for l0 in (0, 2, 1 << 14, 1 << 15, 1 << 28):
            if l0 <= box[0]:
                out.append([l0] + list(box[1:]))
        return out


def run(lib, fc, op, operands, want_out=False):
    n = len(operands[0])
    arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in operands]
    while len(arrs) < 4:
        arrs.append(arrs[0])
    out = np.zeros((n, fc.N), dtype=np.uint32) if want_out else None
    first = ctypes.c_uint32(0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = lib.mont_step_compare(fc.id, op, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), ctypes.c_uint32(n),
                                ptr(out) if want_out else None, ctypes.byref(first))
    assert bad == 0, "%s op %d: %d of %d cases differ from the reference form, first %d: %s" % (
        fc.name, op, bad, n, first.value, [list(map(int, a[first.value])) for a in arrs])
    return out


def cross(lists):
    """Every combination of the extreme operands, as one array per operand."""
    grids = np.meshgrid(*[np.arange(len(l)) for l in lists], indexing="ij")
    return [np.array(l, dtype=np.uint32)[g.ravel()] for l, g in zip(lists, grids)]


@pytest.mark.parametrize("field", ["Fp", "Fq"])
def test_products_match_the_reference_form_limb_for_limb(lib, field):
    fc = FieldCase(field)
    seed = 1
    for sa, sb in fc.mul_pairs:
        run(lib, fc, 0, [fc.random(sa, RANDOM_CASES, seed), fc.random(sb, RANDOM_CASES, seed + 1)])
        run(lib, fc, 0, cross([fc.extremes(sa), fc.extremes(sb)]))
        seed += 2
    for sa in fc.sqr_shapes:
        run(lib, fc, 1, [fc.random(sa, RANDOM_CASES, seed)])
        run(lib, fc, 1, [np.array(fc.extremes(sa), dtype=np.uint32)])
        seed += 1
    for quad in fc.mam_quads:
        run(lib, fc, 2, [fc.random(s, RANDOM_CASES, seed + i) for i, s in enumerate(quad)])
        ext = [fc.extremes(s) for s in quad]
        run(lib, fc, 2, cross([ext[0], ext[1], ext[2][:4], ext[3][:4]]))
        run(lib, fc, 2, cross([ext[0][:4], ext[1][:4], ext[2], ext[3]]))
        seed += 4


@pytest.mark.parametrize("field", ["Fp", "Fq"])
def test_products_are_montgomery_products(lib, field):
    """The reference form is a copy: pin both to the definition, a b R^-1 mod p (+ e d R^-1), on the extreme operands, with
    the output contract (carry-normalised, below p + e)."""
    fc = FieldCase(field)
    ri = pow(1 << (LB * fc.RS), -1, fc.P)
    ops = cross([fc.extremes("wide"), fc.extremes("wide")])
    out = run(lib, fc, 0, ops, want_out=True)
    for a, b, r in zip(ops[0], ops[1], out):
        assert value_of(r) % fc.P == value_of(a) * value_of(b) * ri % fc.P
        assert value_of(r) < fc.P + fc.E and all(int(x) <= MASK for x in r[:-1])
    sq = [np.array(fc.extremes("wide"), dtype=np.uint32)]
    for a, r in zip(sq[0], run(lib, fc, 1, sq, want_out=True)):
        assert value_of(r) % fc.P == value_of(a) ** 2 * ri % fc.P and value_of(r) < fc.P + fc.E
    quad = fc.mam_quads[-1]
    ops = cross([fc.extremes(s)[:6] for s in quad])
    for a, b, e, d, r in zip(*ops, run(lib, fc, 2, ops, want_out=True)):
        assert value_of(r) % fc.P == (value_of(a) * value_of(b) + value_of(e) * value_of(d)) * ri % fc.P
        assert value_of(r) < fc.P + fc.E


def test_products_under_the_sanitizers():
    """The same comparison as a stand-alone program (its own main, its own operands) built with
    -fsanitize=undefined,address: no shift, overflow or out-of-bounds finding in either form, and no difference."""
    if _stale(EXE):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-DMONT_STEP_MAIN",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", EXE, SRC])
    res = subprocess.run([EXE], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "field 0: 0 differences" in res.stdout and "field 1: 0 differences" in res.stdout
