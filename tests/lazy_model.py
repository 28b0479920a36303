"""Contract model, operand generator and case tables for the primitive tests (TEST INFRASTRUCTURE, pure Python).

The lazy forms of csrc/field29.hpp (mul_lz, sqr_lz, mul_add_mul_lz, add_kp_sub, ...) are correct only for operands of
the shapes its comments name; tools/check_lazy_bounds.py proves on intervals that the point formulas stay inside them.
This module turns the same shapes -- imported from that script's shapes() table, not retyped -- into concrete limb
vectors AT the bounds, and states what every primitive must return for them, in exact integers.  The host tier
(tests/test_primitives_host.py, g++ build of the headers) and the device tier (tests/test_primitives_gpu.py, gfx950 build)
run the identical operand arrays through tests/native/primitives_ops.hpp and check the results with the functions here.

A shape is a BOX: an inclusive maximum per limb (what a 64-bit column sum sees) plus the proof's value bound `hi`.
"Every limb at its maximum" is the corner of the box -- for a stored coordinate: twelve limbs of 2^29 - 1 under a top limb
of MOD[12] + 64 -- which no point of the curve ever produces.  Shapes whose consumers need the VALUE bound itself
(canonical operands of add / sub / reduce_once / canon) are `strict`: the whole box lies below hi.
"""
import os
import random
import sys

import numpy as np

import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_lazy_bounds as B  # noqa: E402

LB = 29
BETA = 1 << LB
MASK = BETA - 1
N_RANDOM = 2000  # random vectors per shape, on top of the fixed edge set
N_RANDOM_POLY = 600  # per polynomial-map case of the curve formulas (their shapes have had N_RANDOM in the field cases)

# op numbers of tests/native/primitives_ops.hpp
FIELD_OPS = ["mul_lz", "sqr_lz", "mul_add_mul_lz", "mul", "sqr", "mul_sub_mul", "add", "sub", "neg", "reduce_once", "norm", "csub_mod", "csub_mod2",
             "csub_mod4", "canon", "add_kp2_sub", "add_kp6_sub", "add_kp4w3_sub_sub2", "kp2_sub", "add_lz", "inverse_mont"]
TE_OPS = ["madd", "madd_affine", "add", "finish", "from_base", "from_base_affine", "is_zero"]
G1_OPS = ["madd_lz", "add_lz", "canon_pt", "dbl", "dbl_affine"]
ED_OPS = ["madd", "add", "dbl", "dbl_nt", "make_base", "cneg"]


def value(limbs):
    return sum(int(x) << (LB * j) for j, x in enumerate(limbs))


def nform_limbs(v, n):
    """The carry-normalised limbs of v: limbs 0..n-2 below 2^29, the rest in the top limb (which must fit 32 bits)."""
    out = [(v >> (LB * j)) & MASK for j in range(n - 1)] + [v >> (LB * (n - 1))]
    assert 0 <= out[-1] < (1 << 32), hex(v)
    return out


class Shape:
    def __init__(self, name, box, hi, strict=False):
        self.name, self.box, self.hi, self.strict = name, list(box), hi, strict

    def holds(self, limbs):
        return len(limbs) == len(self.box) and all(0 <= x <= m for x, m in zip(limbs, self.box)) and (not self.strict or value(limbs) < self.hi)


class FieldModel:
    """One field of csrc/field29.hpp as the proof sees it: constants and shapes from tools/check_lazy_bounds.py."""

    def __init__(self, name):
        B.use_field(name)
        self.name, self.index = name, {"Fp": 0, "Fq": 1}[name]
        self.P, self.N, self.RS, self.E = B.P, B.N, B.RS, B.E
        self.MOD, self.K = list(B.MOD), {k: list(v) for k, v in B.K.items()}
        self.R = 1 << (LB * self.RS)  # Montgomery radix: 2^406 for Fp, 2^261 for Fq
        self.Rinv = pow(self.R, -1, self.P)
        self.shapes = {k: Shape(k, v.limbs, v.hi) for k, v in B.shapes().items()}
        # canonical operands feed add / sub / reduce_once, which need value < p: the strict form of the same bound
        self.shapes["canonical"] = self.nform_shape("canonical", self.P)

    def nform_shape(self, name, hi):
        """Carry-normalised values below hi, every vector of the box below hi."""
        top = (hi >> (LB * (self.N - 1))) - 1
        assert top >= 0
        return Shape(name, [MASK] * (self.N - 1) + [top], hi, strict=True)

    # ---- predicates, one per operand shape named in field29.hpp "Montgomery products" ----
    def is_nform(self, limbs, value_bound):
        return all(0 <= x <= MASK for x in limbs[:-1]) and 0 <= limbs[-1] < (1 << 32) and value(limbs) < value_bound

    def is_lazy(self, limbs):
        return self.shapes["lazy"].holds(limbs)

    def is_stored(self, limbs, xyzz_x=False):
        """The storage invariant of a bucket coordinate: carry-normalised, below p + e (X of XYZZ: 5p + e)."""
        return self.is_nform(limbs, (5 * self.P if xyzz_x else self.P) + self.E)

    def check_product(self, out_limbs, expected_residue, what=""):
        """Output contract of a lazy product: limbs 0..N-2 below 2^29, value below p + e, value = expected (mod p)."""
        assert all(0 <= x <= MASK for x in out_limbs[:-1]), ("limb not carry-normalised", what, [hex(x) for x in out_limbs])
        v = value(out_limbs)
        assert v < self.P + self.E, ("product not below p + e", what, hex(v))
        assert v % self.P == expected_residue % self.P, ("wrong residue", what, hex(v))

    def admits_product(self, pairs):
        """True when the proof's column model and value bound admit sum of a_i * b_i for the CORNERS of these boxes."""
        B.use_field(self.name)
        vs = [(B.V(a.box, value(a.box) + 1), B.V(b.box, value(b.box) + 1)) for a, b in pairs]
        try:
            B.check_columns(vs, "model")
        except AssertionError:
            return False
        return sum(value(a.box) * value(b.box) for a, b in pairs) // self.R + 1 <= self.E

    # ---- generator ----
    def vectors(self, shape, seed, n_random=None):
        """Deterministic limb vectors of a shape: the fixed edge set, then n_random vectors with every limb drawn from
        {0, its maximum, uniform}.  Every vector is asserted to lie in the shape; nothing is filtered."""
        if isinstance(shape, str):
            shape = self.shapes[shape]
        n, box = self.N, shape.box
        out = [list(box), [0] * n, [box[j] if j % 2 == 0 else 0 for j in range(n)], [box[j] if j % 2 == 1 else 0 for j in range(n)]]
        out += [[box[j] if j == k else 0 for j in range(n)] for k in range(n)]  # one hot limb; k = n - 1: top limb at its maximum over zeros
        out.append([0] * (n - 1) + [box[-1]])
        for v in (0, 1, self.P - 1, self.P, self.P + 1, 2 * self.P, self.P + self.E - 1):  # where the shape admits them
            if v < shape.hi and v >> (LB * (n - 1)) <= box[-1]:
                out.append(nform_limbs(v, n))
        self.n_edges = len(out)
        rnd = random.Random("%s/%s/%d" % (self.name, shape.name, seed))
        for _ in range(N_RANDOM if n_random is None else n_random):
            out.append([rnd.choice((0, m, rnd.randint(0, m), rnd.randint(0, m))) for m in box])
        for v in out:
            assert shape.holds(v), (shape.name, [hex(x) for x in v])
        return out


def arr(vectors):
    return np.array(vectors, dtype=np.uint32)


def zeros_like_cases(n, width):
    return np.zeros((n, width), dtype=np.uint32)


# ------------------------------------------------------------------ field operations ----

def product_shape_sets(fm):
    """Operand-shape pairs of the lazy products: N x N, lazy x N (the N operand narrow), and the call-site pairs of the
    point formulas.  Each one is checked against the proof's own column model before it is used."""
    s = fm.shapes
    pairs = [("wide", "wide"), ("lazy", "narrow"), ("narrow", "lazy"), ("stored", "stored"), ("canonical", "lazy"), ("stored", "canonical")]
    squares = ["wide", "stored"]
    if fm.name == "Fp":
        pairs += [("stored_x", "stored"), ("diff7", "stored"), ("stored_x", "canonical")]
        squares += ["stored_x", "diff7"]
        fused = [("diff3", "diff7", "kp2_sub", "stored"), ("stored", "stored", "stored", "stored")]
    else:
        fused = [("stored", "stored", "stored", "stored"), ("wide", "narrow", "lazy", "narrow")]
    for a, b in pairs:
        assert fm.admits_product([(s[a], s[b])]), (fm.name, a, b)
    for a in squares:
        assert fm.admits_product([(s[a], s[a])]), (fm.name, a)
    for a, b, c, d in fused:
        assert fm.admits_product([(s[a], s[b]), (s[c], s[d])]), (fm.name, a, b, c, d)
    return pairs, squares, fused


def subtrahend_shapes(fm, kname, w):
    """What add_kp_sub may subtract: at most w units of 2^29 per limb, a top limb up to K's (field29.hpp)."""
    k = fm.K[kname]
    assert all(x >= w * BETA for x in k[:-1]), kname
    return Shape(kname + "-b", [w * BETA] * (fm.N - 1) + [k[-1]], value(k) + 1)


def field_cases(fm, n_random=None):
    """[(op name, label, [a, b, c, d] as uint32 arrays of equal length)] -- operands an op ignores are zero."""
    s, n = fm.shapes, fm.N
    pairs, squares, fused = product_shape_sets(fm)
    cases = []

    full = set()

    def vec(shape, seed):
        # every shape gets its edge set every time and N_RANDOM random vectors the first time it is used; later uses
        # (other pairings of the same shape) take a quarter of that
        name = shape if isinstance(shape, str) else shape.name
        first = name not in full
        full.add(name)
        return fm.vectors(shape, seed, n_random if (n_random is not None or first) else N_RANDOM // 4)

    def add_case(op, label, *ops):
        # shapes admit different numbers of the fixed values: the shorter lists go round again, nothing is dropped
        m = max(len(o) for o in ops)
        full = [arr([o[i % len(o)] for i in range(m)]) for o in ops] + [zeros_like_cases(m, n)] * (4 - len(ops))
        cases.append((op, label, full))

    def rotated(v, k=1):  # a second pairing of the structural edges: the corner against every other edge
        e = 4 + n + 1
        return v[:e][k:] + v[:e][:k] + v[e:]

    for a, b in pairs:
        va, vb = vec(a, 1), vec(b, 2)
        add_case("mul_lz", "%s x %s" % (a, b), va, vb)
        if a == b:
            add_case("mul_lz", "%s x %s rotated" % (a, b), va, rotated(vb))
    for a in squares:
        add_case("sqr_lz", a, vec(a, 3))
    for sh in fused:
        add_case("mul_add_mul_lz", " ".join(sh), *[vec(x, 4 + i) for i, x in enumerate(sh)])
    can = [vec("canonical", 10 + i) for i in range(4)]
    add_case("mul", "canonical", can[0], can[1])
    add_case("mul", "canonical rotated", can[0], rotated(can[1], 3))
    add_case("mul", "%s x canonical" % ("stored_x" if fm.name == "Fp" else "stored"), vec("stored_x" if fm.name == "Fp" else "stored", 14), can[1])
    add_case("sqr", "canonical", can[0])
    add_case("mul_sub_mul", "canonical", *can)
    for op in ("add", "sub"):
        add_case(op, "canonical", can[0], can[1])
        add_case(op, "canonical rotated", can[0], rotated(can[1], 2))
        add_case(op, "a, a", can[0], can[0])
    add_case("neg", "canonical", can[0])
    add_case("reduce_once", "below 2p", vec(fm.nform_shape("below2p", 2 * fm.P), 20))
    # the sums reduce_once sees inside add(): limbs 0..N-2 normalised, the top limb carries the rest
    add_case("reduce_once", "p - 1 + k", [nform_limbs(fm.P - 1 + k, n) for k in (0, 1, 2, fm.P - 1, fm.P)])
    add_case("norm", "lazy", vec("lazy", 21))
    add_case("norm", "wide", vec("wide", 22))
    for op, m in (("csub_mod", 1), ("csub_mod2", 2), ("csub_mod4", 4)):
        add_case(op, "wide", vec("wide", 23))  # Fp: top limbs above 2^31, the int64_t `top` path
        add_case(op, "around %d p" % m, [nform_limbs(m * fm.P + d, n) for d in (-2, -1, 0, 1, 2)])
    add_case("canon", "below 8p", vec(fm.nform_shape("below8p", 8 * fm.P), 24))
    add_case("canon", "k p, k p +- 1", [nform_limbs(k * fm.P + d, n) for k in range(8) for d in (-1, 0, 1) if k * fm.P + d >= 0])
    for op, kname in (("add_kp2_sub", "KP2"), ("add_kp6_sub", "KP6")):
        bs = subtrahend_shapes(fm, kname, 1)
        add_case(op, "stored - allowance", vec("stored", 30), vec(bs, 31))
        add_case(op, "corner - allowance", [s["stored"].box] * 3, [bs.box, [0] * n, fm.K[kname]])
    k4 = fm.K["KP4W3"]
    t = k4[-1] // 3
    b1 = Shape("KP4W3-b", [BETA] * (n - 1) + [t], value(k4) + 1)
    add_case("add_kp4w3_sub_sub2", "stored - b - 2 b2", vec("stored", 32), vec(b1, 33), vec(b1, 34))
    # exactly the allowance: b + 2 b2 = 3 * 2^29 in every limb, K's top limb used up
    add_case("add_kp4w3_sub_sub2", "allowance", [s["stored"].box] * 3,
             [[BETA] * (n - 1) + [k4[-1] - 2 * t], [3 * BETA] * (n - 1) + [k4[-1]], [BETA - 2] * (n - 1) + [k4[-1] % 2]],
             [[BETA] * (n - 1) + [t], [0] * n, [BETA + 1] * (n - 1) + [k4[-1] // 2]])
    add_case("kp2_sub", "allowance", vec(subtrahend_shapes(fm, "KP2", 1), 35))
    add_case("kp2_sub", "stored", vec("stored", 36))
    add_case("add_lz", "stored + stored", vec("stored", 37), vec("stored", 38))
    add_case("add_lz", "lazy + canonical", vec("lazy", 39), vec("canonical", 40))
    add_case("inverse_mont", "edges, both arms, extreme k, random", [nform_limbs(a, n) for a, _, _ in inverse_cases(fm)])
    return cases


def check_field_case(fm, op, label, ins, out):
    """The contract of one field-op launch, in exact integers.  ins: four (n, N) arrays, out: (n, N)."""
    P, N, Ri = fm.P, fm.N, fm.Rinv
    A, Bv, C, D = (x.tolist() for x in ins)
    O = out.tolist()
    assert len(O) == len(A)
    for i in range(len(A)):
        a, b, c, d, o = A[i], Bv[i], C[i], D[i], O[i]
        va, vb, vc, vd, vo = value(a), value(b), value(c), value(d), value(o)
        what = (fm.name, op, label, i)
        if op == "mul_lz":
            fm.check_product(o, va * vb * Ri, what)
        elif op == "sqr_lz":
            fm.check_product(o, va * va * Ri, what)
        elif op == "mul_add_mul_lz":
            fm.check_product(o, (va * vb + vc * vd) * Ri, what)
        elif op in ("mul", "sqr", "mul_sub_mul", "add", "sub", "neg", "reduce_once", "canon"):
            exp = {"mul": va * vb * Ri, "sqr": va * va * Ri, "mul_sub_mul": (va * vb - vc * vd) * Ri, "add": va + vb, "sub": va - vb, "neg": -va,
                   "reduce_once": va, "canon": va}[op] % P
            assert o == nform_limbs(exp, N), (what, hex(vo), hex(exp))  # THE canonical residue, carry-normalised
        elif op == "inverse_mont":  # a = x R -> x^-1 R = a^-1 R^2, THE canonical residue
            assert o == nform_limbs(pow(va, -1, P) * fm.R * fm.R % P, N), (what, hex(va), hex(vo))
        elif op == "norm":
            assert vo == va and all(x <= MASK for x in o[:-1]), what
        elif op in ("csub_mod", "csub_mod2", "csub_mod4"):
            m = {"csub_mod": 1, "csub_mod2": 2, "csub_mod4": 4}[op] * P
            assert o == nform_limbs(va - m if va >= m else va, N), what
        elif op in ("add_kp2_sub", "add_kp6_sub", "add_kp4w3_sub_sub2", "kp2_sub", "add_lz"):
            if op == "add_lz":
                exp = [x + y for x, y in zip(a, b)]
            elif op == "kp2_sub":
                exp = [k - x for k, x in zip(fm.K["KP2"], a)]
            elif op == "add_kp4w3_sub_sub2":
                exp = [x + k - y - 2 * z for x, k, y, z in zip(a, fm.K["KP4W3"], b, c)]
            else:
                exp = [x + k - y for x, k, y in zip(a, fm.K["KP2" if op == "add_kp2_sub" else "KP6"], b)]
            assert all(0 <= x < (1 << 32) for x in exp), (what, "the case itself leaves the contract")
            assert o == exp, (what, [hex(x) for x in o], [hex(x) for x in exp])  # limb by limb, unmasked: nothing wrapped
        else:
            raise AssertionError("no contract for " + op)


# ------------------------------------------------------------------ the inversion walk ----

# fp_inverse.hpp / fq_inverse.hpp: the word count of the walk (its cap is 2 * 32 NW steps), and the k below which the
# conversion takes its two-factor arm: j1 = 2 * 29 RS - k > 376 (Fp: k < 436), > 252 (Fq: 522 - k > 252, k < 270).
INVERSE_WALK = {"Fp": {"cap": 2 * 384, "short_below": 812 - 376}, "Fq": {"cap": 2 * 256, "short_below": 522 - 252}}
INVERSE_SCAN = 100000  # seeded random residues searched for the extreme k
INVERSE_RANDOM = 256  # of them in the case list
INVERSE_EXTREMES = os.path.join(ROOT, "tests", "golden", "inverse_k_extremes.json")


def kaliski_k(fm, a):
    """k of Kaliski's phase 1 as the headers walk it: u = p, v = a mod p; one step per pass, the branches in their order
    (u even; v even; u > v; else), until v = 0 or the cap."""
    u, v, k, cap = fm.P, a % fm.P, 0, INVERSE_WALK[fm.name]["cap"]
    while v and k < cap:
        if not u & 1:
            u >>= 1
        elif not v & 1:
            v >>= 1
        elif u > v:
            u = (u - v) >> 1
        else:
            v = (v - u) >> 1
        k += 1
    return k


def kaliski_k_fast(fm, a):
    """The same k, a run of halvings at a time: a subtraction step halves once, and the even-operand steps that follow it
    each halve once more.  (The host test holds it against kaliski_k.)"""
    u, v, k = fm.P, a % fm.P, 0
    assert v
    tz = (v & -v).bit_length() - 1
    v >>= tz
    k += tz
    while True:
        if u > v:
            u -= v
            tz = (u & -u).bit_length() - 1
            u >>= tz
        else:
            v -= u
            if v == 0:
                return k + 1
            tz = (v & -v).bit_length() - 1
            v >>= tz
        k += tz


def inverse_random_residue(fm, i):
    """Seeded random residue number i in [1, p - 1]: addressable by index, so the scan's extremes can be named."""
    import hashlib

    return int.from_bytes(hashlib.sha512(b"inverse/%s/%d" % (fm.name.encode(), i)).digest(), "little") % (fm.P - 1) + 1


def inverse_edge_values(fm):
    """Montgomery 1, 2, p - 1, (p - 1) / 2 and the plain ones, every power of two below p plain and a few in Montgomery
    form, and the non-canonical a + p the stored box admits (the walk starts with a canonical product that reduces it)."""
    p, Rm = fm.P, fm.R
    vals = []
    for x in (1, 2, p - 1, (p - 1) // 2):
        vals += [(x * Rm % p, "%#x R" % x), (x, "%#x" % x)]
    j = 0
    while (1 << j) < p:
        vals.append((1 << j, "2^%d" % j))
        j += 1
    for j in (1, 29, 376 if fm.name == "Fp" else 252):
        vals.append(((1 << j) * Rm % p, "2^%d R" % j))
    rnd = random.Random("inverse-edges-" + fm.name)
    for a in (1, 2, 3, 1 << 29, rnd.randrange(1, fm.E), fm.E - 1 - (fm.P & MASK)):
        assert fm.shapes["stored"].holds(nform_limbs(a + p, fm.N)), hex(a)
        vals.append((a + p, "%#x + p" % a))
    return vals


def inverse_scan(fm, count=INVERSE_SCAN):
    """-> ((index, k) of the smallest k, (index, k) of the largest) over the first `count` seeded random residues; ties go
    to the lower index.  Seconds of pure Python: the host test runs it and pins tests/golden/inverse_k_extremes.json."""
    lo = hi = None
    for i in range(count):
        k = kaliski_k_fast(fm, inverse_random_residue(fm, i))
        if lo is None or k < lo[1]:
            lo = (i, k)
        if hi is None or k > hi[1]:
            hi = (i, k)
    return lo, hi


_INVERSE_CACHE = {}


def inverse_cases(fm):
    """[(a, k, label)]: the edge list, the scan's two extremes (from the pinned file, their k recomputed here) and
    INVERSE_RANDOM random residues."""
    import json

    if fm.name in _INVERSE_CACHE:
        return _INVERSE_CACHE[fm.name]
    with open(INVERSE_EXTREMES) as f:
        pinned = json.load(f)[fm.name]
    assert pinned["scanned"] == INVERSE_SCAN
    out = [(a, kaliski_k(fm, a), label) for a, label in inverse_edge_values(fm)]
    for which in ("min", "max"):
        i, k = pinned[which]
        a = inverse_random_residue(fm, i)
        assert kaliski_k(fm, a) == k, (fm.name, which)
        out.append((a, k, "%s k of the scan, residue %d" % (which, i)))
    out += [(inverse_random_residue(fm, i), None, "random %d" % i) for i in range(INVERSE_RANDOM)]
    out = [(a, kaliski_k(fm, a) if k is None else k, label) for a, k, label in out]
    _INVERSE_CACHE[fm.name] = out
    return out


# ------------------------------------------------------------------ twisted Edwards formulas ----

class CurveModel:
    """-x^2 + y^2 = 1 + d x^2 y^2 over the model's field: Te377's curve (Fp, d from tools/gen_consts.py) or Edwards-BLS12."""

    def __init__(self, fm):
        import util

        self.fm, self.p = fm, fm.P
        if fm.name == "Fp":
            te = util.te_params()
            self.d = te["d"] % self.p
            g = []
            for k in (1, 2, 3, 5, 12345, R.R_ORDER - 7):
                x, y = R.mul(R.G, k)
                u, v = te["s"] * (x + 1) % self.p, te["s"] * y % self.p
                g.append((te["c"] * u * pow(v, -1, self.p) % self.p, (u - 1) * pow(u + 1, -1, self.p) % self.p))
            self.points = g
        else:
            self.d = R.ED_D
            self.points = [R.ed_mul(R.ED_G, k) for k in (1, 2, 3, 5, 12345, R.ED_SUBGROUP - 7)]
        for pt in self.points:
            assert self.on_curve(pt)

    def on_curve(self, pt):
        x, y = pt
        return (-x * x + y * y - 1 - self.d * x * x * y * y) % self.p == 0

    def add(self, a, b):
        p = self.p
        t = self.d * a[0] * b[0] * a[1] * b[1] % p
        return ((a[0] * b[1] + a[1] * b[0]) * pow(1 + t, -1, p) % p, (a[1] * b[1] + a[0] * b[0]) * pow(1 - t, -1, p) % p)

    def neg(self, a):
        return ((-a[0]) % self.p, a[1])

    def ext_values(self, pt, lam):
        """(X, Y, T, Z) of pt scaled by lam, as stored (Montgomery) integers below p."""
        p, Rm = self.p, self.fm.R
        x, y = pt
        return [x * lam * Rm % p, y * lam * Rm % p, x * y * lam * Rm % p, lam * Rm % p]

    def base_values(self, pt, mu):
        """PBase (Y - X, Y + X, 2d T, 2Z) of pt scaled by mu; mu = 1 gives the ABase in the first three."""
        p, Rm = self.p, self.fm.R
        x, y = pt
        return [(y - x) * mu * Rm % p, (y + x) * mu * Rm % p, 2 * self.d * x * y * mu * Rm % p, 2 * mu * Rm % p]

    def check_ext(self, words, expected, what):
        """A stored Ext: the storage invariant, T Z = X Y, Z != 0, and the point it names (projectively)."""
        fm, p, n = self.fm, self.p, self.fm.N
        co = [words[n * c : n * c + n] for c in range(4)]
        for c in co:
            assert fm.is_stored(c), ("storage invariant", what, [hex(x) for x in c])
        X, Y, T, Z = (value(c) % p for c in co)  # the common factor R drops out of every comparison below
        assert Z != 0, what
        assert (X * Y - T * Z) % p == 0, ("T Z = X Y", what)
        assert (X - expected[0] * Z) % p == 0 and (Y - expected[1] * Z) % p == 0, ("wrong point", what)


def edge_targets(fm, rnd):
    """Stored values one coordinate of a real point is steered to: (value, also as value + p)."""
    n = fm.N
    lowmax = ((fm.MOD[-1] - 1) << (LB * (n - 1))) | ((1 << (LB * (n - 1))) - 1)  # all low limbs at 2^29 - 1, below p
    small = rnd.randrange(1, fm.E)  # below the slack e: v + p is a representative the storage invariant admits
    return [(1, True), (fm.P - 1, False), (lowmax, False), (small, True), (fm.E - 1, True)]


def te_point_cases(cm):
    """Real points with edge representations, for madd / madd_affine / add.
    -> dict op -> (p array, q array, neg array, [expected affine point], [label])"""
    fm, p, n = cm.fm, cm.p, cm.fm.N
    rnd = random.Random("te-points-" + fm.name)
    out = {op: ([], [], [], [], []) for op in ("madd", "madd_affine", "add")}

    def emit(op, pv, qv, neg, exp, label):
        pl = [x for v in pv for x in nform_limbs(v, n)]
        ql = [x for v in qv for x in nform_limbs(v, n)]
        o = out[op]
        o[0].append(pl), o[1].append(ql), o[2].append(neg), o[3].append(exp), o[4].append(label)

    def all_ops(pv, ppt, qpt, neg, label):
        exp = cm.add(ppt, cm.neg(qpt) if neg else qpt)
        emit("madd", pv, cm.base_values(qpt, rnd.randrange(1, p)), neg, exp, label)
        emit("madd_affine", pv, cm.base_values(qpt, 1)[:3] + [0], neg, exp, label)
        if not neg:
            qv = cm.ext_values(qpt, rnd.randrange(1, p))
            emit("add", pv, qv, 0, exp, label)
            emit("add", qv, pv, 0, exp, label + " swapped")

    P0, Q0 = cm.points[4], cm.points[5]
    for rel, (ppt, qpt) in (("generic", (P0, Q0)), ("P = Q", (P0, P0)), ("P = -Q", (P0, cm.neg(P0)))):
        for neg in (0, 1):
            for c, cname in enumerate("XYTZ"):
                coord = [ppt[0], ppt[1], ppt[0] * ppt[1] % p, 1][c]
                for tv, plus_p in edge_targets(fm, rnd):
                    lam = tv * pow(coord * fm.R, -1, p) % p
                    pv = cm.ext_values(ppt, lam)
                    assert pv[c] == tv % p
                    all_ops(pv, ppt, qpt, neg, "%s neg=%d %s -> %#x" % (rel, neg, cname, tv))
                    if plus_p:
                        pv2 = list(pv)
                        pv2[c] += p
                        all_ops(pv2, ppt, qpt, neg, "%s neg=%d %s -> %#x + p" % (rel, neg, cname, tv))
    ident = (0, 1)
    one = fm.R % p
    for neg in (0, 1):
        for qpt in cm.points[:3]:
            all_ops([0, one, 0, one], ident, qpt, neg, "identity() + Q")
            cst = rnd.randrange(1, p)
            all_ops([0, cst, 0, cst], ident, qpt, neg, "(0, c, 0, c) + Q")
            all_ops([p, cst, 0, cst], ident, qpt, neg, "(p, c, 0, c) + Q")  # X = 0 stored as exactly p
            small = rnd.randrange(1, fm.E)
            all_ops([0, small + p, p, small], ident, qpt, neg, "(0, c + p, p, c) + Q")
    for i in range(40):  # plain random representations of random pairs
        ppt, qpt = rnd.choice(cm.points), rnd.choice(cm.points)
        all_ops(cm.ext_values(ppt, rnd.randrange(1, p)), ppt, qpt, i % 2, "random")
    return {op: (arr(o[0]), arr(o[1]), np.array(o[2], dtype=np.uint32), o[3], o[4]) for op, o in out.items()}


def check_te_point_case(cm, op, case, out, flags):
    _, _, _, exps, labels = case
    O = out.tolist()
    for i, (exp, label) in enumerate(zip(exps, labels)):
        cm.check_ext(O[i], exp, (cm.fm.name, op, label, i))
        assert flags[i] == 0, ("is_bad on a finite sum", cm.fm.name, op, label)


def te_poly_cases(cm, n_random=None):
    """finish / madd / madd_affine / add as polynomial maps on in-contract quadruples that are no curve points: the only
    way to have every coordinate of every operand at the corner of its box at once."""
    fm, n = cm.fm, cm.fm.N
    n_random = N_RANDOM_POLY if n_random is None else n_random
    st = [fm.vectors("stored", 50 + i, n_random) for i in range(8)]
    can = [fm.vectors("canonical", 60 + i, n_random) for i in range(4)]
    dbl = Shape("2 x stored", [2 * m for m in fm.shapes["stored"].box], 2 * fm.shapes["stored"].hi)  # finish's d may be limb-wise doubled
    m = min(len(st[0]), len(can[0]))

    def cat(vs):
        return arr([sum((v[i] for v in vs), []) for i in range(m)])

    neg = np.array([i % 2 for i in range(m)], dtype=np.uint32)
    zero = np.zeros(m, dtype=np.uint32)
    lazy_kt = can[:2] + [st[6]] + can[3:]  # an affine record's kt is a lazy product, not canonical
    return {
        "finish": (cat(st[:4]), cat(st[4:]), zero),
        "finish 2d": (cat(st[:3] + [[v for v in fm.vectors(dbl, 58, n_random)][:m]]), cat(st[4:]), zero),
        "madd": (cat(st[:4]), cat(can), neg),
        "madd_affine": (cat(st[:4]), cat(lazy_kt), neg),
        "add": (cat(st[:4]), cat(st[4:]), zero),
    }


def check_te_poly_case(cm, name, case, out):
    """out against the hwcd-3 polynomials on Python integers, up to one common non-zero factor; storage invariant."""
    fm, p, n, d2 = cm.fm, cm.p, cm.fm.N, 2 * cm.d % cm.p
    Ri = fm.Rinv
    Pv, Qv, Ng = case[0].tolist(), case[1].tolist(), case[2].tolist()
    O = out.tolist()
    op = name.split()[0]
    for i in range(len(Pv)):
        x1, y1, t1, z1 = (value(Pv[i][n * c : n * c + n]) * Ri % p for c in range(4))  # stored s names the element s / R
        q = [value(Qv[i][n * c : n * c + n]) * Ri % p for c in range(4)]
        if op == "finish":
            a, b, c, d = x1, y1, t1, z1
        elif op in ("madd", "madd_affine"):
            ymx, ypx, kt, z2 = q
            if Ng[i]:
                ymx, ypx, kt = ypx, ymx, -kt
            a, b, c = (y1 - x1) * ymx, (y1 + x1) * ypx, kt * t1
            d = z1 * z2 if op == "madd" else 2 * z1
        else:
            x2, y2, t2, z2 = q
            a, b, c, d = (y1 - x1) * (y2 - x2), (y1 + x1) * (y2 + x2), d2 * t1 * t2, 2 * z1 * z2
        e, f, g, h = (b - a) % p, (d - c) % p, (d + c) % p, (b + a) % p
        exp = [e * f % p, g * h % p, e * h % p, f * g % p]
        co = [O[i][n * c : n * c + n] for c in range(4)]
        what = (fm.name, name, i)
        for c in co:
            assert fm.is_stored(c), ("storage invariant", what, [hex(x) for x in c])
        got = [value(c) % p for c in co]
        for j in range(4):
            assert (got[j] == 0) == (exp[j] == 0), ("zero pattern", what, j)
            for k in range(j + 1, 4):
                assert (got[j] * exp[k] - got[k] * exp[j]) % p == 0, ("not the same projective quadruple", what, j, k)


def te_from_base_cases(cm):
    """from_base / from_base_affine (Te377 only): canonical records of real points -> the first Ext of a chain."""
    rnd = random.Random("from-base")
    p = cm.p
    out = {}
    for op, mus in (("from_base", (1, p - 1, rnd.randrange(1, p))), ("from_base_affine", (1,))):  # an affine record has Z = 1
        rows, negs, exps = [], [], []
        for pt in cm.points:
            for neg in (0, 1):
                for mu in mus:
                    rows.append([x for v in cm.base_values(pt, mu) for x in nform_limbs(v, cm.fm.N)])
                    negs.append(neg)
                    exps.append(cm.neg(pt) if neg else pt)
        out[op] = (arr(rows), np.array(negs, dtype=np.uint32), exps)
    return out


def te_zero_cases(fm):
    """is_zero_mod_p / is_bad: a coordinate that is 0 mod p is stored as all-zero limbs or as exactly p."""
    n, p = fm.N, fm.P
    vals = [(0, 1), (p, 1), (p + 1, 0), (p - 1, 0), (1, 0), (2 * p, 0), (p + fm.E - 1, 0)]  # 2p is above p + e: never stored, not recognised
    rows, exp = [], []
    one = nform_limbs(fm.R % p, n)
    for vx, fx in vals:
        for vz, fz in vals:
            rows.append(nform_limbs(vx, n) + one + one + nform_limbs(vz, n))
            exp.append(fx | (fz << 1))
    return arr(rows), exp


# ------------------------------------------------------------------ G1 XYZZ formulas ----

def _sqrt_p(v):
    import gen_consts

    return gen_consts._sqrt_p(v % R.P) if v % R.P else 0


def xyzz_values(pt, z):
    p, Rm = R.P, 1 << (LB * 14)
    zz, zzz = z * z % p, z * z * z % p
    return [pt[0] * zz * Rm % p, pt[1] * zzz * Rm % p, zz * Rm % p, zzz * Rm % p]


def steer_xyzz(pt, which, target):
    """z with coordinate `which` (X = x z^2, Y = y z^3, ZZ = z^2, ZZZ = z^3) stored as a value at or just above
    target: the target moves up until target / (x R), / (y R) or / R is a square (X, ZZ) or a cube (Y, ZZZ)."""
    p, Rm = R.P, 1 << (LB * 14)
    assert (p - 1) % 3 == 0 and (p - 1) // 3 % 3 != 0  # 3 divides p - 1 exactly once: a cubic residue has the root c^(1/3 mod (p-1)/3)
    cube_exp = pow(3, -1, (p - 1) // 3)
    t = target
    while True:
        c = t * pow((Rm, pt[0] * Rm, pt[1] * Rm)[(2, 0, 1).index(which) if which != 3 else 0], -1, p) % p
        if which in (0, 2):
            z = _sqrt_p(c) if pow(c, (p - 1) // 2, p) == 1 else None
        else:
            z = pow(c, cube_exp, p) if pow(c, (p - 1) // 3, p) == 1 else None
            assert z is None or pow(z, 3, p) == c
        if z:
            return z, t
        t += 1


def g1_point_cases(fm):
    """Real points in edge representations for G1::madd_lz / add_lz: X as x + k p for k = 0..4 (the stored X may be anything
    below 5p + e), each of X, Y, ZZ, ZZZ in turn steered to 1, to all-low-limbs-max, to values below e (stored as v and
    as v + p; X also as v + 2p .. v + 4p), P = Q, P = -Q, identity accumulators.  -> dict op -> (a, q, neg, [expected affine or None], [label])"""
    p, n = R.P, 13
    rnd = random.Random("g1-points")
    Rm = fm.R
    pts = [R.mul(R.G, k) for k in (1, 2, 3, 12345, R.R_ORDER - 7)]
    out = {op: ([], [], [], [], []) for op in ("madd_lz", "add_lz")}

    def emit(op, av, qv, neg, exp, label):
        o = out[op]
        o[0].append([x for v in av for x in nform_limbs(v, n)])
        o[1].append([x for v in qv for x in nform_limbs(v, n)])
        o[2].append(neg), o[3].append(exp), o[4].append(label)

    def both(av, apt, qpt, neg, label):
        exp = R.add(apt, R.neg(qpt) if neg else qpt)
        emit("madd_lz", av, [qpt[0] * Rm % p, qpt[1] * Rm % p, 0, 0], neg, exp, label)
        if not neg:
            qv = xyzz_values(qpt, rnd.randrange(1, p))
            emit("add_lz", av, qv, 0, exp, label)
            emit("add_lz", qv, av, 0, exp, label + " swapped")

    steer = steer_xyzz
    lowmax = ((fm.MOD[-1] - 1) << (LB * 12)) | ((1 << (LB * 12)) - 1 - 64)
    A, Q = pts[3], pts[4]
    for rel, (apt, qpt) in (("generic", (A, Q)), ("P = Q", (A, A)), ("P = -Q", (A, R.neg(A)))):
        for neg in (0, 1):
            av = xyzz_values(apt, rnd.randrange(1, p))
            for k in range(5):
                both([av[0] + k * p] + av[1:], apt, qpt, neg, "%s neg=%d X + %d p" % (rel, neg, k))
            for which, cname in ((0, "X"), (1, "Y"), (2, "ZZ"), (3, "ZZZ")):
                for target, plus_p in ((1, True), (lowmax, False), (rnd.randrange(1, fm.E >> 1), True), (fm.E - 1000, True)):
                    z, t = steer(apt, which, target)
                    av = xyzz_values(apt, z)
                    assert av[which] == t
                    both(av, apt, qpt, neg, "%s neg=%d %s -> %#x" % (rel, neg, cname, t))
                    if plus_p:
                        for k in (range(1, 5) if which == 0 else (1,)):
                            av2 = list(av)
                            av2[which] += k * p
                            both(av2, apt, qpt, neg, "%s neg=%d %s -> %#x + %d p" % (rel, neg, cname, t, k))
    one = Rm % p
    for neg in (0, 1):
        for qpt in pts[:3]:
            both([0, one, 0, 0], None, qpt, neg, "identity() + Q")
            both([rnd.randrange(p), rnd.randrange(p), 0, rnd.randrange(p)], None, qpt, neg, "(x, y, 0, zzz) + Q")
    for i in range(40):
        apt, qpt = rnd.choice(pts), rnd.choice(pts)
        both(xyzz_values(apt, rnd.randrange(1, p)), apt, qpt, i % 2, "random")
    emit("add_lz", [0, one, 0, 0], [0, one, 0, 0], 0, None, "identity + identity")
    return {op: (arr(o[0]), arr(o[1]), np.array(o[2], dtype=np.uint32), o[3], o[4]) for op, o in out.items()}


def check_g1_words(fm, words, exp, what):
    """A stored XYZZ point: storage invariant (X below 5p + e, the others below p + e, carry-normalised) and its value."""
    import util

    co = [words[13 * c : 13 * c + 13] for c in range(4)]
    assert fm.is_stored(co[0], xyzz_x=True), ("X storage invariant", what)
    for c in co[1:]:
        assert fm.is_stored(c), ("storage invariant", what)
    assert util.affine_from_xyzz_words(words) == exp, ("wrong point", what)


def g1_two_torsion():
    """The three points (x, 0) of y^2 = x^3 + 1: x^3 = -1."""
    import util

    p = R.P
    tp = util.t_prime()
    xs = [p - 1, tp[0], (1 - tp[0]) % p]
    for x in xs:
        assert R.on_curve((x, 0))
    return xs


def g1_dbl_cases(fm):
    """Every stored representation of a real point for the strict G1::dbl (the one place where a non-canonical stored point
    meets strict arithmetic, through canon_pt): X as x + k p while below 5p + e, each of X, Y, ZZ, ZZZ steered below e and
    stored as v and as v + p, the 2-torsion points with Y = 0 and with Y = p (the double is the identity and ZZ must come
    back zero limb by limb), an identity operand.  -> (a rows, [expected affine or None], [label])"""
    p, n = R.P, 13
    rnd = random.Random("g1-dbl")
    pts = [R.mul(R.G, k) for k in (1, 2, 3, 12345, R.R_ORDER - 7)]
    rows, exps, labels = [], [], []
    xmax, omax = fm.shapes["stored_x"].hi, fm.shapes["stored"].hi

    def emit(av, exp, label):
        assert av[0] < xmax and all(v < omax for v in av[1:]), label
        rows.append([x for v in av for x in nform_limbs(v, n)])
        exps.append(exp), labels.append(label)

    for i, pt in enumerate(pts):
        av = xyzz_values(pt, rnd.randrange(1, p))
        for k in range(5):
            emit([av[0] + k * p] + av[1:], R.add(pt, pt), "point %d X + %d p" % (i, k))
    A = pts[3]
    for which, cname in ((0, "X"), (1, "Y"), (2, "ZZ"), (3, "ZZZ")):
        for target in (1, rnd.randrange(1, fm.E >> 1), fm.E - 1000):
            z, t = steer_xyzz(A, which, target)
            av = xyzz_values(A, z)
            assert av[which] == t
            for k in range(6 if which == 0 else 2):
                av2 = list(av)
                av2[which] += k * p
                emit(av2, R.add(A, A), "%s -> %#x + %d p" % (cname, t, k))
    for x in g1_two_torsion():
        for z in (1, rnd.randrange(1, p)):
            av = xyzz_values((x, 0), z)
            for y in (0, p):
                for k in range(5):
                    emit([av[0] + k * p, y] + av[2:], None, "2-torsion x = %#x.. Y = %s X + %d p" % (x >> 340, "p" if y else "0", k))
    emit([rnd.randrange(p), rnd.randrange(p), 0, rnd.randrange(p)], None, "identity operand (x, y, 0, zzz)")
    emit([0, fm.R % p, 0, 0], None, "identity()")
    return arr(rows), exps, labels


def g1_dbl_affine_cases(fm):
    """Canonical affine points for G1::dbl_affine, the 2-torsion points among them.  -> (q rows, [expected], [label])"""
    p, Rm = R.P, fm.R
    pts = [R.mul(R.G, k) for k in (1, 2, 3, 5, 12345, R.R_ORDER - 7, R.R_ORDER - 1)] + [(x, 0) for x in g1_two_torsion()]
    rows = [[x for v in (pt[0] * Rm % p, pt[1] * Rm % p, 0, 0) for x in nform_limbs(v, 13)] for pt in pts]
    return arr(rows), [R.add(pt, pt) for pt in pts], ["point %d" % i for i in range(len(pts))]


def check_g1_doubles(fm, out, exps, labels, op):
    for i, o in enumerate(out.tolist()):
        check_g1_words(fm, o, exps[i], (op, labels[i]))
        if exps[i] is None:
            assert o[26:39] == [0] * 13, ("the identity is ZZ = 0 limb by limb", op, labels[i])


def ed_strict_cases(cm):
    """The strict Edwards-BLS12 formulas (ed_ext.hpp EdT: canonical in, canonical out) on real points: one coordinate of
    the first operand steered to 1, q - 1, all-low-limbs-max and a small value, generic / equal / opposite pairs, identity
    and order-2 operands, random representations.
    -> dict op -> (p rows, q rows, neg, [expected], [label]); expected is an affine point, or for make_base / cneg the three
    exact record values."""
    fm, p, n = cm.fm, cm.p, cm.fm.N
    assert fm.name == "Fq"
    rnd = random.Random("ed-strict")
    out = {op: ([], [], [], [], []) for op in ED_OPS}

    def emit(op, pv, qv, neg, exp, label):
        assert all(0 <= v < p for v in pv + qv), label  # canonical operands only
        o = out[op]
        o[0].append([x for v in pv for x in nform_limbs(v, n)]), o[1].append([x for v in qv for x in nform_limbs(v, n)])
        o[2].append(neg), o[3].append(exp), o[4].append(label)

    def all_ops(pv, ppt, qpt, label):
        emit("madd", pv, cm.base_values(qpt, 1)[:3] + [0], 0, cm.add(ppt, qpt), label)
        qv = cm.ext_values(qpt, rnd.randrange(1, p))
        emit("add", pv, qv, 0, cm.add(ppt, qpt), label)
        emit("add", qv, pv, 0, cm.add(ppt, qpt), label + " swapped")
        for op in ("dbl", "dbl_nt"):
            emit(op, pv, [0] * 4, 0, cm.add(ppt, ppt), label)

    P0, Q0 = cm.points[4], cm.points[5]
    order2 = (0, p - 1)
    assert cm.on_curve(order2)
    for rel, (ppt, qpt) in (("generic", (P0, Q0)), ("P = Q", (P0, P0)), ("P = -Q", (P0, cm.neg(P0))), ("P + order 2", (P0, order2)), ("order 2 + Q", (order2, Q0))):
        for c, cname in enumerate("XYTZ"):
            coord = [ppt[0], ppt[1], ppt[0] * ppt[1] % p, 1][c]
            if coord == 0:
                continue
            for tv, _ in edge_targets(fm, rnd):
                lam = tv * pow(coord * fm.R, -1, p) % p
                pv = cm.ext_values(ppt, lam)
                assert pv[c] == tv % p
                all_ops(pv, ppt, qpt, "%s %s -> %#x" % (rel, cname, tv))
    one = fm.R % p
    for qpt in cm.points[:3] + [(0, 1), order2]:
        all_ops([0, one, 0, one], (0, 1), qpt, "identity() + Q")
        cst = rnd.randrange(1, p)
        all_ops([0, cst, 0, cst], (0, 1), qpt, "(0, c, 0, c) + Q")
    for i in range(40):
        ppt, qpt = rnd.choice(cm.points), rnd.choice(cm.points)
        all_ops(cm.ext_values(ppt, rnd.randrange(1, p)), ppt, qpt, "random")
    for pt in cm.points + [(0, 1), order2]:
        rec = cm.base_values(pt, 1)[:3]
        emit("make_base", [pt[0] * fm.R % p, pt[1] * fm.R % p, 0, 0], [0] * 4, 0, rec, "make_base")
        for neg in (0, 1):
            emit("cneg", [0] * 4, rec + [0], neg, cm.base_values(cm.neg(pt), 1)[:3] if neg else rec, "cneg neg=%d" % neg)
    return {op: (arr(o[0]), arr(o[1]), np.array(o[2], dtype=np.uint32), o[3], o[4]) for op, o in out.items()}


def check_ed_strict_case(cm, op, case, out):
    fm, p, n = cm.fm, cm.p, cm.fm.N
    for i, (o, exp, label) in enumerate(zip(out.tolist(), case[3], case[4])):
        what = ("Ed", op, label, i)
        co = [o[n * c : n * c + n] for c in range(4)]
        for c in co:
            assert c == nform_limbs(value(c) % p, n) and value(c) < p, ("not canonical", what)
        if op in ("make_base", "cneg"):
            assert [value(c) for c in co] == list(exp) + [0], ("wrong record", what)
            continue
        X, Y, T, Z = (value(c) for c in co)
        assert Z != 0 and (X - exp[0] * Z) % p == 0 and (Y - exp[1] * Z) % p == 0, ("wrong point", what)
        if op == "dbl_nt":
            assert T == 0, what
        else:  # T Z = X Y up to the Montgomery factor both sides carry once: stored values s = v R
            assert (T * Z - X * Y) % p == 0, ("T Z = X Y", what)


_GUARD_CACHE = {}


def guard_false_positive_cases(fm, m=1 << 12):
    """Real points for which the P of an XYZZ addition has its low limb inside the guard's range WITHOUT being 0 mod p:
    the false-positive side of `(p.l[0] - 1u) < 3u` (add_lz, g1_add_quad: P = U2 + 2p - U1) and of `(p.l[0] - 1u) < 7u`
    (madd_lz: P = U2 + 6p - X1), which must then fall through canon() to the ordinary formula.  A random pair gets there
    with probability 3 / 2^29 (7 / 2^29), so the low limbs of two growing pools of candidates (multiples of G under two
    fixed scalings) are matched instead.  The search uses a Python model of mul_lz's representative; it is only a way to
    FIND candidates -- check_guard_cases() establishes from the real mul_lz outputs that the guard is hit.
    -> {"add_lz": (a rows, b rows, [expected affine], [low limb of P]), "madd_lz": the same with b = (x, y, 0, 0)}"""
    if fm.name in _GUARD_CACHE:
        return _GUARD_CACHE[fm.name]
    p, Rm = R.P, fm.R
    rnd = random.Random("guard")
    za, zb = rnd.randrange(1, p), rnd.randrange(1, p)
    zza, zzb = za * za % p * Rm % p, zb * zb % p * Rm % p
    pinv = pow(p, -1, Rm)

    def low(a, b):  # low limb of (a b + Q p) / R with Q = -a b / p mod R
        ab = a * b
        return ((ab + (-ab * pinv % Rm) * p) // Rm) & MASK

    pa, pb, u1, x1 = [], [], {}, {}
    add_found, madd_found = {}, {}
    a, b = R.mul(R.G, 1000003), R.mul(R.G, 2000003)
    while len(add_found) < 3 or len(madd_found) < 3:  # about 2^15.5 points in each pool
        assert len(pa) < (1 << 19), "no low-limb match in pools this large: the search itself is broken"
        for _ in range(m):
            xa = a[0] * za * za % p * Rm % p
            u1.setdefault(low(xa, zzb), len(pa))  # add_lz: U1 = X_a ZZ_b
            x1.setdefault(xa & MASK, len(pa))  # madd_lz: X1 itself
            pa.append(a)
            pb.append((b, low(b[0] * zb * zb % p * Rm % p, zza), low(b[0] * Rm % p, zza)))  # U2 = X_b ZZ_a; U2 = x_b ZZ_a
            a, b = R.add(a, R.G), R.add(b, R.G)
        for j, (_, l2, l2m) in enumerate(pb):
            for w in (1, 2, 3):  # low limb of P = (u2 - u1 + 2) mod 2^29 (KP2[0] = 2^29 + 2)
                i = u1.get((l2 + 2 - w) & MASK)
                if i is not None and w not in add_found:
                    add_found[w] = (i, j)
            for w in range(1, 8):  # low limb of P = (u2 - x1 + 6) mod 2^29 (KP6[0] = 2^29 + 6)
                i = x1.get((l2m + 6 - w) & MASK)
                if i is not None and w not in madd_found:
                    madd_found[w] = (i, j)
    out = {}
    for op, found in (("add_lz", add_found), ("madd_lz", madd_found)):
        rows_a, rows_b, exps, lows = [], [], [], []
        for w in sorted(found):
            i, j = found[w]
            av = xyzz_values(pa[i], za)
            bv = xyzz_values(pb[j][0], zb) if op == "add_lz" else [pb[j][0][0] * Rm % p, pb[j][0][1] * Rm % p, 0, 0]
            rows_a.append([x for v in av for x in nform_limbs(v, 13)])
            rows_b.append([x for v in bv for x in nform_limbs(v, 13)])
            exps.append(R.add(pa[i], pb[j][0]))
            lows.append(w)
        out[op] = (arr(rows_a), arr(rows_b), exps, lows)
    _GUARD_CACHE[fm.name] = out
    return out


def check_guard_cases(backend, fm, op, a, b, lows):
    """The guard cases really are guard cases for THIS build: U1 and U2 come from the backend's own mul_lz, whatever
    representative it returns, and the low limb of P = U2 + K - U1 (add_lz: K = 2p; madd_lz: K = 6p, X1 in place of U1)
    computed from them is the wanted 1..3 (1..7) while P is not 0 mod p."""
    n = len(a)
    zero = zeros_like_cases(n, 13)
    ax, azz, bx, bzz = a[:, 0:13], a[:, 26:39], b[:, 0:13], b[:, 26:39]
    u2 = backend.field(fm, "mul_lz", [bx, azz, zero, zero]).tolist()
    if op == "add_lz":
        u1, k, hi = backend.field(fm, "mul_lz", [ax, bzz, zero, zero]).tolist(), fm.K["KP2"], 3
    else:
        u1, k, hi = ax.tolist(), fm.K["KP6"], 7
    for i in range(n):
        pv = value(u2[i]) + value(k) - value(u1[i])
        assert pv & MASK == lows[i] and 1 <= lows[i] <= hi, (op, "the case does not hit the guard with this build's mul_lz", i, pv & MASK)
        assert pv % fm.P != 0, (op, i)


# ------------------------------------------------------------------ the affine conversion's wire map ----

def aff_wire_cases(n_random=200):
    """Wire points for AffWireSource::load: random subgroup points, the on-curve points with a coordinate in {0, 1, p - 1},
    and the points the Edwards model cannot represent (y = 0: the three points of order 2; s (x + 1) = -1: order 4).
    -> (raw (n, 24) array, [(point, expect_flag)])"""
    import util

    p = R.P
    te = util.te_params()
    rnd = random.Random("aff-wire")
    pts = []
    g = R.mul(R.G, rnd.randrange(1, R.R_ORDER))
    step = R.mul(R.G, rnd.randrange(1, R.R_ORDER))
    for _ in range(n_random):
        pts.append((g, 0))
        g = R.add(g, step)
    for x in (0, 1, p - 1):
        y = _sqrt_p(x ** 3 + 1) if pow((x ** 3 + 1) % p, (p - 1) // 2, p) in (0, 1) else None
        if y is not None:
            for yy in {y, (-y) % p}:
                assert R.on_curve((x, yy))
                pts.append(((x, yy), 1 if yy == 0 else 0))
    tp = util.t_prime()
    pts.append((tp, 1))
    w2 = (1 - tp[0]) % p  # the third root of x^3 = -1: the three roots sum to zero
    assert R.on_curve((w2, 0))
    pts.append(((w2, 0), 1))
    x4 = (-1 - pow(te["s"], -1, p)) % p
    y4 = _sqrt_p(x4 ** 3 + 1)
    pts += [((x4, y4), 1), ((x4, (-y4) % p), 1)]
    raw = [[(c >> (32 * i)) & 0xFFFFFFFF for c in pt for i in range(12)] for pt, _ in pts]
    return arr(raw), pts


def check_aff_wire(fm, pts, out, flags):
    import util

    p = R.P
    te = util.te_params()
    O = out.tolist()
    for i, (pt, bad) in enumerate(pts):
        n1, n2, z = O[i][0:13], O[i][13:26], O[i][26:39]
        what = ("AffWireSource::load", i, pt)
        assert flags[i] == bad, what
        assert fm.is_stored(n1) and fm.is_stored(z), ("n1, z below p + e", what)
        assert fm.is_nform(n2, 5 * p + fm.E), ("n2 N-form below 5p + e", what)
        if bad:
            assert value(z) % p == 0, what
            continue
        u, v = te["s"] * (pt[0] + 1) % p, te["s"] * pt[1] % p
        xe, ye = te["c"] * u * pow(v, -1, p) % p, (u - 1) * pow(u + 1, -1, p) % p
        zi = pow(value(z), -1, p)
        assert value(n1) * zi % p == xe and value(n2) * zi % p == ye, ("n1 / z, n2 / z", what)


# ------------------------------------------------------------------ bucket records ----

RECORD_KINDS = {0: ("TeDev", 13, 16), 1: ("EdDev", 9, 12), 2: ("G1Dev", 13, 16)}  # name, limbs, words of a coordinate slot


def record_cases(nl, n_random=300):
    """Packed points (4 x nl words) for the record round trip: all-ones words in every position, each single position
    all-ones, counting patterns that tell every word of every lane apart, random words."""
    w = 4 * nl
    rnd = random.Random("records-%d" % nl)
    rows = [[0xFFFFFFFF] * w, [0] * w]
    rows += [[0xFFFFFFFF if j == k else 0 for j in range(w)] for k in range(w)]
    rows += [[(i << 16) | j for j in range(w)] for i in range(64)]
    rows += [[rnd.getrandbits(32) for _ in range(w)] for _ in range(n_random)]
    return arr(rows)


# ------------------------------------------------------------------ the two builds of primitives_ops.hpp ----

CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
SHIM_SO = os.path.join(NATIVE, "_build", "libfield29_shim.so")
# (MSM377_PRIMTEST_SO: a build of the test library against a copy of csrc/ with a seeded fault, tests/PRIMITIVES.md)
PRIMTEST_SO = os.environ.get("MSM377_PRIMTEST_SO") or os.path.join(CSRC, "libmsm377_primtest.so")
PRIMTEST_ENTRY_POINTS = ["primtest_field", "primtest_te", "primtest_g1", "primtest_ed", "primtest_add_quad", "primtest_madd_quad", "primtest_aff_wire", "primtest_records",
                         "primtest_normalise_g1", "primtest_normalise_ed", "primtest_normalise_guard"]


def build_shim(csrc=CSRC, so=SHIM_SO):
    """g++ build of tests/native/field29_shim.cpp against the headers under csrc (another copy: a seeded fault)."""
    import subprocess

    src = os.path.join(NATIVE, "field29_shim.cpp")
    deps = [src, os.path.join(NATIVE, "primitives_ops.hpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", csrc, "-I", NATIVE, "-o", so, src])
    return so


def _p(a):
    import ctypes

    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class Backend:
    """The raw-limb entry points of the host shim (prefix shim_raw_) or of the gfx950 test library (prefix primtest_)."""

    def __init__(self, path, device):
        import ctypes

        self.lib, self.device = ctypes.CDLL(path), device
        self.prefix = "primtest_" if device else "shim_raw_"

    def _call(self, name, *args):
        import ctypes

        fn = getattr(self.lib, self.prefix + name)
        fn.restype = ctypes.c_int if self.device else None
        rc = fn(*args)
        assert not self.device or rc == 0, "%s%s: HIP status %d" % (self.prefix, name, rc)

    def field(self, fm, op, ins):
        ins = [np.ascontiguousarray(x) for x in ins]
        out = np.zeros_like(ins[0])
        self._call("field", fm.index, FIELD_OPS.index(op), *[_p(x) for x in ins], _p(out), len(out))
        return out

    def te(self, fm, op, p, q, neg):
        p, q, neg = np.ascontiguousarray(p), np.ascontiguousarray(q), np.ascontiguousarray(neg)
        assert p.shape == q.shape == (len(neg), 4 * fm.N)
        out, flags = np.zeros_like(p), np.zeros(len(p), dtype=np.uint32)
        self._call("te", fm.index, TE_OPS.index(op), _p(p), _p(q), _p(neg), _p(out), _p(flags), len(p))
        return out, flags

    def g1(self, op, a, q, neg):
        a, q, neg = np.ascontiguousarray(a), np.ascontiguousarray(q), np.ascontiguousarray(neg)
        assert a.shape == q.shape == (len(neg), 52)
        out = np.zeros_like(a)
        self._call("g1", G1_OPS.index(op), _p(a), _p(q), _p(neg), _p(out), len(a))
        return out

    def ed(self, op, p, q, neg):
        p, q, neg = np.ascontiguousarray(p), np.ascontiguousarray(q), np.ascontiguousarray(neg)
        assert p.shape == q.shape == (len(neg), 36)
        out = np.zeros_like(p)
        self._call("ed", ED_OPS.index(op), _p(p), _p(q), _p(neg), _p(out), len(p))
        return out

    # ---- device only ----
    def normalise(self, curve, form, pts, with_inf=True):
        """k_bm_up / k_bm_across / k_bm_down<form> (curve "g1": form 0 wire, 1 mont_flag, 2 table) or the k_edbm_* three
        (curve "ed": form 0 wire, 1 table) on the stash rows pts.  -> (records (n, record bytes) uint8, the guard band behind
        them, flag bytes (n,) or None, their guard band or None); with_inf=False hands the kernel a null out_inf."""
        import ctypes

        pts = np.ascontiguousarray(pts)
        n, w = pts.shape
        rec = {"g1": (96, 104, 128), "ed": (64, 128)}[curve][form]
        assert w == {"g1": 52, "ed": 36}[curve] and n >= 1
        guard = self.lib.primtest_normalise_guard()
        out = np.zeros(n * rec + guard, dtype=np.uint8)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        if curve == "ed":
            self._call("normalise_ed", form, _p(pts), n, out.ctypes.data_as(u8))
            return out[: n * rec].reshape(n, rec), out[n * rec :], None, None
        inf = np.zeros(n + guard, dtype=np.uint8) if with_inf else None
        self._call("normalise_g1", form, _p(pts), n, out.ctypes.data_as(u8), inf.ctypes.data_as(u8) if with_inf else None)
        return out[: n * rec].reshape(n, rec), out[n * rec :], (inf[:n] if with_inf else None), (inf[n:] if with_inf else None)

    def add_quad(self, kind, a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        n, w = a.shape
        out, flags = np.zeros((n, 4, w), dtype=np.uint32), np.zeros((n, 4), dtype=np.uint32)
        self._call("add_quad", kind, _p(a), _p(b), _p(out), _p(flags), n)
        return out, flags

    def madd_quad(self, fm, a, b, neg):
        a, b, neg = np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(neg)
        n, w = a.shape
        out = np.zeros((n, 4, w), dtype=np.uint32)
        self._call("madd_quad", fm.index, _p(a), _p(b), _p(neg), _p(out), n)
        return out

    def aff_wire(self, raw):
        raw = np.ascontiguousarray(raw)
        n = len(raw)
        out, flags = np.zeros((n, 39), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._call("aff_wire", _p(raw), _p(out), _p(flags), n)
        return out, flags

    def records(self, kind, pts):
        pts = np.ascontiguousarray(pts)
        n, w = pts.shape
        slot = RECORD_KINDS[kind][2]
        rec, rec2 = np.zeros((n, 4 * slot), dtype=np.uint32), np.zeros((n, 4 * slot), dtype=np.uint32)
        out_t, out_q = np.zeros((n, w), dtype=np.uint32), np.zeros((n, 4, w), dtype=np.uint32)
        self._call("records", kind, _p(pts), _p(rec), _p(out_t), _p(out_q), _p(rec2), n)
        return rec, out_t, out_q, rec2


def _report_override(var, path):
    """An override makes a green run say nothing about the repository's own code: it is reported in pytest's summary."""
    import warnings

    warnings.warn("%s is set: the primitive tests run against %s, NOT the repository's own build" % (var, path))


def device_backend():
    """The gfx950 test library build() made -- a missing library is an error, not a skip."""
    assert os.path.exists(PRIMTEST_SO), "%s is missing: build() makes it (make -C csrc)" % PRIMTEST_SO
    if os.environ.get("MSM377_PRIMTEST_SO"):
        _report_override("MSM377_PRIMTEST_SO", PRIMTEST_SO)
    return Backend(PRIMTEST_SO, device=True)


def host_backend():
    """The host shim over the repository's headers -- or, with MSM377_CSRC_COPY naming another copy of csrc/ (one with a
    seeded fault, tests/PRIMITIVES.md), over that copy: the suite must then fail."""
    copy = os.environ.get("MSM377_CSRC_COPY")
    if copy:
        _report_override("MSM377_CSRC_COPY", copy)
        return Backend(build_shim(copy, os.path.join(NATIVE, "_build", "libfield29_shim_%s.so" % os.path.basename(copy.rstrip("/")))), device=False)
    return Backend(build_shim(), device=False)
