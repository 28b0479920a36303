#!/usr/bin/env python3
"""Worst-case bounds of the lazy G1 formulas (csrc/g1_xyzz.hpp madd_lz / add_lz, msm377.hip g1_add_quad).

Every field value is tracked as (limb upper bounds[13], value upper bound, value lower bound); the script replays
the formulas on those intervals and asserts, for every product, that no 64-bit column accumulator of
csrc/field29.hpp (mul_lz, sqr_lz, mul_add_mul_lz) can overflow, for every add_kp_sub that no limb can go negative,
and that the results satisfy the storage invariant the next addition assumes:

    X: N-form, value < 5p + 2^354        Y, ZZ, ZZZ: N-form, value < p + 2^354

normalisation_formulas() replays the batch calls' normalisation (kernels/batch_mul.hpp k_bm_up / k_bm_across / k_bm_down,
kernels/ed_batch_mul.hpp k_edbm_*) the same way, from the stash shapes of NORMALISATION_OPERANDS;
tests/test_normalise_gpu.py puts exactly those operands into the stash on the GPU.

The operand shapes live in ONE table, shapes(): main() reads the ones it starts from (canonical, stored, stored_x) from there, and so do the
primitive tests (tests/lazy_model.py), which feed the real field29.hpp / te377.hpp / g1_xyzz.hpp code operands at exactly
these bounds on the host and on the GPU -- tests/test_primitives_host.py::test_shape_table_is_the_proofs pins the two together.

Run by tests/test_field29_host.py::test_lazy_bounds_proof; exits non-zero on any violation.
"""
import os
import re
import sys

P_FP = 0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001
Q_FQ = 8444461749428370424248824938781546531375899335154063827935233455917409239041
LB = 29
LINCOMB_MAX_TERMS = 8  # MSM377_LINCOMB_MAX_TERMS: consecutive additions of one step of kernels/ed_batch_lincomb.hpp
BETA = 1 << LB
MASK = BETA - 1
# the field under test (use_field): modulus, limbs, reduction steps, slack of a lazy product above the modulus
P, N, RS, E, MOD, K = None, None, None, None, None, None


def load_consts(struct, end, n, rs):
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "webgpu-msm-bls12-377_amd", "csrc", "consts_gen.hpp")).read()
    body = text[text.index("struct " + struct) : text.index(end)]
    out = {}
    for name in ("KP2", "KP6", "KP4W3", "MOD", "MOD2", "MOD4"):
        m = re.search(r"uint32_t %s\[%d\] = \{([^}]*)\}" % (name, n), body)
        out[name] = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    assert "RS = %d" % rs in body
    return out


def use_field(which):
    global P, N, RS, E, MOD, K
    if which == "Fp":
        P, N, RS, E = P_FP, 13, 14, 1 << 354
        K = load_consts("G1Consts", "struct GlvConsts", N, RS)
    else:  # Fq: R = 2^261 = 438 q; a lazy product of values below 5q exceeds q by less than q / 16
        P, N, RS, E = Q_FQ, 9, 9, Q_FQ // 16
        K = load_consts("EdConsts", "struct G1Consts64", N, RS)
    MOD = [(P >> (LB * j)) & MASK for j in range(N)]
    assert K["MOD"] == MOD
    for name, k in (("KP2", 2), ("KP6", 6), ("KP4W3", 4), ("MOD2", 2), ("MOD4", 4)):
        assert sum(x << (LB * j) for j, x in enumerate(K[name])) == k * P, name


class V:
    """Interval model of one 13-limb value."""

    def __init__(self, limbs, hi, lo=0, name=""):
        self.limbs, self.hi, self.lo, self.name = list(limbs), hi, lo, name
        assert all(0 <= x < (1 << 32) for x in self.limbs), (name, [hex(x) for x in self.limbs])

    @property
    def normalised(self):
        return all(x <= MASK for x in self.limbs[:-1])


def nform(hi, lo=0, name=""):
    """Carry-normalised value below hi: limbs 0..11 <= 2^29 - 1, top limb <= (hi - 1) >> 348."""
    return V([MASK] * (N - 1) + [(hi - 1) >> (LB * (N - 1))], hi, lo, name)


# The generic operand shapes of the lazy products (field29.hpp "Montgomery products"): top limb of an N-form value
# below 2^31.6 (2^29.1 when the other operand is lazy), a lazy value has limbs below 3 * 2^29 and a top limb below 2^31.
NFORM_TOP = int(2 ** 31.6)
NARROW_TOP = int(2 ** 29.1)
LAZY_LIMB = 3 * BETA
LAZY_TOP = 1 << 31


def shapes():
    """The operand shapes of the field in use, name -> V, and what the primitive tests generate.  canonical, stored and
    stored_x are what the replays below START from (main(), te_formulas, conversion_formulas, normalisation_formulas).  The others are not inputs
    of a replay: wide / narrow / lazy restate field29.hpp's comment, diff3 / diff7 / kp2_sub name intermediate values, and
    they are tied to the replay only where it asserts that its own values fit them (point_formula, conversion_formulas --
    Fp; the Fq pass consumes none of them) and where a caller runs check_columns on them (tests/lazy_model.py
    admits_product).  A V's limbs are inclusive per-limb maxima (what a column sum sees), hi the exclusive value bound.
        canonical  base records, constants                                         < p
        stored     a lazy product: Y, ZZ, ZZZ of XYZZ, every Edwards coordinate,
                   kt of an affine record                                          < p + e
        stored_x   X of XYZZ (Fp only)                                             < 5p + e
        wide       the widest carry-normalised operand of a product: Fp top limb < 2^31.6 (P and D of madd_lz, below
                   7p + e, fit); Fq a value below 5q (use_field: the radix 2^261 carries products of such values)
        narrow     the N-form partner of a lazy operand: Fp top limb < 2^29.1; Fq a stored value
        lazy       one limb-wise add_kp_sub / add_lz of such values, not carry-normalised
        diff3, diff7, kp2_sub (Fp)  the operands of Y3 = R D + (2p - Y1) PPP: R below 3p + e, D (and P of madd_lz) below
                   7p + e, 2p - Y1 limb-wise (KP2's limbs); point_formula() checks that its values fit them"""
    t = {
        "canonical": nform(P, 0, "canonical"),
        "stored": nform(P + E, 0, "stored"),
    }
    if N == 13:
        t["stored_x"] = nform(5 * P + E, 0, "stored_x")
        t["diff3"] = nform(3 * P + E, 0, "diff3")
        t["diff7"] = nform(7 * P + E, 0, "diff7")
        t["kp2_sub"] = V(list(K["KP2"]), 2 * P + 1, 0, "kp2_sub")
        t["wide"] = V([MASK] * (N - 1) + [NFORM_TOP - 1], NFORM_TOP << (LB * (N - 1)), 0, "wide")
        t["narrow"] = V([MASK] * (N - 1) + [NARROW_TOP - 1], NARROW_TOP << (LB * (N - 1)), 0, "narrow")
        t["lazy"] = V([LAZY_LIMB - 1] * (N - 1) + [LAZY_TOP - 1], (LAZY_TOP << (LB * (N - 1))) + (LAZY_LIMB << (LB * (N - 2))), 0, "lazy")
    else:
        t["wide"] = nform(5 * P, 0, "wide")
        t["narrow"] = nform(P + E, 0, "narrow")
        top = max(K["KP2"][N - 1], t["stored"].limbs[N - 1]) + t["stored"].limbs[N - 1]
        t["lazy"] = V([LAZY_LIMB - 1] * (N - 1) + [top], ((top + 1) << (LB * (N - 1))) + (LAZY_LIMB << (LB * (N - 2))), 0, "lazy")
    assert 7 * P + E <= t["wide"].hi or N != 13
    return t


def m1(name=""):
    s = shapes()["stored"]
    return V(s.limbs, s.hi, 0, name)


def check_columns(pairs, what):
    """pairs: list of (a, b) products accumulated into the same columns, plus RS reduction rows."""
    worst = 0
    for k in range(2 * N):
        s = 0
        for a, b in pairs:
            for i in range(N):
                j = k - i
                if 0 <= j < N:
                    s += a.limbs[i] * b.limbs[j]
        for i in range(RS):  # q_i * MOD[j], q_i <= 2^29 - 1; j = 0 is the implicit + q
            j = k - i
            if 0 <= j < N:
                s += MASK * MOD[j]
        s += 1 << 40  # carry from the column below (a column is < 2^64, >> 29 leaves < 2^35)
        if k < RS:  # a column that a reduction step consumes starts from 2^29 - 1 (field29.hpp column_bias)
            s += MASK
        worst = max(worst, s)
    assert worst < (1 << 64), "%s: column sum 2^%.2f" % (what, __import__("math").log2(worst))
    return worst


def product_value(pairs):
    return sum(a.hi * b.hi for a, b in pairs) // (1 << (LB * RS)) + 1 + P


def mul_lz(a, b, name):
    check_columns([(a, b)], name)
    hi = product_value([(a, b)])
    assert hi <= P + E, (name, hi / P)
    return m1(name)


def sqr_lz(a, name):
    assert a.normalised, name  # 2 * a_i must fit 32 bits for i <= 11
    return mul_lz(a, a, name)


def mul_add_mul_lz(a, b, e, d, name):
    check_columns([(a, b), (e, d)], name)
    hi = product_value([(a, b), (e, d)])
    assert hi <= P + E, (name, hi / P)
    return m1(name)


def add_kp_sub(a, kname, k, b, name, b2=None):
    """a + K - b (- 2 b2): limb-wise; K = k p."""
    Kl = K[kname]
    limbs = []
    for j in range(N):
        sub = b.limbs[j] + (2 * b2.limbs[j] if b2 else 0)
        assert Kl[j] >= sub, "%s: limb %d of %s (%#x) below the subtrahend bound %#x" % (name, j, kname, Kl[j], sub)
        limbs.append(a.limbs[j] + Kl[j])
    sub_hi = b.hi + (2 * b2.hi if b2 else 0)
    sub_lo = b.lo + (2 * b2.lo if b2 else 0)
    return V(limbs, a.hi + k * P - sub_lo, max(0, a.lo + k * P - sub_hi), name)


def kp_sub(kname, k, b, name):
    Kl = K[kname]
    for j in range(N):
        assert Kl[j] >= b.limbs[j], (name, j)
    return V(list(Kl), k * P - b.lo + 1, max(0, k * P - b.hi), name)


def add_lz(a, b, name):
    return V([x + y for x, y in zip(a.limbs, b.limbs)], a.hi + b.hi, a.lo + b.lo, name)


def norm(a, name):
    assert a.hi < (1 << (LB * (N - 1) + 32)), (name, a.hi / P)  # the top limb must fit 32 bits
    return nform(a.hi, a.lo, name)


def canon_ok(a, name):
    assert a.normalised and a.hi <= 8 * P, (name, a.hi / P)


def point_formula(x1, y1, zz1, zzz1, u_in, s_in, kp_p, kname_p, p_mults, tag):
    """Shared tail of madd_lz (u_in = U2, X1 = x1, ...) and add_lz (x1 = U1, y1 = S1)."""
    p = norm(add_kp_sub(u_in, kname_p, kp_p, x1, tag + " P"), tag + " P")
    r = norm(add_kp_sub(s_in, "KP2", 2, y1, tag + " R"), tag + " R")
    # P = 0 mod p <=> P in {p, .., p_mults p}: the guard (P.l[0] - 1) < p_mults must cover the whole range
    assert p.lo > 0 and p.hi <= (p_mults + 1) * P and r.lo > 0, (tag, p.lo, p.hi / P)
    canon_ok(p, tag + " canon(P)")
    canon_ok(r, tag + " canon(R)")
    pp = sqr_lz(p, tag + " PP")
    ppp = mul_lz(p, pp, tag + " PPP")
    qq = mul_lz(x1, pp, tag + " Q")
    rr = sqr_lz(r, tag + " RR")
    x3 = norm(add_kp_sub(rr, "KP4W3", 4, ppp, tag + " X3", b2=qq), tag + " X3")
    assert x3.hi <= 5 * P + E, (tag, x3.hi / P)
    d = norm(add_kp_sub(qq, "KP6", 6, x3, tag + " D"), tag + " D")
    sh = shapes()
    assert r.hi <= sh["diff3"].hi and p.hi <= sh["diff7"].hi and d.hi <= sh["diff7"].hi, tag
    y3 = mul_add_mul_lz(r, d, kp_sub("KP2", 2, y1, tag + " -Y1"), ppp, tag + " Y3")
    return x3, y3, pp, ppp, r, d, qq


def te_formulas(canonical):
    """te377.hpp TeLazy: every stored coordinate is a lazy product (M1), base records canonical."""

    def te_finish(a, b, c, d, tag):
        e = norm(add_kp_sub(b, "KP2", 2, a, tag + " E"), tag + " E")
        f = norm(add_kp_sub(d, "KP2", 2, c, tag + " F"), tag + " F")
        g = norm(add_lz(d, c, tag + " G"), tag + " G")
        h = add_lz(b, a, tag + " H")
        return [mul_lz(x, y, "%s %s" % (tag, nm)) for nm, (x, y) in (("X3", (e, f)), ("Y3", (h, g)), ("T3", (h, e)), ("Z3", (f, g)))]

    PX, PY, PT, PZ = m1("PX"), m1("PY"), m1("PT"), m1("PZ")
    a = mul_lz(add_kp_sub(PY, "KP2", 2, PX, "te madd Y-X"), canonical, "te madd A")
    b = mul_lz(add_lz(PY, PX, "te madd Y+X"), canonical, "te madd B")
    c = mul_lz(kp_sub("KP2", 2, canonical, "te madd -kt"), PT, "te madd C")
    d = mul_lz(PZ, canonical, "te madd D")
    te_finish(a, b, c, d, "te madd")
    a = mul_lz(norm(add_kp_sub(PY, "KP2", 2, PX, "te add Y1-X1"), "te add Y1-X1"), norm(add_kp_sub(PY, "KP2", 2, PX, "te add Y2-X2"), "te add Y2-X2"), "te add A")
    b = mul_lz(norm(add_lz(PY, PX, "te add Y1+X1"), "te add Y1+X1"), norm(add_lz(PY, PX, "te add Y2+X2"), "te add Y2+X2"), "te add B")
    c = mul_lz(mul_lz(PT, PT, "te add T1T2"), canonical, "te add C")
    d = mul_lz(PZ, PZ, "te add D")
    te_finish(a, b, c, add_lz(d, d, "te add 2D"), "te add")
    # madd_affine: A, B, C as in madd, D = 2 Z1 limb-wise
    a = mul_lz(add_kp_sub(PY, "KP2", 2, PX, "te amadd Y-X"), canonical, "te amadd A")
    b = mul_lz(add_lz(PY, PX, "te amadd Y+X"), canonical, "te amadd B")
    c = mul_lz(kp_sub("KP2", 2, canonical, "te amadd -kt"), PT, "te amadd C")
    te_finish(a, b, c, add_lz(PZ, PZ, "te amadd 2Z"), "te amadd")
    # dbl / dbl_nt (dbl_any): four lazy squares, then the four products on factors of the opposite sign.  What it reads
    # and what it returns are stored coordinates, so the walk of kernels/ed_batch_mul_var.hpp is replayed as a chain:
    # the start values, dbl after madd_affine, dbl after dbl, madd_affine after dbl.
    def te_dbl(x, y, z, tag):
        a, b, zz = sqr_lz(x, tag + " A"), sqr_lz(y, tag + " B"), sqr_lz(z, tag + " ZZ")
        s = sqr_lz(norm(add_lz(x, y, tag + " X+Y"), tag + " X+Y"), tag + " S")
        h = add_lz(a, b, tag + " H")
        g = norm(add_kp_sub(a, "KP2", 2, b, tag + " G"), tag + " G")
        e = norm(add_kp_sub(h, "KP2", 2, s, tag + " E"), tag + " E")
        f = norm(add_lz(add_lz(zz, zz, tag + " 2ZZ"), g, tag + " F"), tag + " F")
        assert g.lo > 0 and e.lo > 0 and f.hi <= 5 * P + 3 * E and e.hi <= 4 * P + 2 * E, (tag, f.hi / P, e.hi / P)
        return [mul_lz(u, v, "%s %s" % (tag, nm)) for nm, (u, v) in (("X3", (e, f)), ("Y3", (h, g)), ("T3", (h, e)), ("Z3", (f, g)))]

    def te_amadd(x, y, t, z, tag):
        a = mul_lz(add_kp_sub(y, "KP2", 2, x, tag + " Y-X"), canonical, tag + " A")
        b = mul_lz(add_lz(y, x, tag + " Y+X"), canonical, tag + " B")
        mul_lz(canonical, t, tag + " C")
        c = mul_lz(kp_sub("KP2", 2, canonical, tag + " -kt"), t, tag + " C neg")
        return te_finish(a, b, c, add_lz(z, z, tag + " 2Z"), tag)

    zero, one = V([0] * N, 1, 0, "0"), canonical  # identity(): (0, 1, 0, 1)
    acc = te_amadd(zero, one, zero, one, "te start amadd")  # acc = carry ? P : O
    x, y, t, z = te_dbl(zero, one, one, "te dbl of the start value")
    for pt, tag in ((acc, "te dbl after amadd"), ((x, y, t, z), "te dbl after dbl")):
        x, y, t, z = te_dbl(pt[0], pt[1], pt[3], tag)
    te_amadd(x, y, t, z, "te amadd after dbl")
    # The joint walk of kernels/ed_batch_lincomb2.hpp: two additions per step.  New against the chain above: madd_affine
    # directly after madd_affine (the second term reads what the first returned, T included), dbl_nt after two additions,
    # and both of step 64, the carries': an addition to O and one to what that returned.
    first = te_amadd(zero, one, zero, one, "te l2 carry amadd")
    second = te_amadd(*first, "te l2 carry amadd after amadd")
    first = te_amadd(x, y, t, z, "te l2 amadd after dbl")
    second = te_amadd(*first, "te l2 amadd after amadd")
    for pt, tag in ((second, "te l2 dbl after two amadd"), (first, "te l2 dbl after one amadd")):
        te_amadd(*te_dbl(pt[0], pt[1], pt[3], tag), tag + ", amadd")
    # The k-term walk of kernels/ed_batch_lincomb.hpp: up to LINCOMB_MAX_TERMS additions per step, each reading what the one
    # before returned with no normalisation between them -- after a doubling, and after the start value O (step 64, the
    # carries') -- and the next step's first dbl_nt on what ANY number of them returned (zero digits sit their addition out).
    for start, tag in (((x, y, t, z), "te lk after dbl"), ((zero, one, zero, one), "te lk carries")):
        pt = start
        for j in range(1, LINCOMB_MAX_TERMS + 1):
            pt = te_amadd(*pt, "%s, amadd %d" % (tag, j))
            te_amadd(*te_dbl(pt[0], pt[1], pt[3], "%s, dbl after %d amadd" % (tag, j)), "%s, dbl after %d amadd, amadd" % (tag, j))

    # canonical operations on stored (lazy) coordinates: mul() = reduce_once(mul_lz()) needs mul_lz < 2p
    mul_lz(PX, canonical, "gather X*TO64")


def csub_mod(a, name):
    """field29.hpp csub(x, MOD): x N-form; subtracts p once if x >= p."""
    assert a.normalised, name
    return nform(max(P, a.hi - P), 0, name)


def conversion_formulas():
    """kernels/convert.hpp, the batched affine conversion in lazy forms (AffWireSource::load, k_affine_up, k_affine_down)."""
    canonical = shapes()["canonical"]
    zero = V([0] * N, 1, 0, "zero")
    u = add_lz(mul_lz(canonical, canonical, "conv x*SR"), canonical, "conv u")
    v = mul_lz(canonical, canonical, "conv v")
    cu = csub_mod(norm(add_lz(mul_lz(canonical, canonical, "conv x*CSR"), canonical, "conv cu"), "conv cu"), "conv cu")
    assert cu.hi <= P + E, cu.hi / P
    up = add_lz(u, canonical, "conv u+1")
    assert all(x <= y for x, y in zip(up.limbs, shapes()["lazy"].limbs))  # a lazy operand; v is its N-form partner
    assert v.limbs[-1] <= shapes()["narrow"].limbs[-1]
    z = mul_lz(up, v, "conv z")
    n1 = mul_lz(up, cu, "conv n1")
    n2 = norm(add_kp_sub(z, "KP4W3", 4, zero, "conv n2", b2=v), "conv n2")
    assert n2.lo > 0 and n2.hi <= 5 * P + E, (n2.lo, n2.hi / P)
    c = mul_lz(m1("c"), z, "conv c*z")
    node = mul_lz(c, c, "conv tree node")
    root = mul_lz(node, canonical, "conv root*TO64")  # then reduce_once: needs < 2p
    assert root.hi <= 2 * P
    inv = mul_lz(canonical, node, "conv tree down")  # the host's inverse is canonical; further down N x N
    inv = mul_lz(inv, node, "conv tree down 2")
    zi = mul_lz(inv, c, "conv zi")
    inv = mul_lz(inv, z, "conv inv*Z")
    x = mul_lz(n1, zi, "conv x")  # then reduce_once -> canonical
    y = mul_lz(n2, zi, "conv y")
    assert x.hi <= 2 * P and y.hi <= 2 * P
    kt = mul_lz(mul_lz(canonical, canonical, "conv xy"), canonical, "conv 2dxy")
    # the record's kt is now a lazy product, its y -+ x stay canonical: replay the affine mixed addition with it
    PX, PY, PT, PZ = m1("PX"), m1("PY"), m1("PT"), m1("PZ")
    mul_lz(kp_sub("KP2", 2, kt, "conv-rec -kt"), PT, "conv-rec C neg")
    mul_lz(kt, PT, "conv-rec C")
    mul_lz(kt, canonical, "conv-rec first: kt / d")  # from_base_affine: mul(kt, TE_INV_D), reduce_once needs < 2p


# The stash rows the batch calls' normalisation starts from (g1_xyzz.hpp's storage invariant; ed_batch_mul.hpp "Canonical
# coordinates in"): coordinate -> name in shapes().  tests/normalise_model.py builds its corner operands from this table.
NORMALISATION_OPERANDS = {
    "Fp": {"X": "stored_x", "Y": "stored", "ZZ": "stored", "ZZZ": "stored"},
    "Fq": {"X": "canonical", "Y": "canonical", "T": "canonical", "Z": "canonical"},
}


def reduce_once_ok(a, name):
    """field29.hpp reduce_once: limbs below 2^29 except the top one (< 2^31), value < 2p."""
    assert a.normalised and a.limbs[-1] < (1 << 31) and a.hi <= 2 * P, (name, a.hi / P)


def normalisation_formulas():
    """kernels/batch_mul.hpp k_bm_up / k_bm_across / k_bm_down (Fp) and kernels/ed_batch_mul.hpp k_edbm_* (Fq) from the
    stash shapes of NORMALISATION_OPERANDS: the per-thread running product, both product trees, the inversion's first
    product, the trees walked down, the unfolding, zi, tt, x, y and the last product into each output form.  Every product
    goes through check_columns (mul_lz / sqr_lz above); the value assertions are the ones the source comments make."""
    sh = shapes()
    canonical = sh["canonical"]
    ops = {k: sh[v] for k, v in NORMALISATION_OPERANDS["Fp" if N == 13 else "Fq"].items()}

    def closed(v, name):  # "M1 is closed under mul_lz": the product is again a stored value, limb box and value bound
        assert v.limbs == sh["stored"].limbs and v.hi == sh["stored"].hi and v.normalised, name
        return v

    def tree(leaf, tag):  # eight levels of pairwise products of nodes of one shape; the root
        node = leaf
        for level in range(8):
            node = closed(mul_lz(node, node, "%s tree level %d" % (tag, level)), tag)
        return node

    def tree_down(root_inv, node, tag):  # inv_k * sibling: the first level takes the kernel's input, the others a product
        inv = closed(mul_lz(root_inv, node, tag + " down from the root"), tag)
        for level in range(1, 8):
            inv = closed(mul_lz(inv, node, "%s down level %d" % (tag, level)), tag)
        return inv

    if N == 13:
        one = canonical  # Fp::one(), and the 1 an identity contributes in place of its ZZZ = 0
        # k_bm_up: c = 1, then c = c * z four times, z a stored ZZZ or 1
        c = closed(mul_lz(one, ops["ZZZ"], "up c0*z"), "up")
        mul_lz(one, one, "up c0*1")
        c = closed(mul_lz(c, ops["ZZZ"], "up c*z"), "up")
        mul_lz(c, one, "up c*1")
        block = tree(c, "up")
        # k_bm_across: the same one level up, the factors now workgroup products
        c = closed(mul_lz(one, block, "across c0*prod"), "across")
        c = closed(mul_lz(c, block, "across c*prod"), "across")
        root = tree(c, "across")
        reduce_once_ok(mul_lz(root, one, "inverse a*1"), "inverse a*1")  # FpInverse::inverse_mont: Fp::mul(a, one())
        inv_root = canonical  # ... and its result is a canonical product
        inv = tree_down(inv_root, c, "across")
        closed(mul_lz(inv, one, "across inv*c0"), "across")  # the unfolding: 1 / product_b = (1 / C_(b+1)) C_b
        closed(mul_lz(inv, c, "across inv*c"), "across")
        binv = closed(mul_lz(inv, block, "across inv*prod"), "across")
        # k_bm_down: the workgroup tree from block_inv, then per output
        inv = tree_down(binv, block, "down")
        zi = closed(mul_lz(inv, one, "down zi, first output"), "down")
        zi = closed(mul_lz(inv, c, "down zi"), "down")
        inv = closed(mul_lz(inv, ops["ZZZ"], "down inv*ZZZ"), "down")
        tt = closed(mul_lz(zi, ops["ZZ"], "down tt"), "down")
        sq = closed(sqr_lz(tt, "down tt^2"), "down")  # sqr_lz asserts its operand carry-normalised
        x = closed(mul_lz(ops["X"], sq, "down x"), "down")  # X: N-form below 5p + e, the square below p + e
        y = closed(mul_lz(ops["Y"], zi, "down y"), "down")
        for v, nm in ((x, "x"), (y, "y")):
            reduce_once_ok(v, "table record " + nm)  # BM_FORM_TABLE: reduce_once of the lazy product itself
            reduce_once_ok(mul_lz(v, canonical, "wire / mont_flag " + nm), "wire / mont_flag " + nm)  # Fp::mul with the raw 1 or TO64
    else:
        # Edwards-BLS12: canonical coordinates in, the canonical Fq::mul = reduce_once(mul_lz) throughout
        def mul(a, b, name):
            reduce_once_ok(mul_lz(a, b, "ed " + name), "ed " + name)
            return canonical

        c = mul(mul(canonical, ops["Z"], "up c0*Z"), ops["Z"], "up c*Z")
        root = mul(mul(c, c, "trees"), canonical, "inverse a*1")
        inv = mul(mul(root, c, "trees down"), c, "unfold")
        zi = mul(inv, c, "zi")
        mul(inv, ops["Z"], "inv*Z")
        x, y = mul(ops["X"], zi, "x"), mul(ops["Y"], zi, "y")
        mul(x, canonical, "from_mont")
        mul(mul(x, y, "make_base x*y"), canonical, "make_base 2d")


def main():
    use_field("Fq")  # Edwards-BLS12 buckets (EdDev): same law over the 9-limb field
    te_formulas(shapes()["canonical"])
    normalisation_formulas()
    use_field("Fp")
    canonical = shapes()["canonical"]
    X1 = shapes()["stored_x"]
    Y1, ZZ1, ZZZ1 = m1("Y1"), m1("ZZ1"), m1("ZZZ1")

    # ---- madd_lz ----
    u2 = mul_lz(canonical, ZZ1, "madd U2")
    qy = kp_sub("KP2", 2, canonical, "madd -qy")  # negated base y (lazy); the plain one is canonical
    s2 = mul_lz(qy, ZZZ1, "madd S2")
    x3, y3, pp, ppp, *_ = point_formula(X1, Y1, ZZ1, ZZZ1, u2, s2, 6, "KP6", 7, "madd")
    mul_lz(ZZ1, pp, "madd ZZ3")
    mul_lz(ZZZ1, ppp, "madd ZZZ3")

    # ---- add_lz (thread) ----
    X2 = shapes()["stored_x"]
    u1 = mul_lz(X1, ZZ1, "add U1")
    u2 = mul_lz(X2, ZZ1, "add U2")
    s1 = mul_lz(Y1, ZZZ1, "add S1")
    s2 = mul_lz(Y1, ZZZ1, "add S2")
    x3, y3, pp, ppp, r, d, qq = point_formula(u1, s1, ZZ1, ZZZ1, u2, s2, 2, "KP2", 3, "add")
    mul_lz(mul_lz(ZZ1, ZZ1, "add ZZ1ZZ2"), pp, "add ZZ3")
    mul_lz(mul_lz(ZZZ1, ZZZ1, "add ZZZ1ZZZ2"), ppp, "add ZZZ3")

    # ---- g1_add_quad: round 2 squares P and R through mul_lz, round 4 forms Y3 from two separate products ----
    mul_lz(r, r, "quad RR")
    a = mul_lz(r, d, "quad R*D")
    b = mul_lz(s1, ppp, "quad S1*PPP")
    y = norm(add_kp_sub(a, "KP2", 2, b, "quad Y3"), "quad Y3")
    canon_ok(y, "quad canon(Y3)")

    te_formulas(canonical)
    conversion_formulas()
    normalisation_formulas()

    # canonical operations on stored (lazy) coordinates: mul() = reduce_once(mul_lz()) needs mul_lz < 2p
    mul_lz(X1, canonical, "gather X*TO64")
    print("lazy bounds OK")


if __name__ == "__main__":
    main()
