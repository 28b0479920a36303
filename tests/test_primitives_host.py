"""The lazy field and curve primitives of csrc/field29.hpp, te377.hpp and g1_xyzz.hpp at the bounds of their operand
contracts, on RAW limbs, compiled for the host and checked against Python integers.  CPU only.

tests/lazy_model.py holds the contract, the operand generator and the case tables; tests/test_primitives_gpu.py runs the
same tables through the gfx950 build.  tests/PRIMITIVES.md lists function -> test and seeded fault -> catching test.
"""
import os
import subprocess

import numpy as np
import pytest

import lazy_model as M
import pyref as R
import util

FIELDS = ("Fp", "Fq")


@pytest.fixture(scope="module")
def host():
    return M.host_backend()


@pytest.fixture(scope="module", params=FIELDS)
def fm(request):
    return M.FieldModel(request.param)


def test_shape_table_is_the_proofs():
    """The shapes the generator draws from ARE tools/check_lazy_bounds.py's: same limb maxima, same value bounds, and
    they say what field29.hpp's comments say.  If the proof's table moves, the operands move with it; if someone
    retypes a bound here, this fails."""
    B = M.B
    for name in FIELDS:
        fm = M.FieldModel(name)
        B.use_field(name)
        table = B.shapes()
        assert set(table) == set(fm.shapes)
        for k, v in table.items():
            assert fm.shapes[k].hi == v.hi, (name, k)
            if k != "canonical":  # the model keeps the value bound strict for canonical operands: the box shrinks by one top-limb unit
                assert fm.shapes[k].box == v.limbs, (name, k)
        e = fm.E
        assert table["canonical"].hi == fm.P and table["stored"].hi == fm.P + e
        assert e == ((1 << 354) if name == "Fp" else fm.P // 16)
        assert fm.R == 1 << (29 * fm.RS) and fm.RS == (14 if name == "Fp" else 9)
        if name == "Fp":
            assert table["stored_x"].hi == 5 * fm.P + e
            assert table["stored"].limbs == [M.MASK] * 12 + [fm.MOD[12] + 64]  # "top limb <= MOD[N-1] + 64"
            assert table["lazy"].limbs == [3 * M.BETA - 1] * 12 + [(1 << 31) - 1]
            assert table["wide"].limbs[-1] == int(2 ** 31.6) - 1 and table["narrow"].limbs[-1] == int(2 ** 29.1) - 1
    # the proof itself still runs from that table
    subprocess.check_call(["python3", os.path.join(util.ROOT, "tools", "check_lazy_bounds.py")], stdout=subprocess.DEVNULL)


def test_normalisation_replay_and_the_gpu_tests_operands():
    """tools/check_lazy_bounds.py normalisation_formulas() -- the interval replay of k_bm_up / k_bm_across / k_bm_down and
    the k_edbm_* three -- runs for both fields, and the corner operands tests/test_normalise_gpu.py writes into the stash
    ARE the boxes that replay starts from: same table, same limb maxima, same value bounds."""
    import normalise_model as NM

    B = M.B
    for name in FIELDS:
        B.use_field(name)
        B.normalisation_formulas()
        fm = M.FieldModel(name)
        table = B.shapes()
        ops = B.NORMALISATION_OPERANDS[name]
        got = NM.stash_shapes(fm)
        assert [c for c, _ in got] == list(ops) == (["X", "Y", "ZZ", "ZZZ"] if name == "Fp" else ["X", "Y", "T", "Z"])
        for c, sh in got:
            assert sh.hi == table[ops[c]].hi, (name, c)
            if ops[c] != "canonical":
                assert sh.box == table[ops[c]].limbs, (name, c)
    assert B.NORMALISATION_OPERANDS["Fp"] == {"X": "stored_x", "Y": "stored", "ZZ": "stored", "ZZZ": "stored"}
    fm = M.FieldModel("Fp")
    B.use_field("Fp")
    corners = dict(NM.g1_corner_rows(fm))
    assert corners["all corners"] == B.shapes()["stored_x"].limbs + 3 * B.shapes()["stored"].limbs
    assert corners["all value maxima"] == [x for h in (5 * fm.P + fm.E, fm.P + fm.E, fm.P + fm.E, fm.P + fm.E) for x in M.nform_limbs(h - 1, 13)]
    for c, name in enumerate(("X", "Y", "ZZ", "ZZZ")):
        assert corners[name + " corner"][13 * c : 13 * c + 13] == B.shapes()[ops_name(name)].limbs
    # the steered residues cover both arms of both walks
    for name in FIELDS:
        f = M.FieldModel(name)
        ks = [M.kaliski_k(f, a) for _, a in NM.steered_values(f)]
        cut = M.INVERSE_WALK[name]["short_below"]
        assert sum(k < cut for k in ks) >= 3 and sum(k >= cut for k in ks) >= 3, (name, ks)


def ops_name(coordinate):
    return M.B.NORMALISATION_OPERANDS["Fp"][coordinate]


def test_generator_emits_only_in_contract_vectors(fm):
    """Every shape: its fixed edge set plus at least 2 000 random vectors, all inside the shape (asserted by the generator
    itself, never filtered), deterministic, and the corner of the box really is there."""
    for name, shape in fm.shapes.items():
        v = fm.vectors(name, 1)
        assert v == fm.vectors(name, 1) and v != fm.vectors(name, 2)
        assert len(v) >= 4 + fm.N + 1 + 2000
        assert v[0] == shape.box and v[1] == [0] * fm.N
        assert all(shape.holds(x) for x in v)
        assert not shape.holds([shape.box[0] + 1] + shape.box[1:])
    assert fm.is_lazy(fm.shapes["lazy"].box) and not fm.is_lazy([3 * M.BETA] + [0] * (fm.N - 1))
    assert fm.is_nform(M.nform_limbs(fm.P + fm.E - 1, fm.N), fm.P + fm.E) and not fm.is_nform(M.nform_limbs(fm.P + fm.E, fm.N), fm.P + fm.E)
    assert not fm.is_nform([M.BETA] + [0] * (fm.N - 1), fm.P)


def test_model_group_law_is_pyrefs():
    """The Edwards law the curve cases expect results from is pyref's group law: Edwards-BLS12 directly, Te377's curve
    through the birational map to y^2 = x^3 + 1."""
    cq = M.CurveModel(M.FieldModel("Fq"))
    for a in cq.points:
        for b in cq.points:
            assert cq.add(a, b) == R.ed_add(a, b)
    cp = M.CurveModel(M.FieldModel("Fp"))
    ks = (1, 2, 3, 5, 12345, R.R_ORDER - 7)
    for i, a in enumerate(cp.points):
        for j, b in enumerate(cp.points):
            s = cp.add(a, b)
            words = [x for v in cp.ext_values(s, 7) for x in M.nform_limbs(v, 13)]
            assert util.affine_from_te_ext_words(words) == R.add(R.mul(R.G, ks[i]), R.mul(R.G, ks[j]))


def test_field_ops_at_their_bounds(host, fm):
    """mul_lz, sqr_lz, mul_add_mul_lz, mul, sqr, mul_sub_mul, add, sub, neg, reduce_once, norm, csub (MOD, MOD2, MOD4), canon,
    add_kp_sub (KP2, KP6), add_kp_sub_sub2 (KP4W3), kp_sub, add_lz -- for Fp and Fq, on every operand-shape pair the
    comments allow, against Python integers: residue, bounds and carry-normalisation for the products, the exact value
    and every unmasked limb for the limb-wise forms, THE canonical residue for the canonical ones."""
    seen = set()
    for op, label, ins in M.field_cases(fm):
        M.check_field_case(fm, op, label, ins, host.field(fm, op, ins))
        seen.add(op)
    assert seen == set(M.FIELD_OPS)


def test_edwards_formulas_on_real_points_in_edge_representations(host, fm):
    """Te377 / EdLazy madd, madd_affine, add: one coordinate of the accumulator steered to 1, p - 1, all-low-limbs-max,
    values below the slack e (stored as v and as v + p), for X, Y, T, Z in turn, both signs, P = Q, P = -Q, identity
    accumulators (0, c, 0, c) and identity().  Result: pyref's group law, projectively; storage invariant; no flag."""
    cm = M.CurveModel(fm)
    cases = M.te_point_cases(cm)
    for op, case in cases.items():
        out, flags = host.te(fm, op, case[0], case[1], case[2])
        M.check_te_point_case(cm, op, case, out, flags)
        assert len(case[3]) > 100


def test_edwards_formulas_as_polynomial_maps(host, fm):
    """finish, madd, madd_affine, add on in-contract quadruples that are no curve points -- all four coordinates of every
    operand at the corner of the stored box at once -- against the hwcd-3 polynomials, up to one common factor."""
    cm = M.CurveModel(fm)
    for name, case in M.te_poly_cases(cm).items():
        out, _ = host.te(fm, name.split()[0], case[0], case[1], case[2])
        M.check_te_poly_case(cm, name, case, out)


def test_first_entry_of_a_chain(host):
    """Te377::from_base / from_base_affine: the canonical Ext of (+-) the record's point."""
    fm = M.FieldModel("Fp")
    cm = M.CurveModel(fm)
    for op, (rows, negs, exps) in M.te_from_base_cases(cm).items():
        out, flags = host.te(fm, op, np.zeros_like(rows), rows, negs)
        for i, o in enumerate(out.tolist()):
            cm.check_ext(o, exps[i], (op, i))
            assert all(M.value(o[13 * c : 13 * c + 13]) < fm.P for c in range(4)), "canonical coordinates"
        assert not flags.any()


def test_zero_mod_p_is_recognised_in_both_stored_forms(host, fm):
    """is_zero_mod_p / is_bad: all-zero limbs AND exactly p flag; p + 1, p - 1, 1 do not."""
    rows, exp = M.te_zero_cases(fm)
    _, flags = host.te(fm, "is_zero", rows, np.zeros_like(rows), np.zeros(len(rows), dtype=np.uint32))
    assert flags.tolist() == exp


def test_xyzz_formulas_on_real_points_in_edge_representations(host):
    """G1::madd_lz / add_lz on raw XYZZ limbs: X stored as x + k p up to 5p + e, each of X, Y, ZZ, ZZZ steered to edge values, P = Q,
    P = -Q, identity accumulators; the false-positive side of both guards (add_lz: low limb of P in 1..3, madd_lz: 1..7, P != 0
    mod p); canon_pt."""
    fm = M.FieldModel("Fp")
    cases = M.g1_point_cases(fm)
    for op, case in cases.items():
        out = host.g1(op, case[0], case[1], case[2])
        for i, o in enumerate(out.tolist()):
            M.check_g1_words(fm, o, case[3][i], (op, case[4][i]))
        assert len(case[3]) > 100
    zero = lambda n: np.zeros(n, dtype=np.uint32)  # noqa: E731
    for op, (a, b, exps, lows) in M.guard_false_positive_cases(fm).items():
        assert len(lows) >= 3
        M.check_guard_cases(host, fm, op, a, b, lows)  # from the real mul_lz outputs: the guard IS hit, P != 0 mod p
        out = host.g1(op, a, b, zero(len(a)))
        for i, o in enumerate(out.tolist()):
            M.check_g1_words(fm, o, exps[i], (op, "guard false positive, low limb", lows[i]))
    # canon_pt: every coordinate to THE canonical residue
    pts = cases["add_lz"][0]
    out = host.g1("canon_pt", pts, np.zeros_like(pts), np.zeros(len(pts), dtype=np.uint32))
    for i, (o, a) in enumerate(zip(out.tolist(), pts.tolist())):
        for c in range(4):
            assert o[13 * c : 13 * c + 13] == M.nform_limbs(M.value(a[13 * c : 13 * c + 13]) % fm.P, 13), i


def test_inversion_walk_cases_cover_both_arms(fm):
    """FpInverse / FqInverse::inverse_mont, from the k-model ALONE (nothing native runs here): the case list of
    field_cases holds at least 8 inputs in the two-factor arm of the conversion (Fp: k < 436, Fq: k < 270, read from the
    headers' j1 > 376 / j1 > 252) and 8 in the other, the edge list, 256 random residues, and the smallest and the
    largest k among 10^5 seeded random residues -- which the pinned file names and this test finds again."""
    import json

    walk = M.INVERSE_WALK[fm.name]
    hdr = open(os.path.join(M.CSRC, "fp_inverse.hpp" if fm.name == "Fp" else "fq_inverse.hpp")).read()
    total, cut = (812, 376) if fm.name == "Fp" else (522, 252)
    assert "int j1 = %d - k" % total in hdr and "if (j1 > %d)" % cut in hdr and "k < 2 * %d" % (walk["cap"] // 2) in hdr
    assert walk["short_below"] == total - cut and total == 2 * 29 * fm.RS
    cases = M.inverse_cases(fm)
    ks = [k for _, k, _ in cases]
    short, long_ = [k for k in ks if k < walk["short_below"]], [k for k in ks if k >= walk["short_below"]]
    print("%s inverse_mont: %d cases, %d in the short-k arm, %d in the other, k in [%d, %d]" % (fm.name, len(cases), len(short), len(long_), min(ks), max(ks)))
    assert len(short) >= 8 and len(long_) >= 8
    assert sum(1 for _, _, l in cases if l.startswith("random")) == M.INVERSE_RANDOM == 256
    assert sum(1 for _, _, l in cases if l.endswith("+ p")) >= 4  # non-canonical representatives
    bits = fm.P.bit_length()
    assert all(bits <= k <= 2 * bits for k in ks)  # Kaliski's range; the cap of the loop is never what ends a walk
    for a, k, label in cases:
        assert M.kaliski_k(fm, a) == k == M.kaliski_k_fast(fm, a), label
        assert M.value(M.nform_limbs(a, fm.N)) == a and a % fm.P
    lo, hi = M.inverse_scan(fm)
    with open(M.INVERSE_EXTREMES) as f:
        pinned = json.load(f)[fm.name]
    assert pinned == {"scanned": M.INVERSE_SCAN, "min": list(lo), "max": list(hi)} and M.INVERSE_SCAN == 100000
    assert lo[1] in ks and hi[1] in ks and lo[1] >= walk["short_below"]  # a random residue does not reach the short arm: the edges do


def test_strict_g1_doublings(host):
    """G1::dbl on every stored representation (X = x + k p up to the box, Y, ZZ, ZZZ with + p where the box allows), the
    2-torsion points with Y = 0 and Y = p -> ZZ limb-zero, outputs inside the stored boxes; G1::dbl_affine."""
    fm = M.FieldModel("Fp")
    rows, exps, labels = M.g1_dbl_cases(fm)
    zero = np.zeros(len(rows), dtype=np.uint32)
    M.check_g1_doubles(fm, host.g1("dbl", rows, np.zeros_like(rows), zero), exps, labels, "dbl")
    assert sum(1 for l in labels if "Y = p" in l) >= 15 and sum(1 for l in labels if "+ 5 p" in l) >= 3 and len(rows) > 100
    for c in ("Y", "ZZ", "ZZZ"):
        assert sum(1 for l in labels if l.startswith(c + " ->") and l.endswith("+ 1 p")) == 3
    rows, exps, labels = M.g1_dbl_affine_cases(fm)
    zero = np.zeros(len(rows), dtype=np.uint32)
    M.check_g1_doubles(fm, host.g1("dbl_affine", np.zeros_like(rows), rows, zero), exps, labels, "dbl_affine")
    assert exps.count(None) == 3


def test_strict_edwards_formulas(host):
    """EdT<Fq, EdK29> madd, add, dbl, dbl_nt, make_base, cneg against pyref's group law on real points."""
    cm = M.CurveModel(M.FieldModel("Fq"))
    cases = M.ed_strict_cases(cm)
    assert set(cases) == set(M.ED_OPS)
    for op, case in cases.items():
        assert len(case[3]) >= (8 if op == "make_base" else 16), op  # make_base: six points, the identity, the point of order 2
        M.check_ed_strict_case(cm, op, case, host.ed(op, case[0], case[1], case[2]))


def test_device_test_library_is_built_for_gfx950_and_kept_apart():
    """The default make target builds libmsm377_primtest.so next to the product library, with a gfx950 code object and the
    launchers the GPU test calls -- and nothing of it leaks into libmsm377.so."""
    csrc = M.CSRC
    subprocess.check_call(["make", "-C", csrc, "ARCH=gfx950"], stdout=subprocess.DEVNULL)
    assert os.path.exists(M.PRIMTEST_SO)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.PRIMTEST_SO], text=True)
    for name in M.PRIMTEST_ENTRY_POINTS:
        assert " T %s\n" % name in syms, name
    with open(M.PRIMTEST_SO, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"k_add_quad" in blob
    product = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(csrc, "libmsm377.so")], text=True)
    assert "primtest" not in product
    with open(os.path.join(csrc, "Makefile")) as f:
        mk = f.read()
    link = [l for l in mk.splitlines() if l.startswith("libmsm377.so:")]
    assert link and "primtest" not in link[0]
