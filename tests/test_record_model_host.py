"""CPU pins of tests/record_model.py, the model tests/test_base_records_gpu.py compares the GPU's base records and window
tables with.  Nothing here runs product code: the model is held against pyref's group laws, against the bucket decode the
stage tests already use, and against the proof's shape table."""
import contextlib
import random

import numpy as np
import pytest

import check_vectors as CV
import pyref as R
import record_model as RM
import stage_model as M
import util


@contextlib.contextmanager
def pyref_edwards_over_fp():
    """pyref.ed_add is the a = -1 twisted Edwards law over pyref's module constants; with the modulus and d of the G1 model
    (csrc/te377.hpp) in their place it is the law the records of G1 are added by."""
    saved = (R.Q, R.ED_A, R.ED_D)
    R.Q, R.ED_A, R.ED_D = R.P, R.P - 1, util.te_params()["d"]
    try:
        yield
    finally:
        R.Q, R.ED_A, R.ED_D = saved


def subgroup_points(count, seed):
    return [R.mul(R.G, k) for k in R.rand_scalars(seed, count)]


def odd_order_points():
    """Points the Edwards map represents beyond the subgroup: order 3 (x = 0), a cofactor-torsion point of large odd
    order when there is one, and subgroup + torsion sums."""
    import batch_mul_vectors as V

    return [pt for _, pt in V.bases() if RM.te_representable(pt)]


def test_constants():
    te = util.te_params()
    assert 3 * te["s"] * te["s"] % R.P == 1, "s = 1 / sqrt(3)"
    assert RM.RADIX_FP == util.R29 and RM.RADIX_FQ == 1 << 261
    fq = M.fq_model()
    assert RM.RADIX_FQ * fq.Rinv % R.Q == 1 and fq.P == R.Q and fq.N == 9
    b = RM.beta()
    assert b != 1 and pow(b, 3, R.P) == 1
    lam, _ = M.glv_consts()
    for pt in subgroup_points(3, 0xBE7A):
        assert (b * pt[0] % R.P, pt[1]) == R.mul(pt, lam), "phi(P) = (BETA x, y) = [LAMBDA] P"
    assert RM.fp_limbs(5) == util.to_limbs29_mont(5)
    for form in RM.RECORD_WORDS:
        assert RM.LIMBS[form] * RM.COORDS[form] <= RM.RECORD_WORDS[form] and len(RM.COORD_NAMES[form]) == RM.COORDS[form]


def test_map_lands_on_the_curve_and_inverts():
    d = util.te_params()["d"]
    for pt in subgroup_points(6, 0x3A9) + odd_order_points():
        xe, ye = RM.te_affine(pt)
        assert (-xe * xe + ye * ye - 1 - d * xe * xe * ye * ye) % R.P == 0
        assert RM.te_to_weierstrass((xe, ye)) == pt
        X, Y, T, Z = RM.te_projective(pt)
        assert (X * Y - T * Z) % R.P == 0 and X * pow(Z, -1, R.P) % R.P == xe and Y * pow(Z, -1, R.P) % R.P == ye
    assert RM.te_affine(None) == (0, 1)
    for t in CV.g1_small_order_points():
        order = next(k for k in (2, 3, 4, 6) if R.mul(t, k) is None)
        if order != 6:  # the map is undefined exactly at the points of order 2 and 4
            assert RM.te_representable(t) == (order == 3), (t, order)
    assert not RM.te_representable((R.P - 1, 0)) and not RM.te_representable(util.t_prime())
    assert RM.te_affine((0, 1))[0] != 0 and RM.te_representable((0, R.P - 1))


def test_map_is_a_homomorphism():
    """map(P + Q) = ed_add(map P, map Q) on a dozen pairs, the sums by R.add: distinct points, a doubling, opposite
    points, the identity on either side, points of order 3, points outside the subgroup."""
    ps = subgroup_points(6, 0x40)
    odd = odd_order_points()
    pairs = [(ps[0], ps[1]), (ps[2], ps[3]), (ps[4], ps[5]), (ps[0], ps[0]), (ps[1], R.neg(ps[1])), (None, ps[2]), (ps[3], None), (None, None),
             ((0, 1), (0, 1)), ((0, 1), (0, R.P - 1)), ((0, 1), ps[4]), (odd[-1], ps[5]), (odd[-1], odd[-1]), (odd[-2], odd[-1])]
    assert len(pairs) >= 12
    with pyref_edwards_over_fp():
        for p, q in pairs:
            s = R.add(p, q)
            if not (s is None or RM.te_representable(s)):
                continue
            assert RM.te_affine(s) == R.ed_add(RM.te_affine(p), RM.te_affine(q)), (p, q)
            assert RM.te_add(RM.te_affine(p), RM.te_affine(q)) == RM.te_affine(s)


def ext_words_of_single_entry(form, pt):
    """The bucket a single-entry row holds (te377.hpp from_base / from_base_affine): (2X : 2Y : 2T : 2Z) from the record's
    Y - X, Y + X, 2d T and 2 Z (2 for an affine record), as 52 device words."""
    d = util.te_params()["d"]
    rec = RM.record_words(form, pt)
    ri = pow(RM.RADIX_FP, -1, R.P)
    vals = [(v.value if isinstance(v, RM.Lazy) else RM.value_of(v)) * ri % R.P for v in rec]
    ymx, ypx, kt = vals[:3]
    z2 = vals[3] if form == RM.FORM_TE_PROJECTIVE else 2
    ext = [(ypx - ymx) % R.P, (ypx + ymx) % R.P, kt * pow(d, -1, R.P) % R.P, z2]
    return [w for v in ext for w in RM.fp_limbs(v)]


@pytest.mark.parametrize("form", [RM.FORM_TE_PROJECTIVE, RM.FORM_TE_AFFINE])
def test_records_agree_with_the_bucket_decode_of_the_stage_tests(form):
    for pt in subgroup_points(5, 0xDEC0) + odd_order_points():
        assert util.affine_from_te_ext_words(ext_words_of_single_entry(form, pt)) == pt


def test_edwards_bls12_base_record():
    fq = M.fq_model()
    import ed_curve_points as E

    pts = E.every_curve_point(40)[0]
    for pt in pts:
        ymx, ypx, kt = (RM.value_of(v) * fq.Rinv % R.Q for v in RM.ed_make_base(pt))
        x, y = (ypx - ymx) * pow(2, -1, R.Q) % R.Q, (ypx + ymx) * pow(2, -1, R.Q) % R.Q
        assert (x, y) == pt and kt == 2 * R.ED_D * x * y % R.Q
        # the record feeds the lazy law: identity + record must decode to the point (stage tests' decode)
        words = [w for v in (2 * x, 2 * y, kt * pow(R.ED_D, -1, R.Q), 2) for w in RM.fq_limbs(v)]
        assert M.ed_record_affine(words) == pt


@pytest.mark.parametrize("widths", [RM.WINDOWS16, RM.WIDE_WIDTHS], ids=["c16", "c20"])
def test_table_windows_are_the_multiples(widths):
    assert len(widths) in (16, 13)
    offs = RM.window_offsets(widths)
    if widths is RM.WIDE_WIDTHS:
        assert offs == [M.wide_offset(w) for w in range(13)] and offs[-1] == 234 and widths == (20,) * 6 + (19,) * 7
    else:
        assert offs == [16 * w for w in range(16)]
    for pt in subgroup_points(2, 0x71D) + [(0, 1)]:
        wp = RM.window_points(pt, widths)
        assert len(wp) == len(widths)
        for w, q in enumerate(wp):
            assert q == R.mul(pt, 1 << offs[w]), w
            assert RM.te_affine_words(q)[:2] == [RM.fp_limbs(RM.te_affine(q)[1] - RM.te_affine(q)[0]), RM.fp_limbs(RM.te_affine(q)[1] + RM.te_affine(q)[0])]


def small_order(order):
    return next(t for t in CV.g1_small_order_points() if R.mul(t, order) is None and all(R.mul(t, k) is not None for k in range(1, order)))


def test_batch_table_entries_are_the_multiples():
    """table_rows (additions) against table_point = R.mul(B, d << (c w)) and the identity flag, for the generator and
    bases of order 2, 3 and 4."""
    assert RM.table_records(8) == 4097 and RM.table_records(16) == 524289 and RM.table_windows(8) == 32
    rnd = random.Random("table pins")
    for name, base in (("G", R.G), ("order2", small_order(2)), ("order3", small_order(3)), ("order4", small_order(4))):
        rows = RM.table_rows(base, 8)
        assert len(rows) == 4097
        picks = [0, 1, 126, 127, 128, 129, 4095, 4096] + [rnd.randrange(4097) for _ in range(24)]
        flags = 0
        for t in picks:
            pt = RM.table_point(base, 8, t)
            assert rows[t] == pt, (name, t)
            rec = RM.table_record_words(pt)
            assert len(rec) == 32 and rec[26] == (1 if pt is None else 0) and rec[27:] == [0] * 5
            flags += rec[26]
        if name == "order2":
            assert all(p is None for p in rows[128:]) and rows[1] is None and rows[0] == base
        if name == "order3":
            assert [p is None for p in rows[:6]] == [False, False, True, False, False, True]
        if name == "order4":
            assert all(p is None for p in rows[128:]), "[2^8 w] of a point of order 4 is the identity: whole rows of flags"
            assert rows[3] is None and rows[1] == (R.P - 1, 0)
        assert (flags > 0) == (name != "G")
    for t in (0, 1, (1 << 15) - 2, (1 << 15) - 1, 1 << 15, RM.table_records(16) - 1):
        w, d = t >> 15, (t & 0x7FFF) + 1
        assert RM.table_point(R.G, 16, t) == R.mul(R.G, (d << (16 * w)) % R.R_ORDER)
        assert t == RM.table_index(16, w, d)


def test_box_predicates():
    """The boxes are the proof's (tools/check_lazy_bounds.py shapes()); each accepts its corner and the value below it,
    and rejects the first value outside, a limb above its maximum, and a coordinate with p added limb-wise."""
    rnd = random.Random("boxes")
    for field, mod, n in (("Fp", R.P, 13), ("Fq", R.Q, 9)):
        t = RM.boxes(field)
        assert t["canonical"].hi == mod and t["stored"].hi > mod
        if field == "Fp":
            assert t["stored"].hi == R.P + (1 << 354)
        modl = RM.limbs_of(mod, n)
        for name, box in t.items():
            corner = box.corner()
            assert RM.value_of(corner) == box.hi - 1
            outside = RM.limbs_of(box.hi, n)
            zero = [0] * n
            lo = RM.limbs_of(box.hi - 2, n)
            limb_over = [RM.MASK + 1] + [0] * (n - 1)  # a small value, not carry-normalised
            got = box.accepts(np.array([corner, outside, zero, lo, limb_over], dtype=np.uint32))
            assert got.tolist() == [True, False, True, True, False], (field, name, got)
            vals = [rnd.randrange(mod) for _ in range(50)] + [mod - 1, mod >> 1]
            if name == "stored":
                vals = [v for v in vals if v >= box.hi - mod]  # below that, v + p is still a value the box admits
            plain = np.array([RM.limbs_of(v, n) for v in vals], dtype=np.uint32)
            plus_p = np.array([[a + b for a, b in zip(RM.limbs_of(v, n), modl)] for v in vals], dtype=np.uint32)
            assert box.accepts(plain).all() and not box.accepts(plus_p).any(), (field, name)
    # a canonical coordinate that was stored lazily (y + x by add_lz): rejected by the canonical box whenever it matters
    a, b = RM.fp_limbs(R.G[0]), RM.fp_limbs(R.G[1])
    lz = np.array([[x + y for x, y in zip(a, b)]], dtype=np.uint32)
    assert not RM.boxes("Fp")["canonical"].accepts(lz)[0]


def test_sample_indices_cover_what_the_issue_names():
    for n, windows in ((257, 16), (2049, 13), (300, 16), (4097, 1), (2049, 1)):
        s = set(RM.sample_indices(n, windows, n, 256, "pin"))
        if n <= 2049 and windows == 1:
            assert s == set(range(n))
            continue
        for w in range(windows):
            for i in (0, 255, 256, 2047, 2048, n - 1):
                assert i >= n or w * n + i in s
        for w in (0, min(1, windows - 1), windows - 1):
            assert set(range(w * n, w * n + n)) <= s
        full = len({0, min(1, windows - 1), windows - 1}) * n
        assert len(s) >= min(windows * n, full + 256)
