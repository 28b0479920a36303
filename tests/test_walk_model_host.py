"""CPU pins of tests/walk_model.py and tests/walk_cases.py: the digit lists against the integer identity and against the
product's own recode (the stand-alone programs of tests/native/), the stash checks against rows built by hand -- each rule
of the contract must be able to fail --, and every case of tests/test_walk_stash_gpu.py against what it promises, before
anything runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import batch_mul_vectors as V
import check_vectors as CV
import lazy_model as M
import normalise_model as NM
import pyref as R
import record_model as RM
import walk_cases as WC
import walk_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "native", "_build")
r = R.R_ORDER


def all_crafted():
    out = set()
    for c in (4, 8, 16):
        out |= {s for _, s in WM.crafted_scalars(c)} | set(WC.small_order_extras(c))
    return sorted(out | set(V.EDGE) | set(V.random_scalars(0x3A1C, 16)))


def build(name):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name + "_walk")
    cmd = ["g++", "-O1", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return exe


# ---- digits ----
@pytest.mark.parametrize("c", [4, 8, 16])
def test_digits_satisfy_the_identity_and_their_range(c):
    W, half = WM.windows(c), 1 << (c - 1)
    assert W == -(-256 // c)
    for s in all_crafted():
        digits, carry = WM.signed_digits(s, c)
        assert len(digits) == W and carry in (0, 1)
        assert all(-(half - 1) <= d <= half for d in digits), hex(s)
        assert sum(d << (c * w) for w, d in enumerate(digits)) + (carry << (c * W)) == s, hex(s)
    assert WM.signed_digits(half, c)[0][0] == half and WM.signed_digits(half + 1, c)[0][:2] == [-(half - 1), 1]
    assert WM.signed_digits(2**256 - 1, c) == ([-1] + [0] * (W - 1), 1)  # the carry through every window into row W
    assert WM.var_digits(8)[0][0] == 8 and min(min(WM.var_digits(s)[0]) for s in all_crafted()) == -7


@pytest.mark.parametrize("c", [8, 16])
def test_digits_against_the_products_recode(c):
    exe = build("batch_mul_host")
    scalars = all_crafted()
    res = subprocess.run([exe, "recode", str(c)] + ["%x" % s for s in scalars], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(scalars)
    for s, line in zip(scalars, lines):
        got = [int(x) for x in line.split()]
        digits, carry = WM.signed_digits(s, c)
        assert got == digits + [carry], hex(s)


def test_var_digits_against_the_products_packing():
    exe = build("batch_mul_var_host")
    scalars = all_crafted()
    res = subprocess.run([exe, "pack"] + ["%x" % s for s in scalars], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    for s, line in zip(scalars, res.stdout.strip().split("\n")):
        walked = [int(x) for x in line.split("|")[0].split()]
        digits, carry = WM.var_digits(s)
        assert walked == digits[::-1] + [carry], hex(s)  # the walk hands them out from window 63 down


# ---- the stash contract: every rule can fail ----
def g1_row(pt, z=1):
    """XYZZ words of pt under ZZ = z^2, ZZZ = z^3 (canonical Montgomery limbs)."""
    if pt is None:
        return WM.g1_identity_words()
    p = R.P
    return sum((RM.fp_limbs(v) for v in (pt[0] * z * z % p, pt[1] * z * z * z % p, z * z % p, z * z * z % p)), [])


def test_g1_stash_check_decodes_and_refuses():
    fp = WM.field("Fp")
    p = R.P
    pts = [R.G, None, R.mul(R.G, 77), (0, 1), (R.P - 1, 0)]
    rows = [g1_row(pt, 3 + 5 * i) for i, pt in enumerate(pts)]
    assert WM.check_g1_stash(rows) == pts
    assert WM.g1_identity_words() == NM._row(fp, [0, fp.R % p, 0, 0])

    def refused(row, text):
        with pytest.raises(AssertionError) as e:
            WM.check_g1_stash([rows[0], row])
        assert text in str(e.value) and "stash point 1" in str(e.value), str(e.value)

    live = rows[2]
    limbs_p = M.nform_limbs(p, 13)
    refused(live[:26] + limbs_p + limbs_p, "not G1::identity()")          # ZZ = ZZZ = 0 mod p as the limbs of p
    refused(live[:39] + [0] * 13, "not G1::identity()")                   # ZZZ limb-zero beside a live ZZ
    refused(live[:26] + [0] * 26, "not G1::identity()")                   # an identity with X, Y left over: not tidied
    refused(live[:26] + RM.fp_limbs(4) + live[39:], "ZZ^3 != ZZZ^2")
    refused(RM.fp_limbs(5) + live[13:], "not on the curve")
    y_plus_p = M.nform_limbs(M.value(live[13:26]) + p, 13)
    if M.value(y_plus_p) >= fp.shapes["stored"].hi:
        refused(live[:13] + y_plus_p + live[26:], "Y outside the stored box")
    refused(live[:13] + M.nform_limbs(M.value(live[13:26]) + 2 * p, 13) + live[26:], "Y outside the stored box")
    x5 = M.nform_limbs(M.value(live[:13]) % p + 4 * p, 13)                # X may be lazy up to 5p + e
    assert WM.check_g1_stash([live[:0] + x5 + live[13:]]) == [pts[2]]
    refused(M.nform_limbs(M.value(live[:13]) % p + 6 * p, 13) + live[13:], "X outside the stored_x box")
    loose = list(live)
    loose[0] += 1 << 29                                                   # a limb that is not carry-normalised
    loose[1] -= 1
    if loose[1] >= 0:
        refused(loose, "X outside the stored_x box")


def test_ed_stash_check_decodes_and_refuses():
    q = R.Q
    pts = [R.ED_G, R.ED_ID, R.ed_mul(R.ED_G, 5), (0, q - 1)]

    def row(pt, z):
        x, y = pt
        return sum((RM.fq_limbs(v) for v in (x * z % q, y * z % q, x * y * z % q, z)), [])

    rows = [row(pt, 7 + i) for i, pt in enumerate(pts)]
    assert WM.check_ed_stash(rows) == pts
    top = WM.check_ed_stash([row(R.ED_G, q - 1)])  # a coordinate whose top limb is the modulus's own
    assert top == [R.ED_G]

    def refused(bad, text):
        with pytest.raises(AssertionError) as e:
            WM.check_ed_stash([rows[0], bad])
        assert text in str(e.value), str(e.value)

    live = rows[2]
    refused(live[:27] + [0] * 9, "Z = 0")
    refused(live[:18] + RM.fq_limbs(3) + live[27:], "T Z != X Y")
    zq = M.nform_limbs(M.value(live[27:]) + q, 9)
    refused(live[:27] + zq, "Z outside the canonical box")                # Fq::norm in place of Fq::canon: below 2 q, not below q


def test_running_products_check():
    fp = WM.field("Fp")
    n = 1025 + 300
    rows = np.array(NM.with_identities(fp, NM.tile(NM.random_rows(fp, 64, 5), n), [3, 259, 1024]), dtype=np.uint32)
    prod = np.zeros((n, 16), dtype=np.uint32)
    one = WM.one_limbs("Fp")
    for i in range(n):
        if (i % 1024) // 256 == 0:
            prod[i, :13] = one
        else:
            z = rows[i - 256, 39:].tolist()
            zv = M.value(z) if any(z) else fp.R
            prod[i, :13] = M.nform_limbs(M.value(prod[i - 256, :13].tolist()) * zv * fp.Rinv % fp.P, 13)
    WM.check_products("Fp", rows, prod)
    for i, word, text in ((700, 0, "not C z / R"), (5, 0, "not one()"), (1024, 1, "not one()"), (900, 14, "pad words")):
        bad = prod.copy()
        bad[i, word] ^= 1
        with pytest.raises(AssertionError) as e:
            WM.check_products("Fp", rows, bad)
        assert text in str(e.value) and "stash point %d" % i in str(e.value), str(e.value)
    inclusive = prod.copy()  # the inclusive product in place of the exclusive one
    for i in range(n):
        z = rows[i, 39:].tolist()
        inclusive[i, :13] = M.nform_limbs(M.value(prod[i, :13].tolist()) * (M.value(z) if any(z) else fp.R) * fp.Rinv % fp.P, 13)
    with pytest.raises(AssertionError):
        WM.check_products("Fp", rows, inclusive)


def test_table_entries():
    named = dict(V.bases())
    pts = [R.G, named["small_0"], named["small_3"], named["small_5"], None, named["G_plus_torsion"]]
    words = np.array([[WM.entry_words(pt, e) for pt in pts] for e in range(1, 9)], dtype=np.uint32)
    WM.check_table(words, pts)
    assert words[1, 1].tolist() == [0] * 26 + [1] + [0] * 5 and words[0, 1, 26] == 0     # [2]T = O, flag 1; [1]T live
    assert all(words[e, 4, 26] == 1 and not words[e, 4, :26].any() for e in range(8))    # a flagged input: all eight
    assert words[2, 2, 26] == 1 and words[3, 3, 26] == 1                                   # [3] of order 3, [4] of order 4
    assert words[4, 0].tolist() == RM.table_record_words(R.mul(R.G, 5))
    bad = words.copy()
    bad[5, 0] = words[4, 0]  # entry 6 from one addition too few
    with pytest.raises(AssertionError) as e:
        WM.check_table(bad, pts)
    assert "entry [6]P of point 0" in str(e.value)


# ---- the cases: every promise, from the model alone ----
def case_ids(cases):
    return ["%s/%s" % (c["call"], c["name"]) for c in cases]


@pytest.mark.parametrize("case", WC.all_cases(), ids=case_ids(WC.all_cases()))
def test_case_promises(case):
    assert len(case["rows"]) == case["n"] and case["crafted"] and max(case["crafted"]) < case["n"]
    got = WC.events_of(case)
    assert case["promises"] <= got, (sorted(case["promises"] - got), sorted(got))
    for i in case["crafted"][:3]:
        WC.expected_point(case, i)  # (lane_events asserts the digit walk against the direct sum)


@pytest.mark.parametrize("cases", [WC.batch_mul_cases, WC.multi_cases, WC.commit_cases, WC.var_cases, WC.lincomb2_cases], ids=lambda f: f.__name__)
def test_every_g1_walk_meets_every_event_between_its_cases(cases):
    seen = set()
    for case in cases():
        seen |= WC.events_of(case)
        assert case["promises"] <= WC.events_of(case)
    promised = set().union(*(case["promises"] for case in cases()))
    need = WC.ALL_G1_EVENTS - ({WM.EV_ZERO_O, WM.EV_SMALL_O, WM.EV_MID_O} if cases is WC.commit_cases else set())
    assert need <= promised, sorted(need - promised)  # (promised, not merely seen: the GPU test repeats each promise)
    assert promised <= seen


def test_sizes_and_placements():
    assert WC.SIZES == (1, 64, 65, 255, 257, 1025, 3079)
    for cases in (WC.batch_mul_cases, WC.multi_cases, WC.var_cases, WC.lincomb2_cases, WC.ed_cases):  # (the row commitments: rows 1, 255, 300, below)
        assert set(WC.SIZES) <= {c["n"] for c in cases() if c["placed"]}, cases.__name__
    assert set(WC.SIZES) <= {c["n"] for c in WC.multi_cases() if len(c["bases"]) == 2 and c["c"] == 8} and set(WC.SIZES) <= {c["n"] for c in WC.multi_cases() if c["c"] == 16}
    unplaced = sorted(c["name"] for c in WC.all_cases() if not c["placed"])
    assert unplaced == ["a-stride0", "a=b=1", "b-stride0", "k16-all-ones-c16", "k16-all-ones-c8", "relations-k48", "stride0-64bit", "stride0-carry"], unplaced
    for case in WC.all_cases():
        n = case["n"]
        if case["placed"]:
            assert {i for i in (0, 63, 64, 255, 256, n - 1) if i < n} <= set(case["crafted"]), case["name"]
        if case["placed"] and n >= 255:
            assert not any(any(case["rows"][i]) for i in range(128, 192)), case["name"]  # a whole wave of zero scalars
            assert any(case["rows"][64]) and not any(any(case["rows"][i]) for i in range(65, 128)), case["name"]  # beside a wave with one non-zero lane
    assert {len(c["bases"]) for c in WC.commit_cases()} >= {16, 17, 33, 257} and {c["n"] for c in WC.commit_cases()} >= {1, 255, 300}
    assert {len(c["bases"]) for c in WC.multi_cases()} == {2, 16} and {c["layout"] for c in WC.multi_cases()} == {"rows", "columns"}
    assert {(len(c["bases"]), c["c"]) for c in WC.ed_cases()} >= {(k, c) for k in (1, 2, 16) for c in (8, 16)}


def test_the_fold_meets_its_cases():
    rel = [c for c in WC.commit_cases() if c["name"] == "relations-k48"][0]
    assert set(WC.FOLD_EVENTS) <= WC.fold_events(rel)
    assert CR_plan_matches()


def CR_plan_matches():
    import commit_rows_vectors as CR

    return WC.segments_of(16) == [(0, 16)] and WC.segments_of(17) == [(0, 9), (9, 17)] and len(WC.segments_of(257)) == 17 and CR.plan(33)[:2] == (3, 11)
