"""The batch calls' normalisation kernels -- k_bm_up / k_bm_across / k_bm_down<wire | mont_flag | table> and k_edbm_up /
k_edbm_across / k_edbm_down<wire | table> -- on stashes THE TEST writes, at the corners of the stash contract where no
whole call ever puts them.  The launchers (primtest_normalise_g1 / _ed in csrc/libmsm377_primtest.so) run the product's
own kernels at the product's own launch geometry; tests/normalise_model.py says, on Python integers, what every output
byte must be.  Comparison is bit exact.  Every call also checks the 256-byte guard bands behind the records and the flags.

tests/PRIMITIVES.md lists the seeded faults these tests were run against.
"""
import collections

import numpy as np
import pytest

import lazy_model as M
import normalise_model as NM

pytestmark = pytest.mark.gpu



def compared(curve, family, n, got, forms):
    """Every call says what it compared (pytest -s shows it); an empty family cannot pass silently."""
    assert n >= 1 and got == n * forms, (curve, family, n, got)
    print("%s %-10s n = %4d: %d outputs x %d forms compared" % (curve, family, n, n, forms))


@pytest.fixture(scope="module")
def dev():
    return M.device_backend()  # a missing library fails here


@pytest.fixture(scope="module")
def fp():
    return M.FieldModel("Fp")


@pytest.fixture(scope="module")
def fq():
    return M.FieldModel("Fq")


def first_difference(got, exp, labels, what):
    bad = np.argwhere((got != exp).any(axis=1))
    if len(bad):
        i = int(bad[0][0])
        raise AssertionError("%s: output %d of %d (%s) differs, %d outputs in all\n got %s\n exp %s"
                             % (what, i, len(got), labels[i % len(labels)] if labels else "", len(bad), got[i].tobytes().hex(), exp[i].tobytes().hex()))


def check_g1(dev, fm, family, rows, labels=None, forms=NM.G1_FORMS):
    """One stash through every form: records, flag bytes, both guard bands."""
    exp = NM.G1Expect(fm, rows)
    n, done = len(rows), 0
    for form, fid in forms.items():
        what = "G1 %s, %s, n = %d" % (form, family, n)
        rec, guard, inf, inf_guard = dev.normalise("g1", fid, rows)
        assert (guard == 0xEE).all() and len(guard) >= 256, (what, "the guard band behind the records was written")
        assert (inf_guard == 0xEE).all() and len(inf_guard) >= 256, (what, "the guard band behind the flag bytes was written")
        first_difference(rec, exp.records(form), labels, what)
        assert np.array_equal(inf, exp.inf), (what, "flag bytes", np.argwhere(inf != exp.inf)[:4].tolist())
        done += len(rec)
    compared("G1", family, n, done, len(forms))
    return exp


def check_ed(dev, fm, family, rows, labels=None):
    exp = NM.EdExpect(fm, rows)
    n, done = len(rows), 0
    for form, fid in NM.ED_FORMS.items():
        what = "Ed %s, %s, n = %d" % (form, family, n)
        rec, guard, _, _ = dev.normalise("ed", fid, rows)
        assert (guard == 0xEE).all() and len(guard) >= 256, (what, "the guard band behind the records was written")
        first_difference(rec, exp.records(form), labels, what)
        done += len(rec)
    compared("Ed", family, n, done, len(NM.ED_FORMS))
    return exp


@pytest.mark.parametrize("n", NM.SIZES)
def test_g1_corner_operands(dev, fp, n):
    """Every coordinate at the per-limb maxima of its box (all at once, each alone), and the value-maximal representatives
    x + k p: the operands tools/check_lazy_bounds.py normalisation_formulas() proves the columns for.  The rows go round
    from a different start at every size, so that every row meets every position of a thread's chain somewhere."""
    fam = NM.g1_corner_rows(fp)
    labels, rows = [l for l, _ in fam], [r for _, r in fam]
    assert labels[0] == "all corners" and rows[0] == sum((sh.box for _, sh in NM.stash_shapes(fp)), [])
    check_g1(dev, fp, "corners", NM.tile(rows, n), labels)
    if n > 1:
        check_g1(dev, fp, "corners", NM.tile(rows[:1], n), labels[:1])  # every output of the call at the corner of every box


@pytest.mark.parametrize("n", NM.SIZES)
def test_g1_zero_representatives_and_identities(dev, fp, n):
    """X in {0, p, .., 5p} and Y in {0, p} come out as THE canonical 0 in all three forms (Y = p is the operand for which
    mul_lz(Y, 1 / ZZZ) is exactly p: the table form's reduce_once is what makes it 0); limb-zero ZZ = ZZZ is the identity
    with its flag byte, flag word and record, and the neighbours stay exact."""
    fam = NM.g1_zero_rows(fp)
    labels, rows = [l for l, _ in fam], [r for _, r in fam]
    for offset in {0, 7 % n}:  # n = 1: row 0 (X = 0) and, separately below, the Y = p row alone
        exp = check_g1(dev, fp, "zeros", NM.tile(rows, n, offset), labels[offset:] + labels[:offset])
    yp = labels.index("Y = p")
    exp = check_g1(dev, fp, "zeros", NM.tile(rows[yp : yp + 1], n), ["Y = p"])
    assert exp.pts[0] is not None and exp.pts[0][1] == 0 and exp.pts[0][0] != 0
    table = exp.records("table")[0].view(np.uint32)
    assert not table[13:].any() and table[:13].any()  # y = 0, flag = 0, pads = 0 beside a real x


@pytest.mark.parametrize("n", NM.SIZES)
def test_g1_identity_placements(dev, fp, n):
    """Identities at lanes 0, 63, 64, 255, 256, n - 1, as all four outputs of one thread, as one whole workgroup and as
    ALL outputs of the call, among random in-box rows."""
    base = NM.random_rows(fp, min(n, 1024), 3)
    placements = NM.identity_placements(n)
    names = [l for l, _ in placements]
    assert names[:2] == ["seams", "all"]
    assert n < 3 * NM.THREADS + 6 or any(l.startswith("all four outputs") for l in names)
    assert n <= NM.BLOCK or any(l.startswith("workgroup") for l in names)
    for label, lanes in placements:
        rows = NM.with_identities(fp, NM.tile(base, n), lanes)
        exp = check_g1(dev, fp, "identities", rows, [label])
        assert int(exp.inf.sum()) == len(lanes) >= 1


def test_g1_null_out_inf_is_accepted(dev, fp):
    fam = NM.g1_zero_rows(fp)
    rows = NM.tile([r for _, r in fam], 257)
    exp = NM.G1Expect(fp, rows)
    for form, fid in NM.G1_FORMS.items():
        rec, guard, inf, _ = dev.normalise("g1", fid, rows, with_inf=False)
        assert inf is None and (guard == 0xEE).all()
        first_difference(rec, exp.records(form), [l for l, _ in fam], "G1 %s, null out_inf" % form)


def test_g1_steered_chunk_products(dev, fp):
    """The ONE inversion of k_bm_across on chosen residues: n = 1 with ZZZ = a, and chunks of 2, 257, 1025 and 3079 outputs
    whose ZZZ's multiply to a -- the Montgomery 1, 2, p - 1, 2^j, and the smallest and largest k of the k-model.  Both arms of
    inverse_mont's conversion (k < 436 and not) run on the device here; a whole call practically never takes the first."""
    walk = M.INVERSE_WALK["Fp"]
    arms = collections.Counter()
    for i, (label, a) in enumerate(NM.steered_values(fp)):
        k = M.kaliski_k(fp, a)
        arms[k < walk["short_below"]] += 1
        for n in (1, 2, 257, 1025, 3 * 1024 + 7)[: 5 if i % 3 == 0 else 2]:
            rows = NM.steered_rows(fp, a, n, 20 + i)
            assert NM.chunk_product(fp, rows) == a
            check_g1(dev, fp, "steered", rows, ["%s (k = %d)" % (label, k)])
    print("steered chunk products: %d in the short-k arm, %d in the other" % (arms[True], arms[False]))
    assert arms[True] >= 3 and arms[False] >= 3


@pytest.mark.parametrize("n", NM.SIZES)
def test_g1_random_baseline(dev, fp, n):
    """1024 seeded random in-box operands (limbs from {0, maximum, uniform})."""
    rows = NM.random_rows(fp, 1024, 1)
    check_g1(dev, fp, "random", NM.tile(rows, n))


@pytest.mark.parametrize("n", NM.SIZES)
def test_ed_value_rows_and_random(dev, fq, n):
    """The Edwards stash under its own contract (canonical coordinates, Z != 0): coordinates from {0, 1, q - 1, the
    canonical corner}, identities (0 : c : 0 : c) -> (0, 1), random rows; both forms."""
    fam = NM.ed_value_rows(fq)
    labels, rows = [l for l, _ in fam], [r for _, r in fam]
    exp = check_ed(dev, fq, "values", NM.tile(rows, n, n % len(rows)), labels[n % len(rows) :] + labels[: n % len(rows)])
    if n >= len(rows):
        ident = [i for i in range(len(rows)) if labels[(n + i) % len(rows)].startswith("identity")]
        assert len(ident) == 4 and all(exp.pts[i] == (0, 1) for i in ident)
    check_ed(dev, fq, "random", NM.tile(NM.random_rows(fq, 1024, 2), n))
    check_ed(dev, fq, "corners", NM.tile([r for l, r in fam if l == "all corners"], n), ["all corners"])


def test_ed_steered_chunk_products(dev, fq):
    """k_edbm_across's inversion on chosen residues, both arms of FqInverse::inverse_mont (k < 270 and not)."""
    walk = M.INVERSE_WALK["Fq"]
    arms = collections.Counter()
    for i, (label, a) in enumerate(NM.steered_values(fq)):
        k = M.kaliski_k(fq, a)
        arms[k < walk["short_below"]] += 1
        for n in (1, 257, 3 * 1024 + 7)[: 3 if i % 3 == 0 else 1]:
            rows = NM.steered_rows(fq, a, n, 40 + i)
            check_ed(dev, fq, "steered", rows, ["%s (k = %d)" % (label, k)])
    assert arms[True] >= 3 and arms[False] >= 3
