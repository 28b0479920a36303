"""Every base record and window table the hot kernels gather from, read back and held against tests/record_model.py.

msm377_g1_read_bases describes what the last conversion of a context left -- projective or affine twisted Edwards records,
the windows of a precomputed table, Weierstrass records (with their GLV half), Edwards-BLS12 records --
msm377_g1_read_mul_table the window tables of the batch operations.  For every record read the tests check the info
words, that every pad word is zero, that every limb lies inside the box the interval proof starts from
(tools/check_lazy_bounds.py shapes(): `canonical`, and `stored` for the affine 2d x y) and every value below its bound --
over ALL records of a read, in NumPy -- and that the words (the residue, for a lazy coordinate) are the model's: over all
records where n <= 2049 and there is one window, elsewhere over record_model.sample_indices().

A record that is the right point mod p in the wrong form -- y + x stored lazily, a coordinate with p added, a 2 Z that
is not canonical -- keeps every MSM result exact; here it fails with the record, the window and the coordinate named.
tests/STAGES.md ("base records") lists the faults these tests were run against."""
import random

import numpy as np
import pytest

import batch_mul_vectors as V
import check_vectors as CV
import ed_curve_points as E
import pyref as R
import record_model as RM
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, ESTATE

pytestmark = pytest.mark.gpu

AFF_THREADS, AFF_K, AFF_BLOCK_POINTS = 256, 8, 2048  # csrc/common.hpp: the batched conversion's indexing
SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4097)
N_POOL = 4097
LANES = (0, 63, 64, 255, 256)
T2 = (R.P - 1, 0)
A0, D0 = 0xBA5E5EED, 0x7AB1E


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


def make_engine(max_points=N_POOL, **env):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        return msm.MsmEngine(max_points)


@pytest.fixture(scope="module")
def pool(oracle):
    """4097 subgroup points P_i = [A0 + i D0]G, as wire bytes and as integers; every case takes a prefix."""
    wire = util.oracle_gen_points(oracle, N_POOL, A0, D0)
    return wire, R.decode_points(wire)


@pytest.fixture(scope="module")
def aff():
    """Every msm_device call of this context converts to affine records; capture mode 2 (as run) so that a geometry rerun
    can be told from none -- the read-back does not depend on the mode, the other contexts here run without capture."""
    eng = make_engine(MSM377_AFFINE_MIN=1)
    eng.set_stage_capture(2)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def small():
    """A context with the default knobs: projective records per call (below 2^20 points), affine resident tables."""
    eng = make_engine()
    yield eng
    eng.close()


def run(eng, call, products=None, captured=False):
    """Make one engine call and return verify(expected).  The verdicts on the call -- its result, no fallback to the
    Weierstrass path, the accumulation kernel of `products` field products per addition, and (on a capturing context,
    which never sees a scalar its first geometry refuses) no geometry rerun -- are taken now and asserted by verify(), which
    the tests call AFTER the records were checked: a record in the wrong form is then reported as that record and that
    coordinate, not as "the result differs"."""
    before, _ = eng.fallback_info()
    got = call()
    after, mask = eng.fallback_info()
    ran = eng.accumulate_products()
    reruns = eng.read_stage_ex(0, want=())[0].geometry_reruns if captured else 0

    def verify(expected):
        assert after == before, "%d rerun(s) on the Weierstrass path, mask 0x%x" % (after - before, mask)
        assert products is None or ran == products, "%d field products per addition, expected %d" % (ran, products)
        assert reruns == 0, "a geometry rerun happened"
        assert got == expected, "the result differs"

    return verify


def scalars_for(n, seed):
    return R.rand_scalars(seed, n)


def check_read(eng, form, points, *, windows=1, widths=(), glv=False, flagged=0, seed=0, what=""):
    """Read every record of the last conversion and hold it against the model.  points: the n Weierstrass points of the
    call (for FORM_ED: Edwards-BLS12 points).  Returns the info."""
    n = len(points)
    stride = n
    info, words = eng.read_bases()
    exp_records = windows * n if windows > 1 else (2 * n if glv else n)
    assert (info.form, info.record_words, info.limbs, info.coords) == (form, RM.RECORD_WORDS[form], RM.LIMBS[form], RM.COORDS[form]), (what, info)
    assert (info.n, info.windows, info.window_stride, info.glv, info.records, info.flagged) == (n, windows, stride, int(glv), exp_records, flagged), (what, info)
    assert info.window_bits == tuple(widths), (what, info)
    assert words.shape == (exp_records, RM.RECORD_WORDS[form])
    # a partial read addresses the same records
    if exp_records > 2:
        _, part = eng.read_bases(first=exp_records - 2, count=2)
        assert (part == words[-2:]).all(), what
    RM.check_boxes(words, form, where="%s: " % what, stride=stride if windows > 1 else exp_records)
    if windows > 1:
        table = [RM.window_points(pt, widths) for pt in points]  # table[i][w] = [2^offset_w] P_i
        for t in RM.sample_indices(n, windows, stride, 256, seed):
            w, i = divmod(t, stride)
            RM.check_record(words[t], RM.record_words(form, table[i][w]), form, "%s: record %d of window %d (record %d)" % (what, i, w, t))
        return info
    for t in RM.sample_indices(exp_records, 1, exp_records, 256, seed):
        phi = glv and t >= n
        RM.check_record(words[t], RM.record_words(form, points[t - n if phi else t], phi=phi), form, "%s: record %d of window 0%s" % (what, t, " (phi half)" if phi else ""))
    return info


def offered_indices(n):
    return [i for i in (0, 255, 256, 2047, 2048, n - 1) if i < n]


def test_the_inputs_offer_the_indices():
    """From the model alone, before anything runs on the GPU: the sizes reach every index the comparison must visit --
    both sides of a thread's stride (AFF_THREADS), of a block (AFF_BLOCK_POINTS) and the last record."""
    assert AFF_THREADS * AFF_K == AFF_BLOCK_POINTS
    reach = set()
    for n in SIZES:
        s = set(RM.sample_indices(n, 1, n, 256, n))
        assert set(offered_indices(n)) <= s and n - 1 in s
        reach |= set(offered_indices(n))
    assert reach >= {0, 255, 256, 2047, 2048, 4096}
    for n, windows in ((257, 16), (2049, 16), (257, 13), (2049, 13), (300, 16), (300, 13)):
        s = set(RM.sample_indices(n, windows, n, 256, (n, windows)))
        for w in range(windows):
            assert {w * n + i for i in offered_indices(n)} <= s
        assert set(range(n)) <= s and set(range((windows - 1) * n, windows * n)) <= s and set(range(n, 2 * n)) <= s
    assert RM.sample_indices(2049, 1, 2049, 256, 0) == list(range(2049))


# ---- before the first conversion, and after one that failed ----
def test_estate_before_and_after_a_failed_conversion(pool):
    wire, pts = pool
    eng = make_engine(max_points=512)
    try:
        with pytest.raises(msm.MsmError) as e:
            eng.read_bases()
        assert e.value.code == ESTATE
        for which, index in (("single", 0), ("multi", 0), ("multi", 15), ("generator", 0)):
            with pytest.raises(msm.MsmError) as e:
                eng.read_mul_table(which, index, info_only=True)
            assert e.value.code == ESTATE, (which, index)
        n = 300
        d_p, d_s = dev(wire[: 96 * n]), dev(R.encode_scalars(scalars_for(n, 1)))
        eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), n)
        info, none = eng.read_bases(info_only=True)
        assert none is None and info.n == n and info.form == RM.FORM_TE_PROJECTIVE
        with pytest.raises(msm.MsmError) as e:
            eng.read_bases(first=n, count=1)
        assert e.value.code == EINVAL
        # a scalar the signed recode cannot hold fails the call behind its conversion: nothing is described afterwards
        d_bad = dev(R.encode_scalars([2**256 - 1] * n))
        with pytest.raises(msm.MsmError):
            eng.msm_device(d_p.data_ptr(), d_bad.data_ptr(), n)
        with pytest.raises(msm.MsmError) as e:
            eng.read_bases()
        assert e.value.code == ESTATE
        eng.set_bases_device(d_p.data_ptr(), n)
        check_read(eng, RM.FORM_TE_AFFINE, pts[:n], what="set_bases_device after a failed call")
    finally:
        eng.close()


# ---- affine records ----
@pytest.mark.parametrize("n", SIZES)
def test_affine_records_per_call(aff, oracle, pool, n):
    wire, pts = pool
    ks = R.encode_scalars(scalars_for(n, 0xAF00 + n))
    d_p, d_s = dev(wire[: 96 * n]), dev(ks)
    verify = run(aff, lambda: aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=7, captured=True)
    check_read(aff, RM.FORM_TE_AFFINE, pts[:n], seed=n, what="msm_device n=%d" % n)
    verify(util.oracle_msm(oracle, wire[: 96 * n], ks))


@pytest.mark.parametrize("n", SIZES)
def test_affine_records_of_a_resident_set(small, oracle, pool, n):
    wire, pts = pool
    d_p = dev(wire[: 96 * n])
    small.set_bases_device(d_p.data_ptr(), n)
    check_read(small, RM.FORM_TE_AFFINE, pts[:n], seed=n, what="set_bases_device n=%d" % n)
    ks = R.encode_scalars(scalars_for(n, 0xAF10 + n))
    d_s = dev(ks)
    verify = run(small, lambda: small.msm_fixed_base_device(d_s.data_ptr(), n), products=7)
    check_read(small, RM.FORM_TE_AFFINE, pts[:n], seed=n, what="set_bases_device n=%d, after a fixed-base call" % n)
    verify(util.oracle_msm(oracle, wire[: 96 * n], ks))


def test_affine_records_from_host_buffers(small, pool):
    wire, pts = pool
    small.set_bases(wire[: 96 * 2049])
    check_read(small, RM.FORM_TE_AFFINE, pts[:2049], what="set_bases n=2049")


# ---- projective records ----
@pytest.mark.parametrize("n", (1, 255, 256, 257, 1000))
def test_projective_records_per_call(small, oracle, pool, n):
    wire, pts = pool
    ks = R.encode_scalars(scalars_for(n, 0x9E00 + n))
    d_p, d_s = dev(wire[: 96 * n]), dev(ks)
    verify = run(small, lambda: small.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=8)
    check_read(small, RM.FORM_TE_PROJECTIVE, pts[:n], what="msm_device n=%d" % n)
    verify(util.oracle_msm(oracle, wire[: 96 * n], ks))


def chunk_cuts(n, chunks=4, split_pct=30):
    """The chunks of a host-buffer upload (include/msm377.h, MSM377_UPLOAD_CHUNKS / _SPLIT): the first holds split_pct of the
    points, the others share the rest evenly, every edge rounded down to a multiple of 64."""
    first_end = max(64, (n * split_pct // 100) & ~63)
    cuts = [0]
    for c in range(1, chunks):
        b = first_end if c == 1 else (first_end + (n - first_end) * (c - 1) // (chunks - 1)) & ~63
        if cuts[-1] < b < n:
            cuts.append(b)
    return cuts + [n]


def test_projective_records_of_a_chunked_upload(oracle, pool):
    """engine.msm from MSM377_UPLOAD_CHUNK_MIN points on converts every chunk at its own offset, while the next one is on its
    way: all n records must be exact after the call."""
    wire, pts = pool
    n = 1100
    cuts = chunk_cuts(n)
    assert len(cuts) == 5 and all(c % 256 for c in cuts[1:-1]) and all(c % 64 == 0 for c in cuts[1:-1]), cuts
    eng = make_engine(MSM377_UPLOAD_CHUNK_MIN=100)
    try:
        ks = R.encode_scalars(scalars_for(n, 0xC4C4))
        verify = run(eng, lambda: eng.msm(wire[: 96 * n], ks), products=8)
        check_read(eng, RM.FORM_TE_PROJECTIVE, pts[:n], what="msm (chunks at %s)" % cuts)
        verify(util.oracle_msm(oracle, wire[: 96 * n], ks))
    finally:
        eng.close()


# ---- precomputed tables ----
@pytest.mark.parametrize("c, widths", [(16, RM.WINDOWS16), (20, RM.WIDE_WIDTHS)], ids=["c16", "c20"])
def test_precomputed_tables(oracle, pool, c, widths):
    wire, pts = pool
    eng = make_engine(max_points=2049)
    try:
        eng.set_precompute_window(c)
        for n in (257, 2049, 300):  # the last one on the allocation of the 2049: the stride is the new n
            d_p = dev(wire[: 96 * n])
            eng.set_bases_precomputed_device(d_p.data_ptr(), n)
            what = "set_bases_precomputed c=%d n=%d" % (c, n)
            info = check_read(eng, RM.FORM_TE_AFFINE, pts[:n], windows=len(widths), widths=widths, seed=(c, n), what=what)
            assert info.window_stride == n and info.records == len(widths) * n
            ks = R.encode_scalars(scalars_for(n, 0x7AB0 + n))
            d_s = dev(ks)
            verify = run(eng, lambda: eng.msm_fixed_base_device(d_s.data_ptr(), n), products=7)
            check_read(eng, RM.FORM_TE_AFFINE, pts[:n], windows=len(widths), widths=widths, seed=(c, n, "again"), what=what + ", after a fixed-base call")
            verify(util.oracle_msm(oracle, wire[: 96 * n], ks))
    finally:
        eng.close()


# ---- Weierstrass records ----
def test_weierstrass_records_and_the_glv_half(oracle, pool):
    wire, pts = pool
    eng = make_engine(max_points=1024)
    try:
        eng.set_g1_form("weierstrass")
        for n in (1, 257, 600):
            ks = R.encode_scalars(scalars_for(n, 0x3E1 + n))
            d_p, d_s = dev(wire[: 96 * n]), dev(ks)
            verify = run(eng, lambda: eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=10)
            check_read(eng, RM.FORM_WEIERSTRASS, pts[:n], what="weierstrass msm_device n=%d" % n)
            verify(util.oracle_msm(oracle, wire[: 96 * n], ks))
        eng.set_glv(1)
        for n in (1, 257, 600):
            ks = R.encode_scalars(scalars_for(n, 0x61F + n))
            d_p, d_s = dev(wire[: 96 * n]), dev(ks)
            verify = run(eng, lambda: eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=10)
            check_read(eng, RM.FORM_WEIERSTRASS, pts[:n], glv=True, what="GLV msm_device n=%d" % n)
            verify(util.oracle_msm(oracle, wire[: 96 * n], ks))
        d_p = dev(wire[: 96 * 600])
        eng.set_bases_device(d_p.data_ptr(), 600)
        check_read(eng, RM.FORM_WEIERSTRASS, pts[:600], glv=True, what="GLV set_bases_device")
    finally:
        eng.close()


def test_weierstrass_records_after_a_fallback(small, pool):
    """(-1, 0) at index 256 of 600: the Edwards map does not cover it, so the per-call route reruns and a resident table is
    rebuilt, both on Weierstrass records, and the read-back must describe those."""
    _, pts = pool
    n = 600
    pl = list(pts[:n])
    pl[256] = T2
    kl = R.rand_scalars(0xFA11, n, modulus=1 << 64)
    kl[256] = 5
    exp = R.encode_result(R.msm_naive(pl, kl))
    wire, ks = R.encode_points(pl), R.encode_scalars(kl)
    d_p, d_s = dev(wire), dev(ks)
    before, _ = small.fallback_info()
    assert small.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp
    assert small.fallback_info()[0] == before + 1
    check_read(small, RM.FORM_WEIERSTRASS, pl, what="msm_device after the fallback")
    small.set_bases_device(d_p.data_ptr(), n)
    info, _ = small.read_bases(info_only=True)
    assert info.form == RM.FORM_TE_AFFINE and info.n == n  # built in the Edwards form; the flag waits for the first call
    assert small.msm_fixed_base_device(d_s.data_ptr(), n) == exp
    assert small.fallback_info()[0] == before + 2
    check_read(small, RM.FORM_WEIERSTRASS, pl, what="resident table after the fallback")
    assert small.msm_fixed_base_device(d_s.data_ptr(), n) == exp  # served by the rebuilt table: no further rerun
    assert small.fallback_info()[0] == before + 2


# ---- Edwards-BLS12 records ----
@pytest.mark.parametrize("n", (1, 257, 1000))
def test_edwards_bls12_records(small, n):
    """The law is complete: every curve point has a record, the low-order ones included."""
    points, scalars, planted, expected = E.every_curve_point(n)
    assert n < 64 or any("alone" in v for v in planted.values())
    d_p, d_s = dev(R.ed_encode_points(points)), dev(R.encode_scalars(scalars))
    got = small.ed_msm_device(d_p.data_ptr(), d_s.data_ptr(), n)
    check_read(small, RM.FORM_ED, points, what="ed_msm_device n=%d" % n)
    assert got == R.ed_encode_result(expected)


# ---- special coordinates ----
def odd_order_outside_the_subgroup():
    """The suite's points outside the subgroup, brought to odd order where needed (the cofactor is even; an even-order
    point makes exceptional pairs): what is left of `torsion` after its 2-part, and G plus that."""
    out = [("(0, 1)", (0, 1)), ("(0, p - 1)", (0, R.P - 1))]
    torsion = dict(V.bases())["torsion"]
    # [2^128] of a cofactor-torsion point has no 2-part left (the cofactor is below 2^126)
    odd = R.mul(torsion, 1 << 128)
    if odd is not None and RM.te_representable(odd):
        out += [("odd torsion", odd), ("G + odd torsion", R.add(R.G, odd))]
    return out


def planted_points(pts, n, specials):
    pl = list(pts[:n])
    where = {}
    for j, lane in enumerate(LANES + (n - 1,)):
        name, pt = specials[j % len(specials)]
        pl[lane] = pt
        where[lane] = name
    return pl, where


def test_special_coordinates_in_edwards_records(small, aff, pool):
    _, pts = pool
    n = 300
    specials = odd_order_outside_the_subgroup()
    assert len(specials) >= 2 and all(R.on_curve(p) and RM.te_representable(p) for _, p in specials)
    assert RM.te_affine((0, 1))[0] != 0 and RM.te_affine_words((0, R.P - 1))[0] != RM.te_affine_words((0, 1))[0]
    pl, where = planted_points(pts, n, specials)
    kl = R.rand_scalars(0x5EC1, n, modulus=1 << 32)
    exp = R.encode_result(R.msm_naive(pl, kl))
    d_p, d_s = dev(R.encode_points(pl)), dev(R.encode_scalars(kl))
    verify = run(small, lambda: small.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=8)
    check_read(small, RM.FORM_TE_PROJECTIVE, pl, what="projective, specials at %s" % where)
    verify(exp)
    verify = run(aff, lambda: aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=7, captured=True)
    check_read(aff, RM.FORM_TE_AFFINE, pl, what="affine, specials at %s" % where)
    verify(exp)
    small.set_bases_device(d_p.data_ptr(), n)
    check_read(small, RM.FORM_TE_AFFINE, pl, what="resident affine, specials at %s" % where)


def test_special_coordinates_in_weierstrass_records(pool):
    """Every curve point has a Weierstrass record: a coordinate of p - 1 ((-1, 0)), x = 0, the other 2-torsion points."""
    _, pts = pool
    n = 300
    specials = [("(-1, 0)", T2), ("(0, 1)", (0, 1)), ("(0, p - 1)", (0, R.P - 1)), ("T'", util.t_prime())] + [(nm, p) for nm, p in V.bases() if nm in ("torsion", "G_plus_torsion")]
    pl, where = planted_points(pts, n, specials)
    kl = R.rand_scalars(0x5EC2, n, modulus=1 << 32)
    eng = make_engine(max_points=512)
    try:
        eng.set_g1_form("weierstrass")
        d_p, d_s = dev(R.encode_points(pl)), dev(R.encode_scalars(kl))
        assert eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(R.msm_naive(pl, kl))
        check_read(eng, RM.FORM_WEIERSTRASS, pl, what="weierstrass, specials at %s" % where)
    finally:
        eng.close()


def test_flagged_points_hold_the_generator(pool):
    """MSM377_POINTS_MONT_FLAG: a flagged record's base record is the generator's (its scalar is zeroed instead), and
    info.flagged counts them -- per call and for a resident set."""
    _, pts = pool
    n = 300
    flagged_at = sorted(set(LANES + (n - 1,)))
    native = [None if i in flagged_at else pts[i] for i in range(n)]
    as_converted = [R.G if i in flagged_at else pts[i] for i in range(n)]
    kl = R.rand_scalars(0xF1A6, n, modulus=1 << 32)
    exp = R.encode_result(R.msm_naive([p for p in native if p is not None], [k for p, k in zip(native, kl) if p is not None]))
    for env, form, products in (({}, RM.FORM_TE_PROJECTIVE, 8), ({"MSM377_AFFINE_MIN": 1}, RM.FORM_TE_AFFINE, 7)):
        eng = make_engine(max_points=512, **env)
        try:
            eng.set_input_format("mont_flag", "wire")
            d_p, d_s = dev(msm.encode_points_native(native, "mont_flag")), dev(R.encode_scalars(kl))
            verify = run(eng, lambda: eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), n), products=products)
            check_read(eng, form, as_converted, flagged=len(flagged_at), what="mont_flag msm_device")
            verify(exp)
            eng.set_bases_device(d_p.data_ptr(), n)
            check_read(eng, RM.FORM_TE_AFFINE, as_converted, flagged=len(flagged_at), what="mont_flag set_bases_device")
            assert eng.msm_fixed_base_device(d_s.data_ptr(), n) == exp
        finally:
            eng.close()


# ---- window tables ----
def table_bases():
    """The generator, a base of order 3, one of order 4 (whole rows of identity flags) and one outside the subgroup."""
    b = dict(V.bases())
    small = CV.g1_small_order_points()
    order3 = next(t for t in small if R.mul(t, 3) is None)
    order4 = next(t for t in small if R.mul(t, 2) is not None and R.mul(t, 4) is None)
    return [("G", R.G, 0), ("order3", order3, 3), ("order4", order4, 4), ("G_plus_torsion", b["G_plus_torsion"], 0)]


def check_table_info(info, c, key):
    assert (info.width, info.rows, info.records, info.key) == (c, RM.table_windows(c) + 1, RM.table_records(c), key)


def expected_flags(c, order):
    """flag[t] of a table whose base has the small order `order` (0: no record is the identity)."""
    t = np.arange(RM.table_records(c), dtype=np.int64)
    if not order:
        return np.zeros(t.shape, dtype=np.uint32)
    w, d = t >> (c - 1), (t & ((1 << (c - 1)) - 1)) + 1
    weight = np.array([pow(2, c * int(x), order) for x in range(RM.table_windows(c) + 1)], dtype=np.int64)
    return ((d * weight[w]) % order == 0).astype(np.uint32)


@pytest.mark.parametrize("name, base, order", table_bases(), ids=[b[0] for b in table_bases()])
def test_single_base_table_c8_every_record(small, name, base, order):
    d_s, d_out = dev(R.encode_scalars([1, 2, 3, R.R_ORDER - 1])), dev(bytes(96 * 4))
    small.set_mul_window(8)
    try:
        small.batch_mul_device(V.base_bytes(base), d_s.data_ptr(), 4, d_out.data_ptr())
    finally:
        small.set_mul_window(0)
    info, words = small.read_mul_table("single")
    check_table_info(info, 8, V.base_bytes(base))
    assert words.shape == (4097, 32)
    RM.check_table_boxes(words, where="%s c=8: " % name)
    assert (words[:, RM.TABLE_FLAG_WORD] == expected_flags(8, order)).all()
    for t, pt in enumerate(RM.table_rows(base, 8)):
        RM.check_table_record(words[t], pt, 8, t, "%s c=8: " % name)
    _, part = small.read_mul_table("single", first=4095, count=2)
    assert (part == words[4095:]).all()


@pytest.mark.parametrize("name, base, order", table_bases(), ids=[b[0] for b in table_bases()])
def test_single_base_table_c16(small, name, base, order):
    """524 289 records: all boxed and flag-checked; compared: d = 1, 2, 2^15 - 1, 2^15 of every row, the carry row's single
    record and 256 seeded others."""
    c = 16
    d_s, d_out = dev(R.encode_scalars([1, 2, 3, R.R_ORDER - 1])), dev(bytes(96 * 4))
    small.set_mul_window(c)
    try:
        small.batch_mul_device(V.base_bytes(base), d_s.data_ptr(), 4, d_out.data_ptr())
    finally:
        small.set_mul_window(0)
    info, words = small.read_mul_table("single")
    check_table_info(info, c, V.base_bytes(base))
    assert words.shape == (RM.table_records(c), 32) and RM.table_records(c) == 524289
    RM.check_table_boxes(words, where="%s c=16: " % name)
    flags = expected_flags(c, order)
    bad = np.flatnonzero(words[:, RM.TABLE_FLAG_WORD] != flags)
    assert bad.size == 0, "%s c=16: record %d (row %d): flag %d" % (name, bad[0], bad[0] >> 15, words[bad[0], RM.TABLE_FLAG_WORD])
    picks = {RM.table_index(c, w, d) for w in range(16) for d in (1, 2, (1 << 15) - 1, 1 << 15)} | {RM.table_records(c) - 1}
    rnd = random.Random("c16 table/%s" % name)
    while len(picks) < 65 + 256:
        picks.add(rnd.randrange(RM.table_records(c)))
    for t in sorted(picks):
        RM.check_table_record(words[t], RM.table_point(base, c, t), c, t, "%s c=16: " % name)


def test_multi_base_slots(small):
    """k = 3 with B_1 = -B_0: both slots are read; slot 2 survives a following k = 2 call untouched."""
    b = dict(V.bases())
    b0, b2 = b["fixed_base"], b["G_plus_torsion"]
    bases = [b0, R.neg(b0), b2]
    rows = [RM.table_rows(x, 8) for x in bases]
    small.set_mul_window(8)
    try:
        d_s, d_out = dev(R.encode_scalars([1, 2, 3, 4, 5, 6])), dev(bytes(96 * 2))
        small.batch_mul_multi_device(R.encode_points(bases), d_s.data_ptr(), 2, d_out.data_ptr())
        tables = []
        for j in range(3):
            info, words = small.read_mul_table("multi", j)
            check_table_info(info, 8, V.base_bytes(bases[j]))
            RM.check_table_boxes(words, where="slot %d: " % j)
            for t, pt in enumerate(rows[j]):
                RM.check_table_record(words[t], pt, 8, t, "slot %d: " % j)
            tables.append(words)
        assert (tables[0][:, :13] == tables[1][:, :13]).all() and (tables[0][:, 13:26] != tables[1][:, 13:26]).any(axis=1).all()
        builds = small.mul_multi_table_builds()
        other = [R.G, b["torsion"]]
        small.batch_mul_multi_device(R.encode_points(other), d_s.data_ptr(), 2, d_out.data_ptr())
        assert small.mul_multi_table_builds() == builds + 2
        info, words = small.read_mul_table("multi", 2)
        check_table_info(info, 8, V.base_bytes(b2))
        assert (words == tables[2]).all(), "slot 2 changed under a k = 2 call"
        for j in range(2):
            info, words = small.read_mul_table("multi", j)
            check_table_info(info, 8, V.base_bytes(other[j]))
            for t in (0, 127, 128, 4095, 4096):
                RM.check_table_record(words[t], RM.table_point(other[j], 8, t), 8, t, "slot %d, second call: " % j)
        with pytest.raises(msm.MsmError) as e:
            small.read_mul_table("multi", 3, info_only=True)
        assert e.value.code == ESTATE
    finally:
        small.set_mul_window(0)


def test_generator_tables(small):
    """k = 17 at c = 8: generators 0, 15 and 16 -- both sides of the edge of a segment of 16; a set that failed to build
    leaves nothing to read."""
    gens = [R.mul(R.G, 3 + 5 * j) for j in range(17)]
    gens[15] = (0, 1)  # order 3: flagged entries inside the set
    small.set_generators(R.encode_points(gens), 8)
    try:
        assert small.generators() == (17, 8)
        for j in (0, 15, 16):
            info, words = small.read_mul_table("generator", j)
            check_table_info(info, 8, bytes(96))
            RM.check_table_boxes(words, where="generator %d: " % j)
            assert (words[:, RM.TABLE_FLAG_WORD] == expected_flags(8, 3 if j == 15 else 0)).all()
            for t, pt in enumerate(RM.table_rows(gens[j], 8)):
                RM.check_table_record(words[t], pt, 8, t, "generator %d: " % j)
        with pytest.raises(msm.MsmError) as e:
            small.read_mul_table("generator", 17, info_only=True)
        assert e.value.code == ESTATE
        bad = R.encode_points(gens[:2]) + (R.P).to_bytes(48, "little") + (1).to_bytes(48, "little")
        with pytest.raises(msm.MsmError):
            small.set_generators(bad, 8)
        assert small.generators() == (0, 0)
        with pytest.raises(msm.MsmError) as e:
            small.read_mul_table("generator", 0, info_only=True)
        assert e.value.code == ESTATE
    finally:
        small.set_generators(None)
