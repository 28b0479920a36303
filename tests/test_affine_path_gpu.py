"""The per-call affine Edwards path of msm377_g1_msm_device (and of the window partials) at its edges.

From MSM377_AFFINE_MIN points on (2^20 by default) msm377_g1_msm_device converts the points to affine twisted Edwards
records on every call -- k_affine_up, a host inversion of the block products, k_affine_down (kernels/convert.hpp),
queued behind the sort through the before_accumulate hook -- and accumulates them with the 7-product madd_affine.
Below that size the records are projective, so the edge cases of the other modules never reach this path.  Here a
context created with MSM377_AFFINE_MIN=1 sends every msm_device call through it, and the 2^20 cases run it under the
default knobs.

Every case is bit-exact against the CPU oracle, pyref or a closed form.  Cases whose points all lie in the prime-order
subgroup also assert that nothing reran on the Weierstrass path (a false exceptional flag would keep the results exact
and only halve the speed) and that the last accumulation launch took 7 products per addition, i.e. that the affine
kernel ran.  Host-buffer calls (engine.msm) do not pin their product count."""
import pytest

import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from test_g1_parity_gpu import check_edwards_law_placements, dev, even_edge_scalars, seeded_inputs
from webgpu_msm_bls12_377_amd.host.engine import FB_CONVERT, WINDOW_PARTIAL_BYTES

pytestmark = pytest.mark.gpu

AFF_BLOCK_POINTS = 2048  # points per workgroup of the conversion (csrc/common.hpp)
T2 = (R.P - 1, 0)  # the 2-torsion point (-1, 0): the Edwards map does not cover it (ERR_TE_CONVERT)
N_POOL = 100003


def affine_engine(affine_min, max_points=1 << 17):
    """A context whose msm_device calls take affine records from affine_min points on (knobs are read at creation)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_AFFINE_MIN", str(affine_min))
        return msm.MsmEngine(max_points)


@pytest.fixture(scope="module")
def aff():
    eng = affine_engine(1)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def pool(oracle):
    """One set of seeded points; every case below takes a prefix."""
    return seeded_inputs(oracle, N_POOL, 0xAFF1)[0]


def device_msm(eng, pts, ks):
    d_p, d_s = dev(pts), dev(ks)
    return eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(ks) // 32)


def replaced(base, pl, kl, i, pt=None, k=None):
    """base - k_i P_i + k P: the expected result after one input of a known MSM changes (pyref, Python integers)."""
    pt = pl[i] if pt is None else pt
    k = kl[i] if k is None else k
    return R.add(R.add(base, R.neg(R.mul(pl[i], kl[i]))), R.mul(pt, k))


# ---- a. sizes at the conversion's block edges ----
@pytest.mark.parametrize(
    "geometry, sizes",
    [
        ("narrow", [1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4097, 63488, 63489, 65536]),
        ("even", [1, 257, 2048, 2049, 10007, 65537, 100003]),
    ],
)
def test_sizes_at_the_block_edges(aff, oracle, pool, geometry, sizes):
    """Whole and partial blocks of AFF_BLOCK_POINTS, one block, 31 / 32 blocks (the tail pool's prewake from 32 on:
    63488 = 31 x 2048), on both window geometries of the affine records."""
    aff.set_narrow_max(1 << 16 if geometry == "narrow" else 0)
    try:
        for n in sizes:
            pts = pool[: 96 * n]
            ks = R.encode_scalars(R.rand_scalars(0xA000 + n, n))
            with util.edwards_only(aff, products=7):
                assert device_msm(aff, pts, ks) == util.oracle_msm(oracle, pts, ks), (geometry, n)
    finally:
        aff.set_narrow_max()


# ---- b. edge scalars of the even geometry ----
def test_even_edge_scalars_on_affine_records(aff, oracle, pool):
    """The even geometry's edge scalars one at a time and all together, and scalars of 2^253 and more at the first
    point, both sides of the first block edge and the last point of a partial block: the call reruns on sixteen equal
    windows after the hook has been used up, with the affine records still in place."""
    n = 4100  # two whole blocks and a partial one
    pts = pool[: 96 * n]
    kl = R.rand_scalars(0xB0B, n)
    pl = R.decode_points(pts)
    base = R.decode_result(util.oracle_msm(oracle, pts, R.encode_scalars(kl)))
    aff.set_narrow_max(0)
    d_p = dev(pts)
    try:
        edge = even_edge_scalars()
        for i, k in enumerate(edge):
            kk = list(kl)
            kk[i] = k
            d_s = dev(R.encode_scalars(kk))
            with util.edwards_only(aff, products=7):
                assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(replaced(base, pl, kl, i, k=k)), hex(k)
        kk = list(kl)
        kk[: len(edge)] = edge
        exp = base
        for i, k in enumerate(edge):
            exp = replaced(exp, pl, kl, i, k=k)
        d_s = dev(R.encode_scalars(kk))
        with util.edwards_only(aff, products=7):
            assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(exp)
        bigs = [(1 << 253) + 3, (1 << 254) + 5, (1 << 254) - 1, (1 << 255) - (1 << 239) - (1 << 224)]
        where = [0, AFF_BLOCK_POINTS - 1, AFF_BLOCK_POINTS, n - 1]
        exp_all, kk_all = base, list(kl)
        for i, k in zip(where, bigs):
            kk = list(kl)
            kk[i] = kk_all[i] = k
            exp_all = replaced(exp_all, pl, kl, i, k=k)
            d_s = dev(R.encode_scalars(kk))
            with util.edwards_only(aff, products=7):
                assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(replaced(base, pl, kl, i, k=k)), (i, hex(k))
        d_s = dev(R.encode_scalars(kk_all))
        with util.edwards_only(aff, products=7):
            assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(exp_all)
    finally:
        aff.set_narrow_max()


# ---- c. cancellation and skew ----
def test_cancellation_and_skew(aff, oracle, pool):
    """P and -P with one shared scalar (every bucket cancels to the identity), one scalar for all points (split rows
    and merges of affine additions) on both geometries, and three scalar values over 65537 points."""
    pl = R.decode_points(pool[: 96 * 2048])
    pm = []
    for p in pl:
        pm += [p, R.neg(p)]
    k = R.rand_scalars(0xC0, 1)[0]
    with util.edwards_only(aff, products=7):
        assert device_msm(aff, R.encode_points(pm), R.encode_scalars([k] * len(pm))) == R.encode_result(None)
    for n in (65, 2049, 70001):
        pts = pool[: 96 * n]
        ks = R.encode_scalars([R.rand_scalars(0xC1 + n, 1)[0]] * n)
        with util.edwards_only(aff, products=7):
            assert device_msm(aff, pts, ks) == util.oracle_msm(oracle, pts, ks), n
    n = 65537
    vals = R.rand_scalars(0xC3, 3)
    pts = pool[: 96 * n]
    ks = R.encode_scalars([vals[i % 3] for i in range(n)])
    with util.edwards_only(aff, products=7):
        assert device_msm(aff, pts, ks) == util.oracle_msm(oracle, pts, ks)


# ---- d. exceptional inputs ----
def test_every_check_of_the_edwards_law_fires_on_affine_records(aff):
    """The placements of test_every_check_of_the_edwards_law_fires (bucket chain, merge, tree levels, host tail) with
    msm_device and the window partials on affine records."""
    check_edwards_law_placements(aff)


def test_unrepresentable_point_at_the_block_edges(aff, oracle, pool):
    """(-1, 0) at the first point, both sides of the first block edge and the last point of the partial block: the
    conversion flags it inside the hooked flow, the call reruns exactly once (FB_CONVERT) and the result is exact; the
    next clean call on the same context shows that the conversion's error word was cleared."""
    n = 4100
    pts = pool[: 96 * n]
    kl = R.rand_scalars(0xD0, n)
    ks = R.encode_scalars(kl)
    pl = R.decode_points(pts)
    plain = util.oracle_msm(oracle, pts, ks)
    base = R.decode_result(plain)
    d_s = dev(ks)
    for i in (0, AFF_BLOCK_POINTS - 1, AFF_BLOCK_POINTS, n - 1):
        bad = bytearray(pts)
        bad[96 * i : 96 * i + 96] = R.encode_points([T2])
        d_p = dev(bytes(bad))
        before, _ = aff.fallback_info()
        assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(replaced(base, pl, kl, i, pt=T2)), i
        count, mask = aff.fallback_info()
        assert count == before + 1 and mask & FB_CONVERT, (i, count - before, mask)
    d_p = dev(pts)
    with util.edwards_only(aff, products=7):
        assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == plain


# ---- e. stage parity ----
def test_stage_parity_of_the_affine_kernel(aff, oracle):
    """k_accumulate on affine records, bucket by bucket against the oracle's SMVP: with 5000 points most buckets hold
    zero or one point, so this reads individual records that k_affine_down wrote."""
    import ctypes

    import numpy as np

    n = 5000
    pts, ks = seeded_inputs(oracle, n, 4343)
    aff.set_stage_capture(True)
    try:
        with util.edwards_only(aff, products=7):
            assert device_msm(aff, pts, ks) == util.oracle_msm(oracle, pts, ks)
        assert aff.stage_form() == 1
        for slot in (0, 9, 15):
            bk = aff.read_stage(slot, n, want=("buckets",))["buckets"]
            bo = ctypes.create_string_buffer(96 * 32768)
            assert oracle.oracle_g1_smvp_window(pts, ks, n, 16, slot, ctypes.addressof(bo)) == 0
            nonempty = 0
            for t in range(1, 32769):
                exp = bo.raw[96 * (t % 32768) : 96 * (t % 32768) + 96]
                words = bk[t - 1]
                if not words[0:13].any() and np.array_equal(words[13:26], words[39:52]):  # (0 : c : 0 : c): the identity
                    assert exp == R.encode_result(None), (slot, t)
                    continue
                nonempty += 1
                if nonempty <= 300:
                    assert R.encode_result(util.affine_from_te_ext_words(words)) == exp, (slot, t)
            assert nonempty > (1000 if slot < 15 else 500)
    finally:
        aff.set_stage_capture(False)


# ---- f. timing and state ----
def test_timing_modes_around_the_conversion(aff, oracle, pool):
    """Stage timing records events on the side stream inside the conversion: every mode, results exact."""
    for n in (3000, 70001):
        pts = pool[: 96 * n]
        ks = R.encode_scalars(R.rand_scalars(0xF0 + n, n))
        exp = util.oracle_msm(oracle, pts, ks)
        d_p, d_s = dev(pts), dev(ks)
        try:
            for timing in (False, 2, True, False):
                aff.set_timing(timing)
                with util.edwards_only(aff, products=7):
                    assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp, (n, timing)
                st = aff.stage_ms()
                if timing:
                    assert st["accumulate_kernel"] > 0.0, (n, timing)
                    assert (st["reduce"] > 0.0) == (timing is True), (n, timing)
        finally:
            aff.set_timing(False)


def test_one_context_alternating_entry_points(aff, oracle, pool):
    """msm_device at different sizes, a resident table with fixed-base calls and host-buffer calls in turn on one
    context: none of them may see state another one left behind (the affine records live in the same d_bases)."""
    sets = {}
    for n in (5000, 300, 70001, 2049):
        pts = pool[: 96 * n]
        ks = R.encode_scalars(R.rand_scalars(0xE0 + n, n))
        sets[n] = (pts, ks, util.oracle_msm(oracle, pts, ks))
    with util.edwards_only(aff):
        for n in (5000, 300, 70001, 2049, 5000):
            pts, ks, exp = sets[n]
            assert device_msm(aff, pts, ks) == exp, n
            assert aff.accumulate_products() == 7
            other = 300 if n != 300 else 2049
            aff.set_bases(sets[other][0])
            assert aff.msm_fixed_base(sets[other][1]) == sets[other][2], (n, other)
            assert aff.msm(pts, ks) == exp, n


def test_the_gate_itself(oracle, pool):
    """MSM377_AFFINE_MIN=3000: 2999 points take projective records (8 products), 3000 affine ones (7)."""
    with affine_engine(3000, 1 << 13) as eng:
        for n, products in ((2999, 8), (3000, 7), (2999, 8)):
            pts = pool[: 96 * n]
            ks = R.encode_scalars(R.rand_scalars(0x3000 + n, n))
            with util.edwards_only(eng, products=products):
                assert device_msm(eng, pts, ks) == util.oracle_msm(oracle, pts, ks), n


# ---- g. window partials on the affine gate ----
@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_window_partials_on_affine_records(aff, oracle, pool, world):
    n = 6000
    pts = pool[: 96 * n]
    ks = R.encode_scalars(R.rand_scalars(0x6000 + world, n))
    d_p, d_s = dev(pts), dev(ks)
    parts = []
    for r in range(world):
        b, c = msm.windows_for_rank(r, world)
        with util.edwards_only(aff, products=7):
            parts.append(aff.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, b, c))
        assert all(parts[-1][WINDOW_PARTIAL_BYTES * w + 47] >> 7 for w in range(c)), r  # tagged: Edwards records
    exp = util.oracle_msm(oracle, pts, ks)
    assert msm.combine_partials(b"".join(parts)) == exp == aff.combine_partials(b"".join(parts))


def test_resident_window_partials_on_affine_records(aff, oracle, pool):
    import torch

    n, world = 6000, 2
    pts = pool[: 96 * n]
    ks = R.encode_scalars(R.rand_scalars(0x6100, n))
    d_p, d_s = dev(pts), dev(ks)
    gathered = torch.zeros(16 * WINDOW_PARTIAL_BYTES, dtype=torch.uint8, device="cuda")
    off = 0
    for r in range(world):
        b, c = msm.windows_for_rank(r, world)
        with util.edwards_only(aff, products=7):
            aff.window_partials_resident(d_p.data_ptr(), d_s.data_ptr(), n, b, c, gathered.data_ptr() + off)
        off += c * WINDOW_PARTIAL_BYTES
    rec = gathered.cpu().numpy().tobytes()
    assert aff.combine_partials(rec) == util.oracle_msm(oracle, pts, ks) == msm.combine_partials(rec)


def signed_digit16(k, w):
    """Digit of window w in the signed recoding of k into sixteen 16-bit windows (digits in [-2^15, 2^15))."""
    carry = 0
    for x in range(w + 1):
        v = ((k >> (16 * x)) & 0xFFFF) + carry
        carry = 1 if v >= 32768 else 0
    return v - 65536 * carry


def test_window_partials_with_an_exceptional_pair_in_one_rank(aff, oracle, pool):
    """P and P + T' (util.t_prime) share a bucket in window 9 only: rank 1 of 2 (windows 8..15) reruns on the Weierstrass
    path alone, exactly once; rank 0 stays on affine records; the mixed records combine to the exact sum."""
    n = 6000
    pts = pool[: 96 * n]
    kl = R.rand_scalars(0x6200, n)
    pl = R.decode_points(pts)
    base = R.decode_result(util.oracle_msm(oracle, pts, R.encode_scalars(kl)))
    p = R.mul(R.G, 31337)
    q = R.add(p, util.t_prime())
    i, j = 17, n - 5
    # a bucket of window 9 that no other point reaches, so that P and P + T' are added to each other directly
    used = {abs(signed_digit16(k, 9)) for x, k in enumerate(kl) if x not in (i, j)}
    d = next(b for b in range(5, 32768) if b not in used)
    exp = replaced(base, pl, kl, i, pt=p, k=d << 144)
    kl2 = list(kl)
    kl2[i] = d << 144
    pl2 = list(pl)
    pl2[i] = p
    exp = replaced(exp, pl2, kl2, j, pt=q, k=d << 144)
    kl2[j] = d << 144
    pl2[j] = q
    d_p, d_s = dev(R.encode_points(pl2)), dev(R.encode_scalars(kl2))
    with util.edwards_only(aff, products=7):
        r0 = aff.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 0, 8)
    before, _ = aff.fallback_info()
    r1 = aff.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 8, 8)
    assert aff.fallback_info()[0] == before + 1
    assert r0[47] >> 7 == 1 and r1[47] >> 7 == 0  # rank 0: Edwards records; rank 1: Weierstrass ones after its rerun
    assert msm.combine_partials(r0 + r1) == R.encode_result(exp) == aff.combine_partials(r0 + r1)


# ---- h. short scalars on per-call affine records ----
SHORT_N, SHORT_BITS = 2049, 64  # two workgroups of the conversion; 64-bit scalars in 8 bytes


@pytest.fixture(scope="module")
def short_case(oracle, pool):
    pts = pool[: 96 * SHORT_N]
    kl = [k & ((1 << SHORT_BITS) - 1) for k in R.rand_scalars(0x5409, SHORT_N)]
    kl[0], kl[SHORT_N - 1] = (1 << SHORT_BITS) - 1, 1 << (SHORT_BITS - 1)
    kl[AFF_BLOCK_POINTS] |= 1  # (an odd multiple of a two-torsion point is the point itself)
    return pts, kl, util.oracle_msm(oracle, pts, R.encode_scalars(kl))


@pytest.mark.parametrize("geometry, log", [("narrow", 11), ("main", 15)])
def test_short_scalars_on_affine_records(aff, short_case, geometry, log):
    """msm_short_device (the conversion's way up now, the rest from the hook) and msm_short (host buffers: both phases
    back to back from the hook) on affine records, on 2^11 and on 2^15 buckets: the oracle's sum, the 7-product kernel,
    the short geometry, no rerun."""
    pts, kl, exp = short_case
    ks = msm.encode_scalars(kl, 8)
    d_p, d_s = dev(pts), dev(ks)
    aff.set_narrow_max(1 << 16 if geometry == "narrow" else 0)
    try:
        for call in (lambda: aff.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), SHORT_N, 8, SHORT_BITS), lambda: aff.msm_short(pts, ks, 8, SHORT_BITS)):
            with util.edwards_only(aff, products=7):
                assert call() == exp, geometry
            assert aff.accumulate_products() == 7
            assert aff.last_geometry() == (msm.short_windows(SHORT_BITS, log), log), geometry
    finally:
        aff.set_narrow_max()


def test_short_host_call_with_a_two_torsion_point(aff, short_case):
    """(-1, 0) among the points of a short host-buffer call: the conversion inside the hook flags it, the call reruns
    exactly once on the Weierstrass path (W windows of 2^15 buckets) and answers pyref's sum."""
    pts, kl, exp = short_case
    i = AFF_BLOCK_POINTS  # the one point of the second workgroup
    bad = bytearray(pts)
    bad[96 * i : 96 * i + 96] = R.encode_points([T2])
    want = R.encode_result(replaced(R.decode_result(exp), R.decode_points(pts), kl, i, pt=T2))
    before, _ = aff.fallback_info()
    assert aff.msm_short(bytes(bad), msm.encode_scalars(kl, 8), 8, SHORT_BITS) == want
    count, mask = aff.fallback_info()
    assert count == before + 1 and mask & FB_CONVERT, (count - before, mask)
    assert aff.last_geometry() == (msm.short_windows(SHORT_BITS, 15), 15)


# ---- i. full size on the session engine, default knobs ----
A0, D = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA
N_FULL = 1 << 20


@pytest.fixture(scope="module")
def full_points(oracle):
    """[A0 + i D]G for i < 2^20 on the device, and the host bytes."""
    pts = util.oracle_gen_points(oracle, N_FULL, A0, D)
    return pts, dev(pts)


def full_total(kl):
    return sum(k * (A0 + i * D) for i, k in enumerate(kl)) % R.R_ORDER


def test_full_size_skewed_and_big_scalars(engine, oracle, full_points):
    """msm_device at 2^20 on the default knobs with three scalar values, one repeated scalar, and uniform scalars with
    four of 2^253 and more at the block edges; each on affine records without a rerun."""
    import bench

    _, d_p = full_points
    n = N_FULL
    vals = R.rand_scalars(0x3A1, 3)
    uni = R.decode_scalars(bench.seeded_scalars(0x5CA1A5 + 20, n))
    big = list(uni)
    for i, k in zip((0, AFF_BLOCK_POINTS - 1, AFF_BLOCK_POINTS, n - 1), ((1 << 253) + 1, (1 << 254) + 7, 1 << 253, (1 << 255) - (1 << 239) - (1 << 224))):
        big[i] = k
    cases = {
        "three values": [vals[i % 3] for i in range(n)],
        "one scalar": [vals[0]] * n,
        "big scalars": big,
    }
    for name, kl in cases.items():
        d_s = dev(R.encode_scalars(kl))
        with util.edwards_only(engine, products=7):
            assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == util.closed_form(oracle, full_total(kl)), name


def test_full_size_unrepresentable_last_point(engine, oracle, full_points):
    """(-1, 0) as the last of 2^20 points: one rerun (FB_CONVERT), exact result."""
    import bench

    pts, _ = full_points
    n = N_FULL
    kl = R.decode_scalars(bench.seeded_scalars(0x5CA1A5 + 21, n))
    d_p = dev(pts[: 96 * (n - 1)] + R.encode_points([T2]))
    d_s = dev(R.encode_scalars(kl))
    exp = R.add(R.mul(R.G, (full_total(kl[: n - 1]))), R.mul(T2, kl[n - 1]))
    before, _ = engine.fallback_info()
    assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == R.encode_result(exp)
    count, mask = engine.fallback_info()
    assert count == before + 1 and mask & FB_CONVERT, (count - before, mask)


def test_full_size_window_partials_gate(engine, oracle, full_points):
    """window_partials at 2^20 under the default gate (n >= 2^18 and windows x n >= 2^24): all 16 windows in one call
    take affine records (7 products), a rank of two (8 windows, 2^23 pairs) keeps projective ones (8)."""
    import bench

    _, d_p = full_points
    n = N_FULL
    ks = bench.seeded_scalars(0x5CA1A5 + 23, n)
    d_s = dev(ks)
    exp = util.closed_form(oracle, full_total(R.decode_scalars(ks)))
    with util.edwards_only(engine, products=7):
        rec = engine.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 0, 16)
    assert engine.combine_partials(rec) == exp
    parts = []
    for r in range(2):
        with util.edwards_only(engine, products=8):
            parts.append(engine.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, *msm.windows_for_rank(r, 2)))
    assert engine.combine_partials(b"".join(parts)) == exp
