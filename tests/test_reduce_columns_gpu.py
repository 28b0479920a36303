"""The bucket reduction's column launches (csrc/kernels/reduce.hpp k_tree_columns; MSM377_REDUCE_COLUMNS=1, the default)
against one launch per level (=0) on the same inputs.  The column kernel performs the same additions on the same operands
in the same order, so the two contexts must agree on the final point, which is also compared with the CPU oracle, and
word for word on every partial record (window_partials_device, raw bytes) wherever the buckets themselves are pinned by
the input (test_records_word_for_word says when they are).  The sizes are the smallest that reach each
geometry the stage serves: 2^12 (narrow path, 2^11 buckets, one column launch), 2^16 + 1 (main path, 2^15 buckets, two
column launches; about two entries per bucket, so both identity branches of the rule are taken, and whole waves of empty
buckets in the top one of sixteen equal windows), 2^17 on the Edwards-BLS12 curve, and a fixed-base call over the 20-bit
table (one window of 2^19 buckets, three column launches).  The plan itself: tests/test_reduce_columns_host.py."""
import random

import pytest

import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm

pytestmark = pytest.mark.gpu

SETTINGS = (0, 1)
N_NARROW, N_MAIN, N_ED = 1 << 12, (1 << 16) + 1, 1 << 17


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def engines():
    """One context per setting; the variable is read when a context is created."""
    engs = {}
    for s in SETTINGS:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("MSM377_REDUCE_COLUMNS", str(s))
            engs[s] = msm.MsmEngine(N_ED)
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def pool(oracle):
    """2^16 + 1 subgroup points; the smaller cases take a prefix."""
    return util.oracle_gen_points(oracle, N_MAIN, 0xC01A11, 0x5EED5)


def all_windows(e, d_p, d_s, n):
    return e.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 0, 16)


def test_narrow_path(engines, oracle, pool):
    n = N_NARROW
    pts, ks = pool[: 96 * n], R.encode_scalars(R.rand_scalars(0xC0112, n))
    exp = util.oracle_msm(oracle, pts, ks)
    d_p, d_s = dev(pts), dev(ks)
    for s in SETTINGS:
        e = engines[s]
        with util.edwards_only(e):
            assert e.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp, s
            assert e.last_geometry() == (22, 11), s
            assert e.msm(pts, ks) == exp, s
        # the same points on the sixteen 2^15-bucket windows: seven buckets of eight are empty
        assert msm.combine_partials(all_windows(e, d_p, d_s, n)) == exp, s


def test_main_path(engines, oracle, pool):
    n = N_MAIN
    pts, ks = pool, R.encode_scalars(R.rand_scalars(0xC0116, n))
    exp = util.oracle_msm(oracle, pts, ks)
    d_p, d_s = dev(pts), dev(ks)
    for s in SETTINGS:
        e = engines[s]
        with util.edwards_only(e):
            assert e.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp, s
            assert e.last_geometry() == (16, 15), s
            assert msm.combine_partials(all_windows(e, d_p, d_s, n)) == exp, s  # sixteen equal windows: the top one mostly empty


def one_point_per_bucket(n_pool):
    """Scalars whose sixteen 16-bit limbs are all below 2^15 (no carries, no negative digits) and, window by window, all
    different: limb w of scalar i is (i odd_w mod 2^15), a bijection, so every bucket of every window receives at most
    one point and its content does not depend on the order in which the sort hands a row's entries out.  (Records are
    NOT reproducible from call to call once two points share a bucket: the order inside a row is free, and P1 + P2 and
    P2 + P1 are different projective triples of the same point.  So this is the input on which the reduction's output can be
    compared word for word at all.)  Three indices of eight are left out: empty buckets, in other places in every window.
    The top limb stays below 2^12 and is nonzero for the first 4096 indices only, which keeps the scalars below r and that
    window one point per bucket too."""
    rnd = random.Random(0xC0113)
    idx = [i for i in range(1, 1 << 15) if rnd.random() < 0.625]
    assert len(idx) <= n_pool
    ks = []
    for i in idx:
        k = 0
        for w in range(15):
            k |= ((i * (2 * w + 3)) & 0x7FFF) << (16 * w)
        if i < 4096:
            k |= ((i * 33) & 0xFFF) << 240
        ks.append(k)
    return ks


def test_records_word_for_word(engines, oracle, pool):
    """Every partial record k_gather_partials emits, raw bytes, column launches against one launch per level: all sixteen
    windows in one call (the per-level launches skip empty buckets up to level 5 and use lane quads, which add them like
    any other, at level 6), and a shard of two (lane quads from level 0 on: the records differ from the sixteen-window
    call's, and agree between the settings)."""
    ks = one_point_per_bucket(N_MAIN)
    n = len(ks)
    for w in range(16):
        limbs = [(k >> (16 * w)) & 0xFFFF for k in ks]
        assert max(limbs) < 1 << 15 and len(set(limbs) - {0}) == sum(1 for v in limbs if v), w
    pts, wire = pool[: 96 * n], R.encode_scalars(ks)
    exp = util.oracle_msm(oracle, pts, wire)
    d_p, d_s = dev(pts), dev(wire)
    rec, shard = {}, {}
    for s in SETTINGS:
        e = engines[s]
        with util.edwards_only(e):
            rec[s] = all_windows(e, d_p, d_s, n)
            assert all_windows(e, d_p, d_s, n) == rec[s], (s, "the input does not pin the records")
            shard[s] = e.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 14, 2)
        assert msm.combine_partials(rec[s]) == exp, s
        assert msm.combine_partials(rec[s][: 14 * len(rec[s]) // 16] + shard[s]) == exp, s
    assert rec[0] == rec[1]
    assert shard[0] == shard[1]


def test_edwards_bls12(engines, oracle):
    n = N_ED
    pts = util.oracle_ed_gen_points(oracle, n, 0xED5C01, 0x1357ACE)
    ks = R.encode_scalars(R.rand_scalars(0xEDC0, n, R.ED_SUBGROUP))
    exp = util.oracle_ed_msm(oracle, pts, ks)
    d_p, d_s = dev(pts), dev(ks)
    for s in SETTINGS:
        assert engines[s].ed_msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp, s


def test_fixed_base_wide_window(engines, oracle, pool):
    n = N_NARROW
    pts, ks = pool[: 96 * n], R.encode_scalars(R.rand_scalars(0xC0120, n))
    exp = util.oracle_msm(oracle, pts, ks)
    for s in SETTINGS:
        e = engines[s]
        e.set_precompute_window(20)
        try:
            e.set_bases_precomputed(pts)
            with util.edwards_only(e):
                assert e.msm_fixed_base(ks) == exp, s
            e.set_precompute_window(16)  # sixteen tables folded into one window of 2^15 buckets (wc_out = 1)
            e.set_bases_precomputed(pts)
            with util.edwards_only(e):
                assert e.msm_fixed_base(ks) == exp, s
        finally:
            e.set_precompute_window(16)


# bucket pairs (as scalars 1 + index) that meet in a column launch: level 0 and level 5 of the 2^15-bucket windows (first
# and second launch), level 0 of the narrow path's 2^11-bucket windows
EXCEPTIONAL = [("level 0", 1 + (1 << 14), 0), ("level 5", 1 + (1 << 9), 0), ("narrow, level 0", 1 + (1 << 10), None)]


@pytest.mark.parametrize("name,k1,narrow_max", EXCEPTIONAL, ids=[c[0] for c in EXCEPTIONAL])
def test_exceptional_addition_in_the_tree(engines, name, k1, narrow_max):
    """P and P + T' (util.t_prime: the exceptional pair of the a = -1 law, as in test_every_check_of_the_edwards_law_fires)
    in two buckets that a column launch adds: both settings raise the tree's flag, rerun on the Weierstrass path and
    return the exact sum; the records of the rerun agree too."""
    from webgpu_msm_bls12_377_amd.host.engine import FB_TREE

    p = R.mul(R.G, 31337)
    q = R.add(p, util.t_prime())
    pts, ks = [p, q], [1, k1]
    exp = R.encode_result(R.msm_naive(pts, ks))
    pb, sb = R.encode_points(pts), R.encode_scalars(ks)
    d_p, d_s = dev(pb), dev(sb)
    seen, rec = {}, {}
    for s in SETTINGS:
        e = engines[s]
        if narrow_max is not None:
            e.set_narrow_max(narrow_max)
        try:
            before, _ = e.fallback_info()
            assert e.msm(pb, sb) == exp, (name, s)
            count, mask = e.fallback_info()
            assert count == before + 1 and mask & FB_TREE, (name, s, count - before, mask)
            seen[s] = mask
            if narrow_max is not None:
                rec[s] = all_windows(e, d_p, d_s, 2)
                assert e.fallback_info()[0] == before + 2, (name, s)
                assert msm.combine_partials(rec[s]) == exp, (name, s)
        finally:
            e.set_narrow_max()
    assert seen[0] == seen[1], name
    assert rec.get(0) == rec.get(1), name
