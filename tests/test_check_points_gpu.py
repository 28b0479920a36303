"""Point validation on the GPU (msm377_*_check_points*, kernels/validate.hpp): the GPU report against the host
implementation and tests/pyref.py, the resident bases across a check, and the opt-in check of the set-bases calls.
An invalid point is ordinary data to these kernels; nothing here provokes a fault."""
import random

import pytest
import torch

import check_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from check_vectors import as_tuple, expected_report

pytestmark = pytest.mark.gpu


def dev(buf):
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def g1_set():
    return V.g1_crafted()


@pytest.fixture(scope="module")
def ed_set():
    return V.ed_crafted()


@pytest.mark.parametrize("flags", [1, 3, 7, 2, 4])
def test_g1_crafted_gpu_equals_host_equals_pyref(engine, g1_set, flags):
    blob, verdicts = g1_set
    want = expected_report(verdicts, flags)
    assert as_tuple(msm.check_points_host(blob, flags)) == want
    assert as_tuple(engine.check_points(blob, flags)) == want
    d = dev(blob)
    assert as_tuple(engine.check_points_device(d.data_ptr(), len(verdicts), flags)) == want


@pytest.mark.parametrize("flags", [1, 3, 7, 2, 4])
def test_ed_crafted_gpu_equals_host_equals_pyref(engine, ed_set, flags):
    blob, verdicts = ed_set
    want = expected_report(verdicts, flags)
    assert as_tuple(msm.ed_check_points_host(blob, flags)) == want
    assert as_tuple(engine.ed_check_points(blob, flags)) == want
    d = dev(blob)
    assert as_tuple(engine.ed_check_points_device(d.data_ptr(), len(verdicts), flags)) == want


def test_small_order_points_alone_and_in_a_crowd(engine):
    """Every point of order 2, 3, 4, 6 and every P + T: outside the subgroup, one per wave and all in one wave."""
    small = V.g1_small_order_points()
    pts = small + [R.add(R.mul(R.G, 500 + i), t) for i, t in enumerate(small)]
    for pt in pts:
        assert V.g1_verdict(*pt) == V.SUBGROUP
    blob = R.encode_points(pts)
    assert as_tuple(engine.check_points(blob, 7)) == (len(pts), 0, 0, len(pts), 0, V.SUBGROUP)
    for i, pt in enumerate(pts):
        assert as_tuple(engine.check_points(R.encode_points([R.G, pt]), 7)) == (2, 0, 0, 1, 1, V.SUBGROUP), i
    low = V.ed_low_order_points()
    ed = low + [R.ed_add(R.ED_G, t) for t in low]
    assert as_tuple(engine.ed_check_points(R.ed_encode_points(ed), 7)) == (len(ed), 0, 0, len(ed), 0, V.SUBGROUP)


def _planted(n, seed):
    """Indices (0 and n - 1 among them, a run inside one wave, one alone in the last partial wave) -> bad wire record."""
    gx, gy = R.G
    kinds = [
        ((R.P, gy), V.CANONICAL),
        ((gx, gy ^ 2), V.CURVE),
        ((R.P - 1, 0), V.SUBGROUP),
        (R.add(R.mul(R.G, 99), util.t_prime()), V.SUBGROUP),
        ((gx, 2**384 - 1), V.CANONICAL),
        ((1, 1), V.CURVE),
        ((0, 1), V.SUBGROUP),
    ]
    for pt, v in kinds:
        assert V.g1_verdict(*pt) == v  # pyref
    rng = random.Random(seed)
    idx = {0, n - 1}
    if n > 8:
        base = rng.randrange(0, max(1, n - 8)) & ~63 if n > 128 else 1
        idx |= {min(n - 1, base + k) for k in (1, 2, 3, 5)}  # several in one wave
        idx |= {rng.randrange(n) for _ in range(6)}
        if n % 64:
            idx.add(n - 1 - rng.randrange(n % 64))  # in the last partial wave
    return {i: kinds[(i + k) % len(kinds)] for k, i in enumerate(sorted(idx))}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099, 1 << 16])
def test_planted_points_counters_and_first_bad_exact(engine, n):
    d = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0xC4EC + n, n, d.data_ptr())  # multiples of the generator: valid
    clean = as_tuple(engine.check_points_device(d.data_ptr(), n, 7))
    assert clean == (n, 0, 0, 0, None, 0)
    plan = _planted(n, n)
    for i, (pt, _) in plan.items():
        d[96 * i : 96 * i + 96] = dev(R.encode_points([pt]))
    verdicts = [plan[i][1] if i in plan else 0 for i in range(n)]
    for flags in (7, 3, 1):
        want = expected_report(verdicts, flags)
        print("n=%d flags=%d want=%s" % (n, flags, want))
        assert as_tuple(engine.check_points_device(d.data_ptr(), n, flags)) == want
    if n <= 4099:  # the host implementation on the same bytes (a subgroup test is ~0.1 ms per point there)
        assert as_tuple(msm.check_points_host(bytes(d.cpu().numpy()), 7)) == expected_report(verdicts, 7)


def test_a_million_points(engine):
    n = 1 << 20
    d = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0x100000, n, d.data_ptr())
    assert as_tuple(engine.check_points_device(d.data_ptr(), n, 7)) == (n, 0, 0, 0, None, 0)
    gx, gy = R.G
    plan = {777_777: ((R.P + 3, gy), V.CANONICAL), 123_456: ((gx, gy ^ 4), V.CURVE), n - 1: (R.add(R.mul(R.G, 7), (R.P - 1, 0)), V.SUBGROUP)}
    for i, (pt, v) in plan.items():
        assert V.g1_verdict(*pt) == v
        d[96 * i : 96 * i + 96] = dev(R.encode_points([pt]))
    assert as_tuple(engine.check_points_device(d.data_ptr(), n, 7)) == (n, 1, 1, 1, 123_456, V.CURVE)


def test_a_check_leaves_the_resident_table_and_the_fallback_count_alone(engine, oracle):
    n = 3000
    pts = util.oracle_gen_points(oracle, n, 0x51DE, 0x77)
    ks = R.encode_scalars(R.rand_scalars(0x51DE, n))
    want = util.oracle_msm(oracle, pts, ks)
    bad = bytearray(pts)
    bad[96:192] = R.encode_points([(R.P - 1, 0)])
    for setter in (engine.set_bases_precomputed, engine.set_bases):
        setter(pts)
        before = engine.fallback_info()
        assert engine.check_points(pts, 7).ok  # the host-buffer upload must not land on the table's raw copy
        assert as_tuple(engine.check_points(bytes(bad), 7)) == (n, 0, 0, 1, 1, V.SUBGROUP)
        d = dev(bad)
        assert as_tuple(engine.check_points_device(d.data_ptr(), n, 3)) == (n, 0, 0, 0, None, 0)
        assert engine.ed_check_points(R.ed_encode_points([R.ED_G] * 100), 7).ok
        assert engine.fallback_info() == before
        assert engine.msm_fixed_base(ks) == want


def test_argument_errors(engine):
    d = dev(R.encode_points([R.G] * 4))
    for call in (
        lambda: engine.check_points_device(d.data_ptr(), 4, 0),
        lambda: engine.check_points_device(d.data_ptr(), 4, 8),
        lambda: engine.check_points_device(d.data_ptr() + 4, 4, 7),
        lambda: engine.check_points_device(0, 4, 7),
        lambda: engine.check_points_device(d.data_ptr(), engine.max_points + 1, 7),
        lambda: engine.ed_check_points_device(d.data_ptr(), 4, 16),
        lambda: engine.check_points(b"", 0),
    ):
        with pytest.raises(msm.MsmError) as e:
            call()
        assert e.value.code == -1
    assert as_tuple(engine.check_points_device(0, 0, 7)) == (0, 0, 0, 0, None, 0)
    assert as_tuple(engine.ed_check_points(b"", 1)) == (0, 0, 0, 0, None, 0)


def test_set_bases_opt_in_refuses_a_cofactor_point(engine, oracle):
    n = 2048
    pts = util.oracle_gen_points(oracle, n, 0xBA5E, 0x31)
    ks = R.encode_scalars(R.rand_scalars(0xBA5E, n))
    where = 1234
    bad = bytearray(pts)
    bad[96 * where : 96 * where + 96] = R.encode_points([R.add(R.mul(R.G, 5), util.t_prime())])
    bad = bytes(bad)
    try:
        engine.set_base_checks(7)
        for setter in (engine.set_bases, engine.set_bases_precomputed, lambda b: engine.set_bases_device(dev(b).data_ptr(), n)):
            engine.set_bases(pts)  # a valid set passes, and is resident
            assert engine.last_check().ok and engine.last_check().checked == n
            assert engine.msm_fixed_base(ks) == util.oracle_msm(oracle, pts, ks)
            with pytest.raises(msm.MsmError) as e:
                setter(bad)
            assert e.value.code == -8 and str(where) in str(e.value)
            assert as_tuple(engine.last_check()) == (n, 0, 0, 1, where, V.SUBGROUP)
            with pytest.raises(msm.MsmError) as e:
                engine.msm_fixed_base(ks)
            assert e.value.code == -5  # MSM377_ESTATE: no resident bases after a refused set
        with pytest.raises(msm.MsmError) as e:
            engine.set_base_checks(8)
        assert e.value.code == -1
        engine.set_base_checks(0)
        engine.set_bases(bad)  # as today: converted without a look
        assert engine.msm_fixed_base(ks) == util.oracle_msm(oracle, bad, ks)
    finally:
        engine.set_base_checks(0)


def test_glv_promise_is_verified_by_the_opt_in(engine, oracle):
    n = 1024
    pts = util.oracle_gen_points(oracle, n, 0x61F, 0x13)
    ks = R.encode_scalars(R.rand_scalars(0x61F, n))
    bad = bytearray(pts)
    bad[96 * 17 : 96 * 18] = R.encode_points([R.add(R.mul(R.G, 3), (R.P - 1, 0))])
    try:
        engine.set_g1_form(0)
        engine.set_glv(1)
        engine.set_base_checks(7)
        with pytest.raises(msm.MsmError) as e:
            engine.set_bases(bytes(bad))
        assert e.value.code == -8
        assert engine.last_check().first_bad == 17
        engine.set_bases(pts)
        assert engine.msm_fixed_base(ks) == util.oracle_msm(oracle, pts, ks)
    finally:
        engine.set_base_checks(0)
        engine.set_glv(0)
        engine.set_g1_form(1)
