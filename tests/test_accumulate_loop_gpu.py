"""The accumulation loop and the Montgomery step on the GPU: k_accumulate forms an addition's operands, gathers the next
record into the registers the current one leaves and adds; the field products reduce biased columns with a three-
instruction step; is_bad tests one limb and runs the full comparison behind a branch.  None of it may change a limb.

  - device mul_lz / mul_add_mul_lz / sqr_lz / madd_affine against the host build (and, through
    tests/native/mont_step_host.cpp, against the earlier form of the step), word for word, on the corners of the
    operand shapes;
  - G1 MSMs through msm_device on affine records -- the kernel the benchmark runs -- against the CPU oracle, the bucket
    records against tests/stage_model.py: rows of 1..5 entries (the peeled first entry alone, first plus one, both
    parities behind it), a negated entry first, in the middle and last, rows split into several work items, n = 1 and
    n = 33; a chunked host-buffer call (later chunks continue from the buckets of earlier ones: `into`);
  - P, P + T' in one chain: MSM377_FB_ACCUMULATE is raised and the sum is exact."""
import numpy as np
import pytest

import lazy_model as LM
import pyref as R
import stage_model as SM
import util
import webgpu_msm_bls12_377_amd as msm
from test_g1_parity_gpu import dev
from test_mont_step_host import FieldCase, cross, load_lib, run
from test_stage_geometries_gpu import FORM_TE, run_case
from webgpu_msm_bls12_377_amd.host.engine import FB_ACCUMULATE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def one_hip_runtime():
    """The engine's loader brings torch's HIP runtime in before its own library (host/engine.py load_library); the test
    library of the primitives must not be the first to pull a runtime in, or torch finds no GPU afterwards."""
    msm.load_library()


@pytest.fixture(scope="module")
def aff():
    """msm_device on affine Edwards records at every size, 16-bit windows: k_accumulate<TeDev, 2, TeAffBase>."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_AFFINE_MIN", "1")
        eng = msm.MsmEngine(1 << 13)
    eng.set_narrow_max(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def pool(oracle):
    return util.oracle_gen_points(oracle, 4096, 0xACC0, 0x100F)


def device_call(eng, wire):
    d_p = dev(wire)

    def call(kk):
        d_s = dev(R.encode_scalars(kk))
        return eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(kk))

    return call


# ---- the products and the mixed addition, device against host ----
@pytest.mark.parametrize("field", ["Fp", "Fq"])
def test_device_products_equal_the_host_build_on_the_corners(field):
    lib, fc, fm = load_lib(), FieldCase(field), LM.FieldModel(field)
    devb, hostb = LM.device_backend(), LM.host_backend()
    cases = [("mul_lz", 0, cross([fc.extremes(a), fc.extremes(b)])) for a, b in fc.mul_pairs[2:]]
    cases += [("sqr_lz", 1, [np.array(fc.extremes("wide"), dtype=np.uint32)])]
    cases += [("mul_add_mul_lz", 2, cross([fc.extremes(s)[:6] for s in fc.mam_quads[-1]]))]
    for op, code, ops in cases:
        ops = [np.ascontiguousarray(x) for x in ops]
        while len(ops) < 4:
            ops.append(ops[0])
        assert 100 <= len(ops[0]) <= 2000 or op == "sqr_lz"
        reference = run(lib, fc, code, ops, want_out=True)  # host build, asserted equal to the earlier form of the step
        got = devb.field(fm, op, ops)
        assert np.array_equal(got, reference), (field, op, "device differs from the host build")
        assert np.array_equal(hostb.field(fm, op, ops), reference), (field, op)


@pytest.mark.parametrize("field", ["Fp", "Fq"])
def test_device_madd_affine_equals_the_host_build_on_the_corners(field):
    fm = LM.FieldModel(field)
    cm = LM.CurveModel(fm)
    devb, hostb = LM.device_backend(), LM.host_backend()
    for name in ("madd_affine", "madd"):
        p, q, neg = LM.te_poly_cases(cm, n_random=100)[name]
        out, flags = devb.te(fm, name, p, q, neg)
        hout, hflags = hostb.te(fm, name, p, q, neg)
        assert np.array_equal(out, hout) and np.array_equal(flags, hflags), (field, name)
        LM.check_te_poly_case(cm, name, (p, q, neg), out)
    rows, exp = LM.te_zero_cases(fm)  # is_bad's two stages: low limb 0 or MOD[0] with and without the rest matching
    _, flags = devb.te(fm, "is_zero", rows, np.zeros_like(rows), np.zeros(len(rows), dtype=np.uint32))
    assert flags.tolist() == exp


# ---- every path of the loop ----
def rows_case():
    """Window 0 holds rows of 1, 2, 3, 4 and 5 entries (digits 101..105), and seven rows of three entries (digits 201..207)
    with every pattern of negated entries (scalar 2^16 - d: digit -d, carry into window 1): the sort decides where in its
    row a negated entry ends up, so all seven patterns are there and the test reads back what it got."""
    ks = []
    for r in range(1, 6):
        ks += [100 + r] * r
    for pattern in range(1, 8):
        d = 200 + pattern
        ks += [(1 << 16) - d if (pattern >> i) & 1 else d for i in range(3)]
    return ks


def test_rows_of_one_to_five_entries_and_negated_entries_in_every_position(aff, pool):
    g = SM.even16()
    ks = rows_case()
    n = len(ks)
    pts = pool[: 96 * n]
    other = [k + 1000 for k in ks]
    exp = R.encode_result(R.msm_naive(R.decode_points(pts), ks))
    run_case(aff, device_call(aff, pts), g, ks, pts, FORM_TE, [0, 1], other, exp, small=[0, 1], label="rows 1..5")
    assert aff.accumulate_products() == 7
    # the premise: the rows have those lengths, and a negated entry is first / in the middle / last in its row
    aff.set_stage_capture(2)
    try:
        assert device_call(aff, pts)(ks) == exp
        st = aff.read_stage_ex(0, want=("row_ptr", "val_idx"))[1]
    finally:
        aff.set_stage_capture(0)
    rp, vi = st["row_ptr"], st["val_idx"]
    lens = np.diff(rp.astype(np.int64))[1:]  # row of key t + 1 at index t
    assert [int(lens[100 + r - 1]) for r in range(1, 6)] == [1, 2, 3, 4, 5]
    first, middle, last = set(), set(), set()  # rows (by their count of negated entries) with a negated entry there
    for pattern in range(1, 8):
        row = vi[rp[200 + pattern] : rp[200 + pattern + 1]] >> 31
        assert len(row) == 3 and int(row.sum()) == bin(pattern).count("1")
        for seen, at in ((first, 0), (middle, 1), (last, 2)):
            if row[at]:
                seen.add(int(row.sum()))
    # a negated entry opens a chain (the peeled first entry), sits in the middle, and closes one behind plain entries
    assert first and middle and last and min(last) < 3, (first, middle, last)


@pytest.mark.parametrize("n", [1, 33])
def test_smallest_inputs(aff, pool, n):
    pts = pool[: 96 * n]
    ks = R.rand_scalars(0xACC + n, n)
    ks = [k >> 3 for k in ks]  # below 2^253: the even geometry without a rerun
    exp = R.encode_result(R.msm_naive(R.decode_points(pts), ks))
    other = [k ^ 0x5555 for k in ks]
    run_case(aff, device_call(aff, pts), SM.even16(), ks, pts, FORM_TE, [0, 15], other, exp, small=[0, 15], label="n = %d" % n)
    assert aff.accumulate_products() == 7


def test_rows_split_into_several_work_items(aff, oracle, pool):
    """4096 points over five scalar values: every window holds a handful of rows of ~800 entries, each cut into work
    items whose partial sums k_merge_split_rows_quad adds back."""
    n = 4096
    vals = [k >> 3 for k in R.rand_scalars(0x5EED, 5)]
    ks = [vals[(i * i + i // 7) % 5] for i in range(n)]
    other = [vals[(i + 1) % 5] ^ 0x3333 for i in range(n)]
    exp = util.oracle_msm(oracle, pool, R.encode_scalars(ks))
    run_case(aff, device_call(aff, pool), SM.even16(), ks, pool, FORM_TE, [0, 7], other, exp, small=[0, 7], label="split rows")
    assert aff.accumulate_products() == 7


def test_chunked_call_continues_from_the_buckets(oracle, pool, monkeypatch):
    """Host buffers in chunks of points: chunks after the first start each row from the bucket the earlier chunks left
    (`into`), for rows of every length (uniform scalars) and for split rows (one scalar)."""
    monkeypatch.setenv("MSM377_UPLOAD_CHUNK_MIN", "100")
    eng = msm.MsmEngine(1 << 13)
    try:
        for n, ks in ((131, R.rand_scalars(0x1270, 131)), (4096, [R.rand_scalars(0x1271, 1)[0]] * 4096), (1000, rows_case() * 40)):
            pts, kb = pool[: 96 * n], R.encode_scalars(ks[:n])
            before, _ = eng.fallback_info()
            assert eng.msm(pts, kb) == util.oracle_msm(oracle, pts, kb), n
            assert eng.fallback_info()[0] == before, n
    finally:
        eng.close()


def test_exceptional_pair_in_a_chain_raises_the_flag_and_the_sum_is_exact(aff, pool):
    """P and P + T' (util.t_prime) share a row of the call (digit 5), four other points another (digit 9): in either
    order the row's one addition has Z3 = 0 -- is_bad's rare branch must be taken and must say yes -- and the call
    reruns on the Weierstrass path, exactly once, with the exact sum.  The pair in the middle of a longer chain is no
    exceptional pair for the partial sum it meets; that call must simply stay exact."""
    tp = util.t_prime()
    p = R.mul(R.G, 31337)
    q = R.add(p, tp)
    others = R.decode_points(pool[: 96 * 4])
    pts = [p, q] + others
    ks = [5, 5, 9, 9, 9, 9]
    exp = R.encode_result(R.msm_naive(pts, ks))
    d_p, d_s = dev(R.encode_points(pts)), dev(R.encode_scalars(ks))
    before, _ = aff.fallback_info()
    assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(ks)) == exp
    count, mask = aff.fallback_info()
    assert count == before + 1 and mask & FB_ACCUMULATE, (count - before, mask)
    # the same pair in the middle of a chain of six: (R1 + R2 + P) + (P + T') is no exceptional pair, the sum stays exact
    ks = [5] * 6
    pts = others[:2] + [p, q] + others[2:]
    d_p, d_s = dev(R.encode_points(pts)), dev(R.encode_scalars(ks))
    assert aff.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(ks)) == R.encode_result(R.msm_naive(pts, ks))
