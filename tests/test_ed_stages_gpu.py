"""Stage read-backs of Edwards-BLS12 calls (msm377_ed_msm[_device], capture mode 2, msm377_g1_read_stage_ex with records of
form MSM377_STAGE_FORM_ED): digits, CSR rows and bucket records of k_decompose, the sort, k_accumulate<EdDev>,
k_merge_split_rows_quad<EdDev> against tests/stage_model.py over pyref.ed_add (pinned by tests/test_stage_model_host.py) and
against the stored-record contract of tools/check_lazy_bounds.py under use_field("Fq").  The checks are run_case /
check_slot of tests/test_stage_geometries_gpu.py, which are generic over the limb count and the coordinate shapes; every
case runs a call of the same size with other scalars first on the same context.  tests/STAGES.md maps the EdDev kernel arms
to these tests and lists the seeded faults they were shown to catch."""
import pytest

import ed_curve_points as V
import pyref as R
import stage_model as M
import util
import webgpu_msm_bls12_377_amd as msm
from test_g1_parity_gpu import dev
from test_stage_geometries_gpu import FORM_ED, fits, run_case, three, wire_points

pytestmark = pytest.mark.gpu

# csrc/kernels/accumulate.hpp LONG_ROW_PARTIALS = 32 overflow partials and csrc/common.hpp SEG_MIN = 16 entries per work item
# (auto_seg at these sizes): a row of more than 32 * 16 = 512 entries is one k_fold_long_rows would fold.  No Edwards-BLS12
# call launches that kernel (it follows short-scalar calls only, which this curve refuses), so such a row goes through
# k_merge_split_rows_quad<EdDev> with all of its partials: 600 entries, 38 work items, 37 partials.
LONG_ROW_PARTIALS, SEG_MIN = 32, 16
LONG_ROW = 600
assert LONG_ROW > LONG_ROW_PARTIALS * SEG_MIN


POOL_A0, POOL_D = 0xED57A6E5, 0xD15717C7


@pytest.fixture(scope="module")
def pool(oracle):
    """5000 points of the prime-order subgroup, P_i = [POOL_A0 + i POOL_D]G, shared by every case (prefixes of it)."""
    return util.oracle_ed_gen_points(oracle, 5000, POOL_A0, POOL_D)


def host_call(engine, pts):
    return lambda ks: engine.ed_msm(pts, R.encode_scalars(ks))


def device_call(engine, pts):
    d_p = dev(pts)

    def call(ks):
        d_s = dev(R.encode_scalars(ks))
        return engine.ed_msm_device(d_p.data_ptr(), d_s.data_ptr(), len(ks))

    return call


def expected_over_pool(pts, ks):
    """The expected result over a prefix of the pool: pyref.ed_msm_naive up to 20 points, and its closed form over the
    progression beyond that (ed_curve_points.progression_msm: one multiplication instead of 20 ms per point)."""
    if len(ks) <= 20:
        return R.ed_encode_result(R.ed_msm_naive(wire_points(pts, FORM_ED), ks))
    return R.ed_encode_result(V.progression_msm(POOL_A0, POOL_D, ks))


@pytest.mark.parametrize("buffers", ["device", "host"])
def test_even_geometry(engine, oracle, pool, buffers):
    """k_decompose even mode under an Edwards-BLS12 call, the two-level sort, k_accumulate<EdDev>, the 48-word record store."""
    g = M.even16()
    n = 5000
    ks, other = V.uniform_scalars(n, 1), V.uniform_scalars(n, 2)
    call = device_call(engine, pool) if buffers == "device" else host_call(engine, pool)
    run_case(engine, call, g, ks, pool, FORM_ED, three(g), other, util.oracle_ed_msm(oracle, pool, R.encode_scalars(ks)), label="ed even, %s buffers" % buffers)
    assert engine.accumulate_products() == 7


def test_even_geometry_edge_scalars(engine, pool):
    g = M.even16()
    ek = fits(g, V.even_edge_scalars())
    assert len(ek) == 13  # the other four rerun: all-ones top windows with a carry into them (twice), 2^253, 2^254 + 5
    pts = pool[: 64 * len(ek)]
    other = V.uniform_scalars(len(ek), 3)
    run_case(engine, host_call(engine, pts), g, ek, pts, FORM_ED, range(16), other, expected_over_pool(pts, ek), small=range(16), label="ed even edge scalars")


@pytest.mark.parametrize("n", [1, 257])
def test_smallest_inputs(engine, pool, n):
    """An Edwards-BLS12 call has no narrow path: one point runs sixteen windows of 2^15 buckets like any other input."""
    g = M.even16()
    pts = pool[: 64 * n]
    ks, other = V.uniform_scalars(n, 4), V.uniform_scalars(n, 5)
    run_case(engine, device_call(engine, pts), g, ks, pts, FORM_ED, range(16), other, expected_over_pool(pts, ks), small=range(16), label="ed n=%d" % n)


def test_a_scalar_that_does_not_fit_reruns_on_equal_windows(engine, pool):
    """One scalar of 2^253 and more among 500: exactly one rerun, the read-back describes the pass on sixteen equal windows,
    and the key_max word of its tracked top window is the model's bit for bit."""
    n = 500
    pts = pool[: 64 * n]
    ks, other = V.uniform_scalars(n, 6), V.uniform_scalars(n, 7)
    ks[77] = (1 << 253) + 99
    other[5] = (1 << 253) - (1 << 238) + (1 << 237) + 12345
    assert M.recode(ks[77], M.even16()).flags == M.ERR_RERUN and M.recode(ks[77], M.equal16()).flags == 0
    run_case(engine, host_call(engine, pts), M.equal16(), ks, pts, FORM_ED, [0, 15], other, expected_over_pool(pts, ks), small=(0, 15), reruns=1, label="ed rerun")


def test_equal_windows_with_a_tracked_top_window(oracle, pool):
    """MSM377_EVEN_WINDOWS=0.  The call before covers 16384 keys of window 15 (scalars up to 2^253 + r), the call under test
    8192 (scalars below r): the words above its covered keys are the rp_w[idx] = total fill of k_local_sort_lds, and all
    2^15 + 2 row_ptr words of the slot are compared."""
    g = M.equal16()
    n = 5000
    ks, other = R.rand_scalars(0xED3E12, n), [k + ((i & 1) << 253) for i, k in enumerate(R.rand_scalars(0xED3E13, n))]
    cols, _ = M.digit_matrix(ks, g)
    top = M.key_max_word(cols[15], 1 << 15, False) & 0xFFFF
    assert (1 << 12) <= top < (1 << 14) and (1 << 13) <= max(k >> 240 for k in other) < (1 << 14)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_EVEN_WINDOWS", "0")
        eng = msm.MsmEngine(1 << 13)
    try:
        run_case(eng, host_call(eng, pool), g, ks, pool, FORM_ED, three(g), other, util.oracle_ed_msm(oracle, pool, R.encode_scalars(ks)), label="ed equal windows")
    finally:
        eng.close()


def test_long_rows(engine, pool):
    """5 distinct scalars over 3000 points: rows of ~600 entries, ~38 work items each, k_merge_split_rows_quad<EdDev>.  At
    most 5 buckets per slot are non-empty: all are decoded."""
    g = M.even16()
    n = 3000
    pts = pool[: 64 * n]
    ks, other = V.few_distinct_scalars(n, 5, 8), V.few_distinct_scalars(n, 5, 9)
    run_case(engine, device_call(engine, pts), g, ks, pts, FORM_ED, three(g), other, expected_over_pool(pts, ks), small=range(16), label="ed long rows")


def test_one_row_past_the_fold_length(engine, pool):
    """One row of LONG_ROW entries in every slot among 500 uniform scalars: more partials than LONG_ROW_PARTIALS, merged one
    after the other (see LONG_ROW above).  Every non-empty bucket of the slots read is decoded."""
    g = M.even16()
    n = LONG_ROW + 500
    pts = pool[: 64 * n]
    ks, other = V.one_long_row_scalars(n, LONG_ROW, 10), V.one_long_row_scalars(n, LONG_ROW, 11)
    cols, _ = M.digit_matrix(ks, g)
    for slot in three(g):
        s = g.slots[slot]
        assert M.csr(cols[slot], 15, s.bias).counts[1:].max() >= LONG_ROW
    run_case(engine, host_call(engine, pts), g, ks, pts, FORM_ED, three(g), other, expected_over_pool(pts, ks), small=range(16), label="ed one long row")


def test_every_curve_point(engine):
    """Subgroup points mixed with the identity, (0, -1), both points of order 4 and P + T for each: at the first and last
    lane of a wave and of a 256-thread block, alone in a row, with their own negative, in rows that add up to the identity or
    to a low-order point, under the scalars 0 .. 4 and full-width ones (tests/ed_curve_points.py)."""
    g = M.even16()
    n = 600
    points, ks, planted, expected = V.every_curve_point(n, 1)
    assert len(planted) >= 80 and {0, 63, 64, 255, 256, 511, 512, n - 1} <= set(planted)
    pts = R.ed_encode_points(points)
    other = V.uniform_scalars(n, 12)
    run_case(engine, device_call(engine, pts), g, ks, pts, FORM_ED, range(16), other, R.ed_encode_result(expected), small=range(16),
             label="ed every curve point")


def test_which_calls_each_capture_mode_describes(oracle, pool, golden):
    """Mode 0 and mode 1 describe no Edwards-BLS12 call (MSM377_ESTATE from both read-backs, stage_form() -1); mode 2 does,
    and switches the chunked upload of msm377_ed_msm off as it does for G1 (MSM377_UPLOAD_CHUNK_MIN=100 here: without that
    the rows would be laid out per chunk and nothing would be describable); a G1 call on the same context reads as before."""
    from webgpu_msm_bls12_377_amd.host.engine import ESTATE

    n = 300
    pts = pool[: 64 * n]
    ks, other = V.uniform_scalars(n, 13), V.uniform_scalars(n, 14)
    exp = expected_over_pool(pts, ks)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_UPLOAD_CHUNK_MIN", "100")
        eng = msm.MsmEngine(1 << 12)

    def refuses(read):
        with pytest.raises(msm.MsmError) as e:
            read()
        assert e.value.code == ESTATE

    try:
        for mode in (0, 1):
            eng.set_stage_capture(mode)
            assert eng.ed_msm(pts, R.encode_scalars(ks)) == exp
            assert eng.last_geometry() == (16, 15) and eng.stage_form() == -1
            refuses(lambda: eng.read_stage_ex(0))
            refuses(lambda: eng.read_stage(0, n))
        run_case(eng, host_call(eng, pts), M.even16(), ks, pts, FORM_ED, [0, 15], other, exp, small=(0, 15), label="ed host buffers, chunk minimum 100")
        eng.set_stage_capture(2)
        assert eng.ed_msm(pts, R.encode_scalars(ks)) == exp
        info, st = eng.read_stage_ex(3, want=("buckets",))
        assert info.form == FORM_ED and st["buckets"].shape == (1 << 15, 36) and eng.stage_form() == -1
        refuses(lambda: eng.read_stage(0, n))
        refuses(lambda: eng.read_stage_ex(16))
        case = golden["g1_n1024_random"]
        assert eng.msm(case["points"], case["scalars"]) == case["expected"]
        info, st = eng.read_stage_ex(3, want=("buckets",))
        assert info.form == 1 and st["buckets"].shape == (1 << 11, 52) and eng.stage_form() == 1
        eng.set_stage_capture(0)
        assert eng.ed_msm(pts, R.encode_scalars(ks)) == exp
        refuses(lambda: eng.read_stage_ex(0))
    finally:
        eng.close()
