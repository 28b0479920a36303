"""Edwards-BLS12 variable-base batch multiplication on the GPU (include/msm377.h "Edwards-BLS12 variable-base batch
multiplication"; csrc/kernels/ed_batch_mul_var.hpp): out[i] = [s_i]P_i through msm377_ed_batch_mul_var_device /
msm377_ed_batch_mul_var.  Expected values: the host twin (which tests/test_ed_batch_mul_var_host.py pins to tests/pyref.py
and to the reference's vectors), pyref itself, and the model tests/ed_walk_var_model.py for the stash and the tables.  No
expected value comes from the device call.  Every test leaves the engine at (wire, wire)."""
import ctypes

import numpy as np
import pytest

import batch_mul_vectors as V
import ed_batch_mul_var_vectors as VV
import ed_curve_points as EP
import ed_walk_var_model as WVM
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import engine as E
from webgpu_msm_bls12_377_amd.host.engine import CHECK_CANONICAL, CHECK_CURVE, EINVAL, EPOINT, ESTATE

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
PASS = VV.PASS


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


def poisoned(nbytes, value=0xEE):
    import torch

    return torch.full((max(16, nbytes),), value, dtype=torch.uint8, device="cuda")


def run_device(engine, points: bytes, scalars: bytes, stride=32):
    """The records of one device call on a freshly poisoned (0xEE) output buffer."""
    n = len(points) // 64
    d_p, d_s, d_out = dev(points), dev(scalars), poisoned(64 * n)
    engine.ed_batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), stride)
    return bytes(d_out.cpu().numpy()[: 64 * n])


def code_of(call, *args):
    with pytest.raises(msm.MsmError) as err:
        call(*args)
    return err.value


# ---- GPU == host twin ----
@pytest.fixture(scope="module")
def cases():
    """n -> (point bytes, scalar bytes, the twin's records): every_curve_point with the edge scalars over LANES."""
    out = {}
    for n in SIZES:
        pb, sb = VV.encode(*VV.case(n))
        out[n] = (pb, sb, msm.ed_batch_mul_var_host(pb, sb))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin(engine, cases, n):
    pb, sb, wire = cases[n]
    assert run_device(engine, pb, sb) == wire


def test_probe_against_pyref(engine, cases):
    """The special classes and the edge scalars of the 257-point case by pyref itself, not through the twin."""
    points, scalars = VV.case(257)
    got = run_device(engine, *cases[257][:2])
    probe = [i for i in range(257) if i in EP.LANES or points[i][0] == 0 or points[i][1] == 0][:24] + list(range(1, 20))
    for i in probe:
        assert got[64 * i : 64 * i + 64] == R.ed_encode_result(R.ed_mul(points[i], scalars[i])), i


def test_host_buffer_call_equals_device_call(engine, cases):
    pb, sb, wire = cases[513]
    assert engine.ed_batch_mul_var(pb, sb) == wire
    assert engine.ed_batch_mul_var(b"", b"") == b""
    one = R.encode_scalars([VV.MASK256])
    assert engine.ed_batch_mul_var(pb, one) == msm.ed_batch_mul_var_host(pb, one)  # 32 bytes for 513 points: stride 0


def test_host_buffer_call_past_one_piece(engine):
    """n = 2^20 + 1: the host-buffer call works in pieces of 2^20 points, so its loop runs twice and the second piece is ONE
    point; a call of several pieces checks all of them before the first one runs.  Records equal the device call's on the
    same inputs byte for byte (the tests above pin the device call to the twin), on a poisoned buffer; a point off the curve
    in the SECOND piece is refused with its index in the whole array and nothing written, although the first piece is fine.
    One 40-bit scalar for all points: the walk skips its leading windows."""
    import torch

    n = (1 << 20) + 1
    d_p = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    engine.ed_generate_bases_device(0x9A5507, n, d_p.data_ptr())
    points = bytes(d_p.cpu().numpy())
    del d_p
    one = R.encode_scalars([0xD0E50F7AB1])
    lib = msm.load_library()
    out = ctypes.create_string_buffer(b"\xee" * (64 * n), 64 * n)
    assert lib.msm377_ed_batch_mul_var(engine._ctx, points, one, n, 0, ctypes.addressof(out)) == 0
    assert out.raw == run_device(engine, points, one, stride=0)
    bad = points[: 64 << 20] + R.ed_encode_points([VV.off_curve_point()])
    ctypes.memset(out, 0xA5, 64 * n)
    err = code_of(engine._check, lib.msm377_ed_batch_mul_var(engine._ctx, bad, one, n, 0, ctypes.addressof(out)), "msm377_ed_batch_mul_var")
    assert (err.code, err.index) == (EPOINT, 1 << 20)
    assert out.raw == b"\xa5" * (64 * n)


def test_zero_wave_beside_a_live_wave(engine, cases):
    """Waves 1 and 3 hold the zero scalar in every lane (skipped from the first window to the last), waves 0 and 2 full-width
    ones, wave 4 a single late riser."""
    n = 5 * 64
    pb = cases[513][0][: 64 * n]
    scalars = VV.random_scalars("zero wave", n)
    for i in list(range(64, 128)) + list(range(192, 256)) + list(range(256, n)):
        scalars[i] = 0
    scalars[256 + 17] = 0x1D
    sb = R.encode_scalars(scalars)
    wire = msm.ed_batch_mul_var_host(pb, sb)
    assert wire[64 * 64 : 64 * 128] == VV.IDENTITY_WIRE * 64
    assert run_device(engine, pb, sb) == wire


@pytest.mark.parametrize("scalar", [VV.random_scalars("broadcast", 1)[0] | 1 << 255, 0xD0E5_0F7A_B1 | 1 << 63, 0])
def test_one_scalar_for_all(engine, cases, scalar):
    """A full-width, a 64-bit and the zero scalar: stride 0 equals the per-point form byte for byte."""
    pb = cases[257][0]
    one = R.encode_scalars([scalar])
    exp = msm.ed_batch_mul_var_host(pb, one * 257)
    assert run_device(engine, pb, one * 257) == exp
    assert run_device(engine, pb, one, stride=0) == exp


def test_in_place(engine, cases):
    pb, sb, wire = cases[513]
    d_p, d_s = dev(pb), dev(sb)
    engine.ed_batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), 513, d_p.data_ptr())
    assert bytes(d_p.cpu().numpy()) == wire


def test_equals_the_fixed_base_call_on_copies_of_one_base(engine):
    base = R.ed_mul(R.ED_G, 0xD00E)
    scalars = VV.edge_scalars() + VV.random_scalars("fixed", 100)
    sb = R.encode_scalars(scalars)
    pb = R.ed_encode_points([base]) * len(scalars)
    assert run_device(engine, pb, sb) == engine.ed_batch_mul(R.ed_encode_points([base]), sb)


# ---- the pass boundary ----
@pytest.mark.parametrize("n", [PASS - 1, PASS, PASS + 1])
def test_pass_boundary(engine, oracle, n):
    """One pass, one full pass, two passes (the second of ONE point), against the one-thread twin."""
    pb, sb = VV.boundary_case(n, lambda m, a0, d: util.oracle_ed_gen_points(oracle, m, a0, d))
    got = run_device(engine, pb, sb)
    wire = msm.ed_batch_mul_var_host(pb, sb)
    assert got[-64 * 8 :] == wire[-64 * 8 :]
    assert got == wire
    info, _, _ = engine.read_walk_stash(info_only=True)
    assert (info.kind, info.n, info.pass_offset, info.m) == (E.WALK_ED_BATCH_MUL_VAR, n, PASS if n > PASS else 0, n - PASS if n > PASS else n)


# ---- refusals ----
@pytest.mark.parametrize("where", ["first", "second pass", "last"])
def test_off_curve_point_is_refused(engine, oracle, where):
    import torch

    n = PASS + 5
    bad = {"first": 0, "second pass": PASS, "last": n - 1}[where]
    d_p = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    engine.ed_generate_bases_device(0xBADC0DE, n, d_p.data_ptr())
    d_p[64 * bad : 64 * bad + 64] = dev(R.ed_encode_points([VV.off_curve_point()]))
    d_s = dev(R.encode_scalars([5]))
    d_out = poisoned(64 * n, 0xA5)
    err = code_of(engine.ed_batch_mul_var_device, d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), 0)
    assert err.code == EPOINT and err.index == bad and "not on the curve" in str(err)
    assert bool((d_out == 0xA5).all().item())


def test_noncanonical_and_two_bad_points(engine, cases):
    pb, sb, _ = cases[257]
    gx, gy = R.ED_G
    noncanonical, off = R.ed_encode_points([(gx + R.Q, gy)]), R.ed_encode_points([VV.off_curve_point()])

    def plant(buf, at):
        b = bytearray(pb)
        for i, rec in at.items():
            b[64 * i : 64 * i + 64] = rec
        return bytes(b)

    for at, index, text in (({200: noncanonical}, 200, "not below q"), ({130: off, 64: off}, 64, "not on the curve"), ({70: noncanonical, 69: off}, 69, "not on the curve")):
        points = plant(pb, at)
        d_p, d_s, d_out = dev(points), dev(sb), poisoned(64 * 257, 0xA5)
        err = code_of(engine.ed_batch_mul_var_device, d_p.data_ptr(), d_s.data_ptr(), 257, d_out.data_ptr())
        assert err.code == EPOINT and err.index == index and text in str(err), at
        assert bool((d_out == 0xA5).all().item())
        host = code_of(engine.ed_batch_mul_var, points, sb)  # the host-buffer call: the same verdict, before any upload
        assert (host.code, host.index) == (EPOINT, index)
        twin = code_of(msm.ed_batch_mul_var_host, points, sb)
        assert (twin.code, twin.index) == (EPOINT, index)
        rep = msm.ed_check_points_host(points, CHECK_CANONICAL | CHECK_CURVE)
        assert rep.first_bad == index


def test_arguments(engine, cases):
    lib = msm.load_library()
    ctx = engine._ctx
    pb, sb, wire = cases[1]
    pb2, sb2 = VV.encode([R.ED_G, R.ed_mul(R.ED_G, 5)], [3, 4])
    d_p, d_s = dev(pb2 + bytes(16)), dev(sb2 + bytes(16))
    d_out = poisoned(160, 0xA5)
    p, s, o = d_p.data_ptr(), d_s.data_ptr(), d_out.data_ptr()
    call = lib.msm377_ed_batch_mul_var_device
    assert call(ctx, p, s, 0, 32, o) == 0  # n = 0: no launch
    assert call(ctx, None, None, 0, 0, None) == 0
    for stride in (1, 4, 16, 31, 33, 64):
        assert call(ctx, p, s, 2, stride, o) == EINVAL, stride
    assert call(ctx, p, s, 0, 16, o) == EINVAL  # the stride is checked first
    assert call(ctx, None, s, 2, 32, o) == EINVAL
    assert call(ctx, p, None, 2, 32, o) == EINVAL
    assert call(ctx, p, s, 2, 32, None) == EINVAL
    assert call(ctx, p + 8, s, 2, 32, o) == EINVAL
    assert call(ctx, p, s + 8, 2, 32, o) == EINVAL
    assert call(ctx, p, s, 2, 32, o + 8) == EINVAL
    for forms in (("mont", "wire"), ("wire", "mont"), ("mont_flag", "wire")):
        engine.set_input_format(*forms)
        try:
            assert call(ctx, p, s, 2, 32, o) == EINVAL, forms
            assert lib.msm377_ed_batch_mul_var(ctx, pb2, sb2, 2, 32, None) == EINVAL
        finally:
            engine.set_input_format("wire", "wire")
    assert lib.msm377_ed_batch_mul_var(ctx, None, None, 2, 32, None) == EINVAL
    assert lib.msm377_ed_batch_mul_var(ctx, None, None, 2, 8, None) == EINVAL
    assert lib.msm377_ed_batch_mul_var(ctx, None, None, 0, 32, None) == 0
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 160
    assert call(ctx, p, s, 2, 32, o) == 0
    assert bytes(d_out.cpu().numpy()) == R.ed_encode_points([R.ed_mul(R.ED_G, 3), R.ed_mul(R.ED_G, 20)]) + b"\xa5" * 32


# ---- independence ----
def test_other_state_survives_and_the_other_way_round(engine, oracle, cases):
    pb, sb, wire = cases[257]
    n = 1000
    # resident G1 bases under an opt-in check (its report is the context's last check), an Edwards-BLS12 MSM, an
    # Edwards-BLS12 window table and a G1 one
    res_points = util.oracle_gen_points(oracle, n, 0x7654321, 0xBA98)
    ks = R.encode_scalars(R.rand_scalars(0x4E53, n))
    d_rp, d_k = dev(res_points), dev(ks)
    exp = util.oracle_msm(oracle, res_points, ks)
    engine.set_base_checks(E.CHECK_ALL)
    try:
        engine.set_bases_device(d_rp.data_ptr(), n)
    finally:
        engine.set_base_checks(0)
    report = engine.last_check()
    ed_points = util.oracle_ed_gen_points(oracle, n, 0x1234567, 0x89AB)
    d_ep = dev(ed_points)
    ed_exp = util.oracle_ed_msm(oracle, ed_points, ks)
    ed_base = R.ed_encode_points([R.ed_mul(R.ED_G, 0xD00E)])
    fixed = R.encode_scalars(VV.edge_scalars())
    ed_fixed_exp = msm.ed_batch_mul_multi_host(ed_base, fixed)
    assert engine.ed_batch_mul(ed_base, fixed) == ed_fixed_exp
    g1_base = V.base_bytes(R.mul(R.G, 0xD00E))
    g1_fixed_exp = msm.batch_mul_host(g1_base, fixed)
    assert engine.batch_mul(g1_base, fixed) == g1_fixed_exp
    g1_var_points = res_points[: 96 * 300]
    g1_var_exp = msm.batch_mul_var_host(g1_var_points, ks[: 32 * 300])
    d_vo, d_vi = poisoned(96 * 300), poisoned(300)

    def g1_var():
        engine.batch_mul_var_device(d_rp.data_ptr(), d_k.data_ptr(), 300, d_vo.data_ptr(), d_vi.data_ptr())
        return bytes(d_vo.cpu().numpy()[: 96 * 300]), bytes(d_vi.cpu().numpy()[:300])

    builds = (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds())
    assert g1_var() == g1_var_exp  # the table memory is shared and never valid between calls
    assert run_device(engine, pb, sb) == wire
    assert g1_var() == g1_var_exp
    assert run_device(engine, pb, sb) == wire
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == builds
    assert engine.last_check() == report
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp  # the resident bases ...
    assert engine.ed_batch_mul(ed_base, fixed) == ed_fixed_exp  # ... and both window tables are still there
    assert engine.batch_mul(g1_base, fixed) == g1_fixed_exp
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == builds
    assert run_device(engine, pb, sb) == wire  # and a call survives all of them
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp
    assert engine.ed_msm_device(d_ep.data_ptr(), d_k.data_ptr(), n) == ed_exp  # (an MSM of other points: it gives up the resident bases itself)
    assert run_device(engine, pb, sb) == wire


# ---- stash and tables against the model ----
def test_walk_stash_and_tables_against_the_model(engine, cases):
    n = 257
    pb, sb, wire = cases[n]
    points, scalars = VV.case(n)
    assert run_device(engine, pb, sb) == wire
    info, rows, products = engine.read_walk_stash()
    want = dict(kind=E.WALK_ED_BATCH_MUL_VAR, form=E.WALK_FORM_ED, point_words=36, product_words=9, product_pad=3, n=n, pass_offset=0, m=n, width=4, k=1, segments=1, stride=0)
    assert info._asdict() == want
    lanes = sorted(set(i for i in EP.LANES if i < n) | set(range(1, 60)))  # the planted classes and every edge scalar
    decoded = WVM.check_stash(rows, products, points, scalars, lanes, "n = 257: ")
    assert b"".join(R.ed_encode_result(p) for p in decoded) == wire  # the tie: the records are these points
    tinfo, words = engine.ed_read_walk_tables()
    assert (tinfo.m, tinfo.tables, tinfo.entries) == (n, 1, 8)
    WVM.check_tables(words, points, "n = 257: ")
    _, part = engine.ed_read_walk_tables(first=250, count=7)
    assert np.array_equal(part, words[:, 250:257])
    assert code_of(engine.read_walk_tables).code == ESTATE  # not a G1 pass
    engine.ed_batch_mul(R.ed_encode_points([R.ED_G]), R.encode_scalars([1, 2]))
    assert code_of(engine.ed_read_walk_tables).code == ESTATE  # not a variable-base pass


def test_n_zero_touches_nothing(engine, cases):
    pb, sb, wire = cases[65]
    assert run_device(engine, pb, sb) == wire
    before = engine.read_walk_stash(info_only=True)[0]
    lib = msm.load_library()
    builds = engine.ed_mul_table_builds()
    assert lib.msm377_ed_batch_mul_var_device(engine._ctx, None, None, 0, 32, None) == 0
    assert engine.ed_mul_table_builds() == builds
    out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    assert lib.msm377_ed_batch_mul_var(engine._ctx, pb, sb, 0, 32, ctypes.addressof(out)) == 0
    assert out.raw == b"\xa5" * 64
    assert before.kind == E.WALK_ED_BATCH_MUL_VAR
