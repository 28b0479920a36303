"""Variable-base batch multiplication on the GPU (include/msm377.h "variable-base batch multiplication";
csrc/kernels/batch_mul_var.hpp): out[i] = [s_i]P_i through msm377_g1_batch_mul_var_device / msm377_g1_batch_mul_var.
Expected values: tests/pyref.py (every exceptional case), the C oracle's scalar multiplication and closed form, and the host
twin (which tests/test_batch_mul_var_host.py pins to pyref).  No expected value comes from the device call.  Every test
leaves the engine at (wire, wire)."""
import contextlib
import ctypes

import numpy as np
import pytest

import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import check_vectors as CV
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

pytestmark = pytest.mark.gpu

r = R.R_ORDER
BLOCK = 1024  # outputs per workgroup product tree of the normalisation (4 per thread, 256 threads)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)  # around a wave, a workgroup, a thread's outputs, a tree
A0, DELTA = 0x1234567, 0x89AB  # oracle_gen_points: P_i = [A0 + i DELTA]G
STRIDE = {"wire": 96, "mont": 96, "mont_flag": 104}


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


@contextlib.contextmanager
def input_format(engine, points="wire", scalars="wire"):
    engine.set_input_format(points, scalars)
    try:
        yield
    finally:
        engine.set_input_format("wire", "wire")


def run_device(engine, points: bytes, scalars: bytes, out_form="wire", flags=True, stride=32, point_form="wire"):
    """(records, flag bytes) of one device call on freshly poisoned (0xEE) output buffers."""
    import torch

    n = len(points) // STRIDE[point_form]
    out_stride = STRIDE[out_form]
    d_p, d_s = dev(points), dev(scalars)
    d_out = torch.full((max(16, out_stride * n),), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((max(16, n),), 0xEE, dtype=torch.uint8, device="cuda")
    engine.batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr() if flags else 0, out_form, stride)
    return bytes(d_out.cpu().numpy()[: out_stride * n]), bytes(d_inf.cpu().numpy()[:n])


def oracle_mul(oracle, points: bytes, scalars, indices):
    """[s_i]P_i for the given indices by the C oracle (subgroup points: s mod r)."""
    out = ctypes.create_string_buffer(96)
    recs = []
    for i in indices:
        assert oracle.oracle_g1_scalar_mul(points[96 * i : 96 * i + 96], (scalars[i] % r).to_bytes(32, "little"), 32, ctypes.addressof(out)) == 0
        recs.append(out.raw)
    return b"".join(recs)


def pick(wire: bytes, indices):
    return b"".join(wire[96 * i : 96 * i + 96] for i in indices)


# ---- GPU == host twin == oracle ----
@pytest.fixture(scope="module")
def bulk(oracle):
    """4097 points [A0 + i DELTA]G, the edge scalars then seeded full-width ones, and the host twin's records, which a
    probe of indices pins to the oracle.  Every size takes a prefix."""
    n = max(SIZES)
    points = util.oracle_gen_points(oracle, n, A0, DELTA)
    scalars = (V.EDGE + V.random_scalars(0xF1BA5F, n))[:n]
    buf = R.encode_scalars(scalars)
    wire, flags = msm.batch_mul_var_host(points, buf)
    probe = list(range(len(V.EDGE))) + [62, 63, 64, 65, 255, 256, 257, 1022, 1023, 1024, 1025, 4095, 4096]
    assert pick(wire, probe) == oracle_mul(oracle, points, scalars, probe)
    assert flags == bytes(1 if s % r == 0 else 0 for s in scalars)
    return points, buf, wire, flags


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin_and_oracle(engine, bulk, n):
    points, buf, wire, flags = bulk
    got, got_flags = run_device(engine, points[: 96 * n], buf[: 32 * n])
    assert got_flags == flags[:n]
    assert got == wire[: 96 * n]


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_host_buffer_call(engine, bulk, out_form):
    points, buf, wire, flags = bulk
    n = 1025
    exp = wire[: 96 * n] if out_form == "wire" else V.mont_flag_records(wire[: 96 * n], flags[:n])
    assert engine.batch_mul_var(points[: 96 * n], buf[: 32 * n], out_form) == (exp, flags[:n])
    assert engine.batch_mul_var(b"", b"", out_form) == (b"", b"")


@pytest.mark.parametrize("scalar_stride", [32, 0])
def test_host_buffer_call_past_one_piece(engine, scalar_stride):
    """n = 2^20 + 1: the host-buffer call works in pieces of 2^20 points, so its loop runs twice and the second piece is
    ONE point.  Records and flags are the device call's on the same inputs, byte for byte (the tests above pin the device
    call to the oracle), on poisoned buffers: a piece that is not uploaded or downloaded shows.  With stride 0 the one
    scalar is uploaded once, before the loop, and serves both pieces."""
    import torch

    n = (1 << 20) + 1
    d_p = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0x9A5507, n, d_p.data_ptr())
    points = bytes(d_p.cpu().numpy())
    del d_p
    s = np.random.default_rng(0x9A5508).integers(0, 256, size=(n if scalar_stride else 1, 32), dtype=np.uint8)
    if scalar_stride:
        s[3] = 0
        s[(1 << 20) - 1] = 0  # identity outputs: one early, one at the end of the first piece
    sb = s.tobytes()
    out, inf = ctypes.create_string_buffer(b"\xee" * (96 * n), 96 * n), ctypes.create_string_buffer(b"\xee" * n, n)
    rc = msm.load_library().msm377_g1_batch_mul_var(engine._ctx, points, sb, n, scalar_stride, V.WIRE, ctypes.addressof(out), ctypes.addressof(inf))
    assert rc == 0
    wire, flags = run_device(engine, points, sb, stride=scalar_stride)
    assert inf.raw == flags and flags[n - 1] == 0
    if scalar_stride:
        assert flags[3] == 1 and flags[(1 << 20) - 1] == 1
    assert out.raw == wire


# ---- exceptional points, mixed within waves ----
@pytest.fixture(scope="module")
def exceptional():
    """3 x 1024 + 7 outputs: the points of V.bases() with period 7 among random subgroup points (neighbouring lanes take
    different exits), one whole workgroup's worth of a small-order point (whole table rows flagged), the order-3 point
    (0, 1) with scalar 1.  Expected by pyref."""
    n = 3 * BLOCK + 7
    points = list(VV.mixed_points(n))
    small = CV.g1_small_order_points()
    for i in range(BLOCK, BLOCK + 256):
        points[i] = small[(i // 64) % len(small)]  # a wave each
    pool = V.gpu_base_scalars(130)
    scalars = [pool[(3 * i + i // 130) % len(pool)] for i in range(n)]
    for k, i in enumerate(range(BLOCK + 256, BLOCK + 256 + 12)):
        scalars[i] = 2 + k  # small multiples on neighbouring lanes
    three = 2 * BLOCK + 77
    points[three], scalars[three] = (0, 1), 1
    wire, flags = VV.expected(points, scalars)
    assert wire[96 * three : 96 * three + 96] == V.IDENTITY_WIRE and flags[three] == 0
    assert 1 in flags
    return R.encode_points(points), R.encode_scalars(scalars), wire, flags


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_exceptional_points_mixed_within_waves(engine, exceptional, out_form):
    points, buf, wire, flags = exceptional
    got, got_flags = run_device(engine, points, buf, out_form)
    assert got_flags == flags
    assert got == (wire if out_form == "wire" else V.mont_flag_records(wire, flags))


# ---- identity outputs: a zero in a product tree would wipe a block ----
def test_identity_outputs_leave_their_neighbours_exact(engine, oracle):
    n = 3 * BLOCK + 7
    points = util.oracle_gen_points(oracle, n, A0 + 5, DELTA)
    scalars = V.random_scalars(0x1DE48, n)
    zeros = [0, r, 2 * r]
    where = [0, n - 1, 255, 256, BLOCK - 1, 2 * BLOCK, 3 * BLOCK] + list(range(BLOCK, 2 * BLOCK))  # one whole workgroup's outputs
    where += [2 * BLOCK + 5 + 256 * j for j in range(4)]  # all four outputs of one thread
    for k, i in enumerate(where):
        scalars[i] = zeros[k % 3]
    buf = R.encode_scalars(scalars)
    exp_flags = bytes(1 if i in set(where) else 0 for i in range(n))
    probe = [1, 254, 257, BLOCK - 2, 2 * BLOCK + 1, 2 * BLOCK + 4, 2 * BLOCK + 6, 3 * BLOCK - 1, 3 * BLOCK + 1, n - 2]
    exp_probe = oracle_mul(oracle, points, scalars, probe)
    wire, flags = msm.batch_mul_var_host(points, buf)
    assert flags == exp_flags and pick(wire, probe) == exp_probe
    for out_form in ("wire", "mont_flag"):
        got, got_flags = run_device(engine, points, buf, out_form)
        assert got_flags == exp_flags, out_form
        if out_form == "wire":
            assert pick(got, probe) == exp_probe
            assert pick(got, where) == V.IDENTITY_WIRE * len(where)
        assert got == (wire if out_form == "wire" else V.mont_flag_records(wire, flags)), out_form


# ---- one scalar for all points ----
@pytest.mark.parametrize("scalar", [V.random_scalars(0xB40ADCA5, 1)[0] | 1 << 255, 0xD0E5_0F7A_B1 | 1 << 39])
def test_broadcast_scalar(engine, bulk, scalar):
    points = bulk[0][: 96 * 257]
    one = R.encode_scalars([scalar])
    exp = msm.batch_mul_var_host(points, one * 257)
    assert run_device(engine, points, one * 257) == exp
    assert run_device(engine, points, one, stride=0) == exp
    assert engine.batch_mul_var(points, one) == exp  # 32 bytes for 257 points: stride 0


# ---- short scalars: the leading-window skip ----
@pytest.mark.parametrize("kind", ["64-bit", "zero", "one-lane-bit-255"])
def test_short_scalars(engine, bulk, kind):
    n = 1025
    points = bulk[0][: 96 * n]
    if kind == "64-bit":
        scalars = V.random_scalars(0x5404764, n, bits=64)
    elif kind == "zero":
        scalars = [0] * n
    else:  # one lane per wave walks all 64 windows, its neighbours wake up late
        scalars = V.random_scalars(0x5404765, n, bits=24)
        for wave in range((n + 63) // 64):
            i = min(n - 1, 64 * wave + (11 * wave) % 64)
            scalars[i] |= 1 << 255
    buf = R.encode_scalars(scalars)
    assert run_device(engine, points, buf) == msm.batch_mul_var_host(points, buf)


# ---- a pass boundary, past the context's capacity: every output enters one MSM with a random weight ----
def test_pass_boundary_past_the_context_capacity(engine, oracle):
    """n = 2^17 + 3 on an engine created for 2^16 points: two passes, the second of three outputs."""
    import torch

    n = (1 << 17) + 3
    points = util.oracle_gen_points(oracle, n, A0, DELTA)
    rng = np.random.default_rng(0x5CA1F)
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    t[:, 31] &= 0x0F  # weights below 2^252 < r; the scalars are full width
    sb, tb = s.tobytes(), t.tobytes()
    si = [int.from_bytes(sb[32 * i : 32 * i + 32], "little") for i in range(n)]
    ti = [int.from_bytes(tb[32 * i : 32 * i + 32], "little") for i in range(n)]
    d_p, d_s, d_t = dev(points), dev(sb), dev(tb)
    d_out = torch.full((96 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    with msm.MsmEngine(1 << 16) as small:
        small.batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
    assert not d_inf.any().item()
    total = sum(tw * sw * (A0 + i * DELTA) for i, (sw, tw) in enumerate(zip(si, ti)))
    assert engine.msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == util.closed_form(oracle, total)
    last = bytes(d_out[96 * (n - 3) :].cpu().numpy())
    assert last == b"".join(util.closed_form(oracle, si[i] * (A0 + i * DELTA)) for i in range(n - 3, n))


# ---- forms ----
@pytest.fixture(scope="module")
def mixed_small():
    n = 257
    points = list(VV.mixed_points(n, period=5))
    pool = V.gpu_base_scalars(130)
    scalars = [pool[(7 * i + 2) % len(pool)] for i in range(n)]
    flagged = (0, 1, 63, 64, 129, 256)
    return points, scalars, flagged, VV.expected(points, scalars), VV.expected(points, scalars, flagged)


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
@pytest.mark.parametrize("point_form", ["mont", "mont_flag"])
def test_native_point_forms(engine, mixed_small, point_form, out_form):
    points, scalars, flagged, plain, with_flags = mixed_small
    if point_form == "mont":
        buf, (wire, flags) = VV.mont_records(points), plain
    else:  # flagged records hold garbage coordinates
        buf, (wire, flags) = VV.mont_records(points, True, flagged), with_flags
    exp = wire if out_form == "wire" else V.mont_flag_records(wire, flags)
    sbuf = R.encode_scalars(scalars)
    with input_format(engine, point_form, "wire"):
        assert run_device(engine, buf, sbuf, out_form, point_form=point_form) == (exp, flags)
        assert engine.batch_mul_var(buf, sbuf, out_form) == (exp, flags)


def test_montgomery_scalars(engine, bulk):
    n = 257
    points = bulk[0][: 96 * n]
    values = (VV.MONT_SCALAR_VALUES + V.random_scalars(0x30A8, n))[:n]
    exp = msm.batch_mul_var_host(points, R.encode_scalars(VV.mont_scalars(values)))
    assert msm.batch_mul_var_host(points, R.encode_scalars(values), scalar_form="mont") == exp
    assert run_device(engine, points, R.encode_scalars(VV.mont_scalars(values))) == exp
    with input_format(engine, "wire", "mont"):
        assert run_device(engine, points, R.encode_scalars(values)) == exp
        assert run_device(engine, points, R.encode_scalars(values[7:8]), stride=0) == msm.batch_mul_var_host(points, R.encode_scalars(VV.mont_scalars(values[7:8])))
        assert engine.batch_mul_var(points, R.encode_scalars(values)) == exp


def test_mont_flag_round_trip(engine, oracle):
    """MONT_FLAG records feed set_bases / msm on a mont_flag context."""
    import torch

    n = 257
    points = util.oracle_gen_points(oracle, n, A0, DELTA)
    scalars = V.random_scalars(0xF1A7, n)
    identities = {0, 63, 64, 128, 256}
    for k, i in enumerate(sorted(identities)):
        scalars[i] = (0, r, 2 * r)[k % 3]
    weights = R.rand_scalars(0x7E17, n)
    d_p, d_s, d_t = dev(points), dev(R.encode_scalars(scalars)), dev(R.encode_scalars(weights))
    d_out = torch.empty(104 * n, dtype=torch.uint8, device="cuda")
    engine.batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), 0, "mont_flag")
    exp = util.closed_form(oracle, sum(s * t * (A0 + i * DELTA) for i, (s, t) in enumerate(zip(scalars, weights)) if i not in identities))
    with input_format(engine, "mont_flag", "wire"):
        assert engine.msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == exp
        engine.set_bases_device(d_out.data_ptr(), n)
        assert engine.msm_fixed_base_device(d_t.data_ptr(), n) == exp


def test_in_place(engine, bulk):
    """d_out == d_points, wire to wire."""
    points, buf, wire, flags = bulk
    n = 1025
    d_p, d_s = dev(points[: 96 * n]), dev(buf[: 32 * n])
    engine.batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_p.data_ptr())
    assert bytes(d_p.cpu().numpy()) == wire[: 96 * n]


# ---- state ----
def test_other_state_survives_and_the_other_way_round(engine, oracle, bulk):
    points, buf, wire, flags = bulk
    n = 1000
    vp, vs, vexp = points[: 96 * 300], buf[: 32 * 300], (wire[: 96 * 300], flags[:300])
    res_points = util.oracle_gen_points(oracle, n, 0x7654321, 0xBA98)
    ks = R.encode_scalars(R.rand_scalars(0x4E53, n))
    d_p, d_k = dev(res_points), dev(ks)
    exp = util.oracle_msm(oracle, res_points, ks)
    engine.set_bases_device(d_p.data_ptr(), n)
    base = V.base_bytes(R.mul(R.G, 0xD00E))
    fixed = R.encode_scalars(V.EDGE + V.random_scalars(0x4E54, 100))
    fixed_exp = msm.batch_mul_host(base, fixed)
    assert engine.batch_mul(base, fixed) == fixed_exp
    builds = engine.mul_table_builds()
    assert run_device(engine, vp, vs) == vexp
    assert engine.mul_table_builds() == builds
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp  # the resident bases ...
    assert engine.batch_mul(base, fixed) == fixed_exp                # ... and the window table are still there
    assert engine.mul_table_builds() == builds
    assert engine.check_points_device(d_p.data_ptr(), n).ok
    assert run_device(engine, vp, vs) == vexp                        # and a var call survives all three
    assert engine.check_points_device(d_p.data_ptr(), n).ok
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp


# ---- arguments ----
def test_arguments(engine):
    import torch

    lib = msm.load_library()
    ctx = engine._ctx
    pts = [R.mul(R.G, 0xE1A8), R.FIXED_BASE]
    d_p = dev(R.encode_points(pts) + bytes(16))
    d_s = dev(R.encode_scalars([3, 4]) + bytes(16))
    d_out = torch.full((224,), 0xA5, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    p, s, o = d_p.data_ptr(), d_s.data_ptr(), d_out.data_ptr()

    def call(points, scalars, n, stride, form, out):
        return lib.msm377_g1_batch_mul_var_device(ctx, points, scalars, n, stride, form, out, d_inf.data_ptr())

    assert call(p, s, 0, 32, V.WIRE, o) == 0  # n = 0: no launch
    assert call(None, None, 0, 0, V.MONT_FLAG, None) == 0
    assert call(p, s, 2, 32, V.MONT, o) == EINVAL  # plain mont cannot say "identity"
    assert call(p, s, 0, 32, V.MONT, o) == EINVAL
    assert call(p, s, 2, 32, 3, o) == EINVAL
    for stride in (1, 4, 16, 31, 33, 64):
        assert call(p, s, 2, stride, V.WIRE, o) == EINVAL, stride
    assert call(None, s, 2, 32, V.WIRE, o) == EINVAL
    assert call(p, None, 2, 32, V.WIRE, o) == EINVAL
    assert call(p, s, 2, 32, V.WIRE, None) == EINVAL
    assert call(p + 8, s, 2, 32, V.WIRE, o) == EINVAL  # alignment: 16 bytes for 96-byte records and scalars
    assert call(p, s + 8, 2, 32, V.WIRE, o) == EINVAL
    assert call(p, s, 2, 32, V.WIRE, o + 8) == EINVAL
    assert call(p, s, 2, 32, V.MONT_FLAG, o + 4) == EINVAL  # 8 bytes for 104-byte records
    with input_format(engine, "mont_flag", "wire"):
        assert call(p + 4, s, 1, 32, V.WIRE, o) == EINVAL
    assert lib.msm377_g1_batch_mul_var(ctx, None, None, 2, 32, V.WIRE, None, None) == EINVAL
    assert lib.msm377_g1_batch_mul_var(ctx, None, None, 2, 8, V.WIRE, None, None) == EINVAL
    assert lib.msm377_g1_batch_mul_var(ctx, None, None, 0, 32, V.WIRE, None, None) == 0
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 224 and bytes(d_inf.cpu().numpy()) == b"\xa5" * 16
    exp = R.encode_points([R.mul(pts[0], 3), R.mul(pts[1], 4)])
    got, flags = run_device(engine, R.encode_points(pts), R.encode_scalars([3, 4]), flags=False)  # d_out_inf may be null
    assert got == exp and flags == b"\xee\xee"
    assert call(p, s, 2, 32, V.MONT_FLAG, o + 8) == 0  # an 8-byte aligned mont_flag output is fine
    assert bytes(d_out.cpu().numpy())[8 : 8 + 208] == V.mont_flag_records(exp, b"\x00\x00")
