"""Pairwise linear combination on the GPU (include/msm377.h "pairwise linear combination";
csrc/kernels/batch_lincomb2.hpp): out[i] = [a_i]P_i + [b_i]Q_i through msm377_g1_batch_lincomb2_device /
msm377_g1_batch_lincomb2.  Expected values: tests/pyref.py (every exceptional case and relation), the C oracle's closed
form, and the host twin (which tests/test_batch_lincomb2_host.py pins to pyref).  No expected value comes from the device
call.  Every test leaves the engine at (wire, wire)."""
import contextlib

import numpy as np
import pytest

import batch_lincomb2_vectors as LV
import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

pytestmark = pytest.mark.gpu

r = R.R_ORDER
BLOCK = LV.BLOCK
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)  # around a wave, a workgroup, a thread's outputs, a tree
A0, DELTA = 0x1234567, 0x89AB    # oracle_gen_points: P_i = [A0 + i DELTA]G
A1, DELTA1 = 0x7654321, 0xBA987  # Q_i = [A1 + i DELTA1]G
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


def run_device(engine, p: bytes, q: bytes, a: bytes, b: bytes, out_form="wire", flags=True, a_stride=32, b_stride=32, point_form="wire"):
    """(records, flag bytes) of one device call on freshly poisoned (0xEE) output buffers."""
    import torch

    n = len(p) // STRIDE[point_form]
    out_stride = STRIDE[out_form]
    d_p, d_q, d_a, d_b = dev(p), dev(q), dev(a), dev(b)
    d_out = torch.full((max(16, out_stride * n),), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((max(16, n),), 0xEE, dtype=torch.uint8, device="cuda")
    engine.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr() if flags else 0, out_form, a_stride, b_stride)
    return bytes(d_out.cpu().numpy()[: out_stride * n]), bytes(d_inf.cpu().numpy()[:n])


def pick(wire: bytes, indices):
    return b"".join(wire[96 * i : 96 * i + 96] for i in indices)


def closed(oracle, a, b, indices):
    """[a_i (A0 + i DELTA) + b_i (A1 + i DELTA1)]G by the oracle."""
    return b"".join(util.closed_form(oracle, a[i] * (A0 + i * DELTA) + b[i] * (A1 + i * DELTA1)) for i in indices)


def negated(points: bytes, indices):
    """The wire records of `points` with the records at `indices` negated (y -> p - y)."""
    out = bytearray(points)
    for i in indices:
        y = int.from_bytes(out[96 * i + 48 : 96 * i + 96], "little")
        out[96 * i + 48 : 96 * i + 96] = ((R.P - y) % R.P).to_bytes(48, "little")
    return bytes(out)


# ---- 1. GPU == host twin == oracle ----
@pytest.fixture(scope="module")
def bulk(oracle):
    """4097 pairs P_i = [A0 + i DELTA]G, Q_i = [A1 + i DELTA1]G, the edge scalars then seeded full-width ones, and the host
    twin's records, which a probe of indices pins to the oracle's closed form.  Every size takes a prefix."""
    n = max(SIZES)
    p = util.oracle_gen_points(oracle, n, A0, DELTA)
    q = util.oracle_gen_points(oracle, n, A1, DELTA1)
    a = (V.EDGE + V.random_scalars(0xF1BA60, n))[:n]
    b = (V.EDGE[::-1] + V.random_scalars(0xF1BA61, n))[:n]
    ab, bb = R.encode_scalars(a), R.encode_scalars(b)
    wire, flags = msm.batch_lincomb2_host(p, q, ab, bb)
    probe = list(range(len(V.EDGE))) + [62, 63, 64, 65, 255, 256, 257, 1022, 1023, 1024, 1025, 4095, 4096]
    assert pick(wire, probe) == closed(oracle, a, b, probe)
    assert not any(flags)
    return p, q, ab, bb, wire, flags


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin_and_oracle(engine, bulk, n):
    p, q, a, b, wire, flags = bulk
    got, got_flags = run_device(engine, p[: 96 * n], q[: 96 * n], a[: 32 * n], b[: 32 * n])
    assert got_flags == flags[:n]
    assert got == wire[: 96 * n]


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_host_buffer_call(engine, bulk, out_form):
    p, q, a, b, wire, flags = bulk
    n = 1025
    exp = LV.out_records(wire[: 96 * n], flags[:n], out_form)
    assert engine.batch_lincomb2(p[: 96 * n], q[: 96 * n], a[: 32 * n], b[: 32 * n], out_form) == (exp, flags[:n])
    assert engine.batch_lincomb2(b"", b"", b"", b"", out_form) == (b"", b"")


@pytest.mark.parametrize("a_stride,b_stride", [(32, 0), (0, 32)])
def test_host_buffer_call_past_one_piece(engine, a_stride, b_stride):
    """n = 2^20 + 1: the host-buffer call works in pieces of 2^20 pairs, so its loop runs twice and the second piece is
    ONE pair.  Records and flags are the device call's on the same inputs, byte for byte (the tests above pin the device
    call to the oracle), on poisoned buffers: a piece that is not uploaded or downloaded shows.  One scalar array has a
    scalar per pair, uploaded piece by piece; the other is the stride-0 scalar, uploaded once before the loop."""
    import ctypes

    import torch

    n = (1 << 20) + 1
    d_pq = torch.empty(96 * 2 * n, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0x1C0B2, 2 * n, d_pq.data_ptr())
    pq = bytes(d_pq.cpu().numpy())
    del d_pq
    p, q = pq[: 96 * n], pq[96 * n :]
    rng = np.random.default_rng(0x1C0B3)
    a = rng.integers(0, 256, size=(n if a_stride else 1, 32), dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, size=(n if b_stride else 1, 32), dtype=np.uint8).tobytes()
    out, inf = ctypes.create_string_buffer(b"\xee" * (96 * n), 96 * n), ctypes.create_string_buffer(b"\xee" * n, n)
    rc = msm.load_library().msm377_g1_batch_lincomb2(engine._ctx, p, q, a, b, n, a_stride, b_stride, V.WIRE, ctypes.addressof(out), ctypes.addressof(inf))
    assert rc == 0
    wire, flags = run_device(engine, p, q, a, b, a_stride=a_stride, b_stride=b_stride)
    assert inf.raw == flags == bytes(n)
    assert out.raw == wire


# ---- 2. a pass boundary, past the context's capacity: every output enters one MSM with a random weight ----
def test_pass_boundary_past_the_context_capacity(engine, oracle):
    """n = 2^16 + 3 on an engine created for 2^12 points: two passes, the second of three outputs."""
    import torch

    n = (1 << 16) + 3
    p = util.oracle_gen_points(oracle, n, A0, DELTA)
    q = util.oracle_gen_points(oracle, n, A1, DELTA1)
    rng = np.random.default_rng(0x5CA20)
    a, b, t = (rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for _ in range(3))
    t[:, 31] &= 0x0F  # weights below 2^252 < r; the scalars are full width
    ab, bb, tb = a.tobytes(), b.tobytes(), t.tobytes()
    ai, bi, ti = ([int.from_bytes(buf[32 * i : 32 * i + 32], "little") for i in range(n)] for buf in (ab, bb, tb))
    d_p, d_q, d_a, d_b, d_t = dev(p), dev(q), dev(ab), dev(bb), dev(tb)
    d_out = torch.full((96 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    with msm.MsmEngine(1 << 12) as small:
        small.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
    assert not d_inf.any().item()
    total = sum(tw * (aw * (A0 + i * DELTA) + bw * (A1 + i * DELTA1)) for i, (aw, bw, tw) in enumerate(zip(ai, bi, ti)))
    assert engine.msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == util.closed_form(oracle, total)
    last = bytes(d_out[96 * (n - 3) :].cpu().numpy())
    assert last == closed(oracle, ai, bi, range(n - 3, n))


# ---- 3. relations and exceptional points, mixed within waves ----
@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_relations_and_exceptional_points_mixed_within_waves(engine, out_form):
    """Q = P, Q = -P, Q = [k]P with a = -k b, flagged records, small orders and torsion, zero scalars, carries -- in
    neighbouring lanes, and whole waves of a small-order point (LV.relations).  The flags need the mont_flag point form."""
    p, q, a, b, fp, fq = LV.relations()
    wire, flags = LV.relations_expected(True)
    assert flags.count(1) > 200 and wire[96 * (2 * BLOCK + 77) :][:96] == V.IDENTITY_WIRE and flags[2 * BLOCK + 77] == 0
    pb, qb = VV.mont_records(p, True, fp), VV.mont_records(q, True, fq)
    with input_format(engine, "mont_flag", "wire"):
        got, got_flags = run_device(engine, pb, qb, R.encode_scalars(a), R.encode_scalars(b), out_form, point_form="mont_flag")
    assert got_flags == flags
    assert got == LV.out_records(wire, flags, out_form)


# ---- 4. identity outputs: a zero in a product tree would wipe a block ----
def test_identity_outputs_leave_their_neighbours_exact(engine, oracle):
    n = 3 * BLOCK + 7
    p = util.oracle_gen_points(oracle, n, A0 + 5, DELTA)
    a = V.random_scalars(0x1DE49, n)
    b = V.random_scalars(0x1DE4A, n)
    where = [0, n - 1, 255, 256, BLOCK - 1, 2 * BLOCK, 3 * BLOCK] + list(range(BLOCK, 2 * BLOCK))  # one whole workgroup's outputs
    where += [2 * BLOCK + 5 + 256 * j for j in range(4)]  # all four outputs of one thread
    opposite = [i for k, i in enumerate(where) if k % 2 == 0]  # Q = -P with a = b; the others a = b = 0
    for k, i in enumerate(where):
        a[i] = b[i] = a[i] if k % 2 == 0 else 0
    q = bytearray(util.oracle_gen_points(oracle, n, A0 + 5, DELTA1))  # Q_i = [A0 + 5 + i DELTA1]G ...
    for i in opposite:  # ... but -P_i here
        q[96 * i : 96 * i + 96] = negated(p[96 * i : 96 * i + 96], [0])
    q = bytes(q)
    ab, bb = R.encode_scalars(a), R.encode_scalars(b)
    exp_flags = bytes(1 if i in set(where) else 0 for i in range(n))
    probe = [1, 254, 257, BLOCK - 2, 2 * BLOCK + 1, 2 * BLOCK + 4, 2 * BLOCK + 6, 3 * BLOCK - 1, 3 * BLOCK + 1, n - 2]
    exp_probe = b"".join(util.closed_form(oracle, a[i] * (A0 + 5 + i * DELTA) + b[i] * (A0 + 5 + i * DELTA1)) for i in probe)
    wire, flags = msm.batch_lincomb2_host(p, q, ab, bb)
    assert flags == exp_flags and pick(wire, probe) == exp_probe
    for out_form in ("wire", "mont_flag"):
        got, got_flags = run_device(engine, p, q, ab, bb, out_form)
        assert got_flags == exp_flags, out_form
        if out_form == "wire":
            assert pick(got, probe) == exp_probe
            assert pick(got, where) == V.IDENTITY_WIRE * len(where)
        assert got == LV.out_records(wire, flags, out_form), out_form


# ---- 5. strides; the fold in place ----
@pytest.mark.parametrize("a_stride,b_stride", [(32, 32), (0, 32), (32, 0), (0, 0)])
def test_strides(engine, bulk, a_stride, b_stride):
    p, q, a, b, _, _ = bulk
    n = 257
    p, q = p[: 96 * n], q[: 96 * n]
    one_a, one_b = R.encode_scalars([V.random_scalars(0xB40ADCA6, 1)[0] | 1 << 255]), R.encode_scalars([0xD0E5_0F7A_B1 | 1 << 39])
    a = a[: 32 * n] if a_stride else one_a
    b = b[: 32 * n] if b_stride else one_b
    exp = msm.batch_lincomb2_host(p, q, a * (1 if a_stride else n), b * (1 if b_stride else n))  # the expanded arrays
    assert run_device(engine, p, q, a * (1 if a_stride else n), b * (1 if b_stride else n)) == exp
    assert run_device(engine, p, q, a, b, a_stride=a_stride, b_stride=b_stride) == exp
    assert engine.batch_lincomb2(p, q, a, b) == exp  # 32 bytes for 257 pairs: stride 0


def test_fold_in_place(engine, oracle):
    """G' = [x^-1]G_lo + [x]G_hi written over G_lo: p = G, q = G + h records, out = G, n = h, both strides 0."""
    h = 1025
    basis = util.oracle_gen_points(oracle, 2 * h, A0, DELTA)
    x = V.random_scalars(0xF01D, 1)[0] % r
    xa, xb = R.encode_scalars([pow(x, -1, r)]), R.encode_scalars([x])
    exp, flags = msm.batch_lincomb2_host(basis[: 96 * h], basis[96 * h :], xa, xb)
    probe = [0, 1, 1023, 1024]
    assert pick(exp, probe) == b"".join(util.closed_form(oracle, pow(x, -1, r) * (A0 + i * DELTA) + x * (A0 + (i + h) * DELTA)) for i in probe)
    d_g, d_a, d_b = dev(basis), dev(xa), dev(xb)
    engine.batch_lincomb2_device(d_g.data_ptr(), d_g.data_ptr() + 96 * h, d_a.data_ptr(), d_b.data_ptr(), h, d_g.data_ptr(), 0, "wire", 0, 0)
    got = bytes(d_g.cpu().numpy())
    assert got[96 * h :] == basis[96 * h :]  # the upper half: byte-identical
    assert got[: 96 * h] == exp


# ---- 6. short walks: the wave-uniform skip ----
def test_plain_addition(engine):
    """a = b = 1 with stride 0: P_i + Q_i over the fixture of relations, by pyref's add."""
    p, q, _, _, _, _ = LV.relations()
    one = R.encode_scalars([1])
    assert run_device(engine, R.encode_points(p), R.encode_points(q), one, one, a_stride=0, b_stride=0) == LV.relations_sum()


@pytest.mark.parametrize("kind", ["64-bit", "zero", "one-lane-bit-255"])
def test_short_scalars(engine, bulk, kind):
    n = 1025
    p, q = bulk[0][: 96 * n], bulk[1][: 96 * n]
    if kind == "64-bit":
        a, b = V.random_scalars(0x5404766, n, bits=64), V.random_scalars(0x5404767, n, bits=64)
    elif kind == "zero":
        a, b = [0] * n, [0] * n
    else:  # one lane per wave walks all the windows, its neighbours wake up late: in a in even waves, in b in odd ones
        a, b = V.random_scalars(0x5404768, n, bits=24), V.random_scalars(0x5404769, n, bits=24)
        for wave in range((n + 63) // 64):
            i = min(n - 1, 64 * wave + (11 * wave) % 64)
            (b if wave % 2 else a)[i] |= 1 << 255
    ab, bb = R.encode_scalars(a), R.encode_scalars(b)
    exp = msm.batch_lincomb2_host(p, q, ab, bb)
    if kind == "zero":
        assert exp == (V.IDENTITY_WIRE * n, b"\x01" * n)
    assert run_device(engine, p, q, ab, bb) == exp


# ---- 7. forms ----
@pytest.fixture(scope="module")
def mixed_small():
    n = 257
    p = list(VV.mixed_points(n, period=5))
    q = list(VV.mixed_points(n, seed=0x4B12EE, period=3))
    pool = V.gpu_base_scalars(130)
    a = [pool[(7 * i + 2) % len(pool)] for i in range(n)]
    b = [pool[(11 * i + 5) % len(pool)] for i in range(n)]
    fp, fq = (0, 1, 63, 129, 256), (1, 64, 129, 200)
    return p, q, a, b, fp, fq, LV.expected(p, q, a, b), LV.expected(p, q, a, b, fp, fq)


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
@pytest.mark.parametrize("point_form", ["mont", "mont_flag"])
def test_native_point_forms(engine, mixed_small, point_form, out_form):
    p, q, a, b, fp, fq, plain, with_flags = mixed_small
    if point_form == "mont":
        pb, qb, (wire, flags) = VV.mont_records(p), VV.mont_records(q), plain
    else:  # flagged records hold garbage coordinates
        pb, qb, (wire, flags) = VV.mont_records(p, True, fp), VV.mont_records(q, True, fq), with_flags
    exp = LV.out_records(wire, flags, out_form)
    ab, bb = R.encode_scalars(a), R.encode_scalars(b)
    with input_format(engine, point_form, "wire"):
        assert run_device(engine, pb, qb, ab, bb, out_form, point_form=point_form) == (exp, flags)
        assert engine.batch_lincomb2(pb, qb, ab, bb, out_form) == (exp, flags)


def test_montgomery_scalars(engine, bulk):
    n = 257
    p, q = bulk[0][: 96 * n], bulk[1][: 96 * n]
    va = (VV.MONT_SCALAR_VALUES + V.random_scalars(0x30A9, n))[:n]
    vb = (V.random_scalars(0x30AA, n - 7) + VV.MONT_SCALAR_VALUES)[:n]
    enc = R.encode_scalars
    exp = msm.batch_lincomb2_host(p, q, enc(VV.mont_scalars(va)), enc(VV.mont_scalars(vb)))
    assert msm.batch_lincomb2_host(p, q, enc(va), enc(vb), scalar_form="mont") == exp
    assert run_device(engine, p, q, enc(VV.mont_scalars(va)), enc(VV.mont_scalars(vb))) == exp
    with input_format(engine, "wire", "mont"):
        assert run_device(engine, p, q, enc(va), enc(vb)) == exp
        one = msm.batch_lincomb2_host(p, q, enc(VV.mont_scalars(va[7:8])), enc(VV.mont_scalars(vb)))
        assert run_device(engine, p, q, enc(va[7:8]), enc(vb), a_stride=0) == one
        assert engine.batch_lincomb2(p, q, enc(va), enc(vb)) == exp


def test_mont_flag_round_trip(engine, oracle):
    """MONT_FLAG records feed set_bases / msm on a mont_flag context."""
    import torch

    n = 257
    p = util.oracle_gen_points(oracle, n, A0, DELTA)
    q = util.oracle_gen_points(oracle, n, A1, DELTA1)
    a, b = V.random_scalars(0xF1A8, n), V.random_scalars(0xF1A9, n)
    identities = {0, 63, 64, 128, 256}
    for k, i in enumerate(sorted(identities)):
        a[i], b[i] = (0, r, 2 * r)[k % 3], (r, 0, 0)[k % 3]
    weights = R.rand_scalars(0x7E18, n)
    d_p, d_q, d_a, d_b, d_t = dev(p), dev(q), dev(R.encode_scalars(a)), dev(R.encode_scalars(b)), dev(R.encode_scalars(weights))
    d_out = torch.empty(104 * n, dtype=torch.uint8, device="cuda")
    engine.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr(), 0, "mont_flag")
    exp = util.closed_form(oracle, sum(t * (x * (A0 + i * DELTA) + y * (A1 + i * DELTA1)) for i, (x, y, t) in enumerate(zip(a, b, weights))))
    with input_format(engine, "mont_flag", "wire"):
        assert engine.msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == exp
        engine.set_bases_device(d_out.data_ptr(), n)
        assert engine.msm_fixed_base_device(d_t.data_ptr(), n) == exp


# ---- 8. consistency with the variable-base call ----
def test_zero_b_equals_the_variable_base_call(engine, bulk):
    """With b = 0 the records are those of batch_mul_var_device(P, a), byte for byte, in both forms."""
    import torch

    p, q, a, _, _, _ = bulk
    n = 1025
    d_p, d_q, d_a, d_zero = dev(p[: 96 * n]), dev(q[: 96 * n]), dev(a[: 32 * n]), dev(bytes(32))
    for out_form in ("wire", "mont_flag"):
        size = STRIDE[out_form] * n
        outs = [torch.full((size,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        infs = [torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        engine.batch_mul_var_device(d_p.data_ptr(), d_a.data_ptr(), n, outs[0].data_ptr(), infs[0].data_ptr(), out_form)
        engine.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_zero.data_ptr(), n, outs[1].data_ptr(), infs[1].data_ptr(), out_form, 32, 0)
        assert torch.equal(outs[0], outs[1]) and torch.equal(infs[0], infs[1]), out_form
        assert msm.batch_mul_var_host(p[: 96 * n], a[: 32 * n], out_form)[0] == bytes(outs[1].cpu().numpy())


# ---- 9. in place ----
@pytest.mark.parametrize("over", ["p", "q"])
def test_in_place(engine, bulk, over):
    """d_out == d_p, then d_out == d_q, wire to wire."""
    p, q, a, b, wire, flags = bulk
    n = 1025
    d_p, d_q, d_a, d_b = dev(p[: 96 * n]), dev(q[: 96 * n]), dev(a[: 32 * n]), dev(b[: 32 * n])
    target, other, kept = (d_p, d_q, q) if over == "p" else (d_q, d_p, p)
    engine.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, target.data_ptr())
    assert bytes(target.cpu().numpy()) == wire[: 96 * n]
    assert bytes(other.cpu().numpy()) == kept[: 96 * n]


# ---- 10. state ----
def test_other_state_survives_and_the_other_way_round(engine, oracle, bulk):
    p, q, a, b, wire, flags = bulk
    n = 1000
    m = 300
    lp, lq, la, lb, lexp = p[: 96 * m], q[: 96 * m], a[: 32 * m], b[: 32 * m], (wire[: 96 * m], flags[:m])
    var_exp = msm.batch_mul_var_host(lp, la)
    res_points = util.oracle_gen_points(oracle, n, 0x7654321, 0xBA98)
    ks = R.encode_scalars(R.rand_scalars(0x4E55, n))
    d_r, d_k = dev(res_points), dev(ks)
    exp = util.oracle_msm(oracle, res_points, ks)
    engine.set_bases_device(d_r.data_ptr(), n)
    base = V.base_bytes(R.mul(R.G, 0xD00F))
    fixed = R.encode_scalars(V.EDGE + V.random_scalars(0x4E56, 100))
    fixed_exp = msm.batch_mul_host(base, fixed)
    assert engine.batch_mul(base, fixed) == fixed_exp
    builds = engine.mul_table_builds()
    assert engine.batch_mul_var(lp, la) == var_exp
    assert run_device(engine, lp, lq, la, lb) == lexp
    assert engine.mul_table_builds() == builds
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp  # the resident bases ...
    assert engine.batch_mul(base, fixed) == fixed_exp                # ... the window table ...
    assert engine.batch_mul_var(lp, la) == var_exp                   # ... and a var call are as they were
    assert engine.mul_table_builds() == builds
    assert engine.check_points_device(d_r.data_ptr(), n).ok
    assert run_device(engine, lp, lq, la, lb) == lexp                # and a lincomb2 call survives all four
    assert engine.check_points_device(d_r.data_ptr(), n).ok
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp


# ---- 11. arguments ----
def test_arguments(engine):
    import torch

    lib = msm.load_library()
    ctx = engine._ctx
    pts, qts = [R.mul(R.G, 0xE1A9), R.FIXED_BASE], [R.FIXED_BASE, R.mul(R.G, 0x77)]
    d_p, d_q = dev(R.encode_points(pts) + bytes(16)), dev(R.encode_points(qts) + bytes(16))
    d_a, d_b = dev(R.encode_scalars([3, 4]) + bytes(16)), dev(R.encode_scalars([5, 6]) + bytes(16))
    d_out = torch.full((224,), 0xA5, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    p, q, a, b, o = d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr()

    def call(p=p, q=q, a=a, b=b, n=2, sa=32, sb=32, form=V.WIRE, out=o):
        return lib.msm377_g1_batch_lincomb2_device(ctx, p, q, a, b, n, sa, sb, form, out, d_inf.data_ptr())

    assert call(n=0) == 0  # n = 0: no launch
    assert call(p=None, q=None, a=None, b=None, n=0, sa=0, sb=0, form=V.MONT_FLAG, out=None) == 0
    assert call(form=V.MONT) == EINVAL  # plain mont cannot say "identity"
    assert call(n=0, form=V.MONT) == EINVAL
    assert call(form=3) == EINVAL
    for stride in (1, 4, 16, 31, 33, 64):
        assert call(sa=stride) == EINVAL, stride
        assert call(sb=stride) == EINVAL, stride
        assert call(sa=0, sb=stride) == EINVAL, stride
    for name in ("p", "q", "a", "b", "out"):
        assert call(**{name: None}) == EINVAL, name
    for name, ptr in (("p", p), ("q", q), ("a", a), ("b", b), ("out", o)):  # alignment: 16 bytes for 96-byte records and scalars
        assert call(**{name: ptr + 8}) == EINVAL, name
    assert call(form=V.MONT_FLAG, out=o + 4) == EINVAL  # 8 bytes for 104-byte records
    with input_format(engine, "mont_flag", "wire"):
        assert call(p=p + 4, n=1) == EINVAL
        assert call(q=q + 4, n=1) == EINVAL
    host = lib.msm377_g1_batch_lincomb2
    assert host(ctx, None, None, None, None, 2, 32, 32, V.WIRE, None, None) == EINVAL
    assert host(ctx, None, None, None, None, 2, 8, 32, V.WIRE, None, None) == EINVAL
    assert host(ctx, None, None, None, None, 2, 32, 8, V.WIRE, None, None) == EINVAL
    assert host(ctx, None, None, None, None, 0, 32, 0, V.WIRE, None, None) == 0
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 224 and bytes(d_inf.cpu().numpy()) == b"\xa5" * 16
    exp, _ = LV.expected(pts, qts, [3, 4], [5, 6])
    got, flags = run_device(engine, R.encode_points(pts), R.encode_points(qts), R.encode_scalars([3, 4]), R.encode_scalars([5, 6]), flags=False)  # d_out_inf may be null
    assert got == exp and flags == b"\xee\xee"
    assert call(form=V.MONT_FLAG, out=o + 8) == 0  # an 8-byte aligned mont_flag output is fine
    assert bytes(d_out.cpu().numpy())[8 : 8 + 208] == V.mont_flag_records(exp, b"\x00\x00")
