"""Multi-base batch multiplication on the GPU (include/msm377.h "multi-base batch multiplication";
csrc/kernels/batch_mul_multi.hpp): out[i] = sum_j [s_ij]B_j through msm377_g1_batch_mul_multi_device /
msm377_g1_batch_mul_multi for both window widths and the rule.  Expected values: tests/pyref.py (every relation between
the bases, every exceptional base) and the host twin (which tests/test_batch_mul_multi_host.py pins to pyref, and whose
output is probed against pyref again here); at scale, one MSM over the outputs with random weights against the oracle's
closed form.  No expected value comes from the device call.  Every test leaves the engine at the rule (width 0) and at
(wire, wire)."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import batch_mul_multi_vectors as MV
import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

pytestmark = pytest.mark.gpu

r = R.R_ORDER
BLOCK = 1024  # outputs per workgroup product tree of the normalisation (4 per thread, 256 threads)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)  # around a wave, a workgroup, a thread's outputs, a tree
THREE = (R.G, R.mul(R.G, MV.M), R.FIXED_BASE)


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


@contextlib.contextmanager
def window(engine, bits):
    engine.set_mul_window(bits)
    try:
        yield
    finally:
        engine.set_mul_window(0)


def run_device(engine, bases: bytes, buf: bytes, n, out_stride=None, base_stride=32, out_form="wire", flags=True):
    """(records, flag bytes) of one device call on freshly poisoned output buffers."""
    import torch

    stride = 104 if out_form == "mont_flag" else 96
    d_s = dev(buf)
    d_out = torch.full((max(16, stride * n),), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((max(16, n),), 0xEE, dtype=torch.uint8, device="cuda")
    engine.batch_mul_multi_device(bases, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr() if flags else 0, out_form, out_stride, base_stride)
    return bytes(d_out.cpu().numpy()[: stride * n]), bytes(d_inf.cpu().numpy()[:n])


def run_rows(engine, points, rows, layout="rows", out_form="wire"):
    buf, out_stride, base_stride = MV.pack(rows, layout)
    return run_device(engine, MV.bases_bytes(points), buf, len(rows), out_stride, base_stride, out_form)


# ---- GPU == host twin (== pyref at a probe set) ----
@pytest.fixture(scope="module")
def size_reference():
    """k -> (rows, wire, flags) of the host twin for the largest size; every size takes a prefix (row-major rows)."""
    out = {}
    probe = [0, 1, 2, 3, 4, 5, 6, 7, 64, 1024, 4096]
    for k in (2, 3):
        rows = MV.many_rows(k, max(SIZES), 0xF1BA5E + k)
        wire, flags = msm.batch_mul_multi_host(MV.bases_bytes(THREE[:k]), MV.pack(rows)[0])
        exp = MV.expected(THREE[:k], [rows[i] for i in probe])
        assert b"".join(wire[96 * i : 96 * i + 96] for i in probe) == exp[0] and bytes(flags[i] for i in probe) == exp[1]
        out[k] = (rows, wire, flags)
    return out


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("width", V.WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin(engine, size_reference, n, width, k):
    rows, wire, flags = size_reference[k]
    with window(engine, width):
        got, got_flags = run_rows(engine, THREE[:k], rows[:n])
        assert engine.last_mul_window() == width
    assert got_flags == flags[:n]
    assert got == wire[: 96 * n]


@pytest.mark.parametrize("width", V.WIDTHS)
def test_one_base_is_the_single_base_call(engine, width):
    """k = 1: byte for byte what msm377_g1_batch_mul_device returns, records and flags."""
    import torch

    n = 257
    scalars = (V.EDGE + V.random_scalars(0x0B1, n))[:n]
    buf = R.encode_scalars(scalars)
    base = V.base_bytes(dict(V.bases())["G_plus_torsion"])
    with window(engine, width):
        for out_form, stride in (("wire", 96), ("mont_flag", 104)):
            d_s = dev(buf)
            d_out = torch.full((stride * n,), 0xEE, dtype=torch.uint8, device="cuda")
            d_inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
            engine.batch_mul_device(base, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), out_form)
            single = (bytes(d_out.cpu().numpy()), bytes(d_inf.cpu().numpy()))
            assert run_device(engine, base, buf, n, out_form=out_form) == single
            assert engine.last_mul_window() == width
    assert single[1][0] == 1 and single[1][1] == 0  # scalars 0 and 1


def test_layouts(engine, size_reference):
    """Rows, columns and padded rows of one matrix: identical bytes.  n = 257, k = 3."""
    rows, wire, flags = size_reference[3]
    n = 257
    for width in V.WIDTHS:
        with window(engine, width):
            for layout in ("rows", "columns", "padded"):
                assert run_rows(engine, THREE, rows[:n], layout) == (wire[: 96 * n], flags[:n]), (width, layout)


# ---- relations between the bases, exceptional bases ----
@pytest.fixture(scope="module")
def relation_reference():
    rows = MV.gpu_rows(130)
    return {name: (pts, rows) + MV.expected(pts, rows)[:2] for name, pts in MV.tuples()}


@pytest.mark.parametrize("width", V.WIDTHS)
@pytest.mark.parametrize("name", [name for name, _ in MV.tuples()])
def test_every_relation_between_the_bases(engine, relation_reference, name, width):
    pts, rows, wire, flags = relation_reference[name]
    with window(engine, width):
        got, got_flags = run_rows(engine, pts, rows)
        assert got_flags == flags, name
        assert got == wire, name
        got, got_flags = run_rows(engine, pts, rows, out_form="mont_flag")
        assert got_flags == flags, name
        assert got == V.mont_flag_records(wire, flags), name
    assert 1 in flags and 0 in flags  # the identity comes out with flag 1
    if name in ("G_mG", "G_negG", "G_G"):  # a sum of O with neither term O
        i = {"G_mG": 0, "G_negG": 2, "G_G": 4}[name]
        assert flags[i] == 1 and flags[i + 1] == 0 and all(R.mul(b, s) is not None for b, s in zip(pts, rows[i]))
    if name == "small3_small3":  # (0, 1), order 3: the wire identity's bytes with flag 0
        hits = [i for i in range(len(rows)) if wire[96 * i : 96 * i + 96] == V.IDENTITY_WIRE and flags[i] == 0]
        assert hits and all((rows[i][0] + rows[i][1]) % 3 == 1 for i in hits)


# ---- identity outputs inside product trees, made by cancelling pairs ----
@pytest.mark.parametrize("width", V.WIDTHS)
def test_identity_outputs_leave_their_neighbours_exact(engine, width):
    n = 3 * BLOCK + 7
    pts = (R.G, R.mul(R.G, MV.M))
    rows = MV.many_rows(2, n, 0x1DE48)[7:] + MV.many_rows(2, 7, 0x1DE49, bits=128)
    ts = V.random_scalars(0x1DE4A, 3, bits=230)
    where = [0, n - 1, 255, 256, BLOCK - 1, 2 * BLOCK, 3 * BLOCK] + list(range(BLOCK, 2 * BLOCK))  # one whole workgroup's outputs
    where += [2 * BLOCK + 5 + 256 * j for j in range(4)]  # all four outputs of one thread
    for k, i in enumerate(where):
        t = ts[k % 3] + k
        rows[i] = (MV.M * t, r - t)  # [M t]G + [r - t][M]G = O, neither term O
    wire, flags = msm.batch_mul_multi_host(MV.bases_bytes(pts), MV.pack(rows)[0])
    assert flags == bytes(1 if i in set(where) else 0 for i in range(n))
    probe = [0, 1, 254, 257, BLOCK - 2, BLOCK, 2 * BLOCK - 1, 2 * BLOCK + 1, n - 2, n - 1]
    exp = MV.expected(pts, [rows[i] for i in probe])
    assert b"".join(wire[96 * i : 96 * i + 96] for i in probe) == exp[0]
    with window(engine, width):
        for out_form in ("wire", "mont_flag"):
            got, got_flags = run_rows(engine, pts, rows, out_form=out_form)
            assert got_flags == flags, out_form
            assert got == (wire if out_form == "wire" else V.mont_flag_records(wire, flags)), out_form


# ---- scale: every output enters one MSM with a random weight ----
SCALE_B = (0x5CA1E0B0, 0x5CA1E0B1F, 0x5CA1E0B22)  # B_j = [b_j]G


@functools.lru_cache(maxsize=None)
def scale_bases(k):
    return MV.bases_bytes([R.mul(R.G, b) for b in SCALE_B[:k]])


@functools.lru_cache(maxsize=2)
def scale_inputs(n, k):
    """(row-major scalar bytes s_ij in [1, 2^252), weight bytes t_i below 2^64, sum_i t_i sum_j s_ij b_j)."""
    rng = np.random.default_rng(0x5CA1E + 16 * n + k)
    s = rng.integers(0, 256, size=(n, k, 32), dtype=np.uint8)
    s[:, :, 31] &= 0x0F  # below 2^252 < r
    s[:, :, 0] |= 1      # not zero
    t = rng.integers(1, 2**63, size=n, dtype=np.uint64)
    tw = np.zeros((n, 4), dtype=np.uint64)
    tw[:, 0] = t
    sb = s.tobytes()
    ti = t.tolist()
    total = 0
    for j in range(k):
        col = s[:, j, :].tobytes()
        total += SCALE_B[j] * sum(w * int.from_bytes(col[32 * i : 32 * i + 32], "little") for i, w in enumerate(ti))
    return sb, tw.tobytes(), total, ti


def weighted_sum(engine, d_points, tb, lo, hi):
    d_t = dev(tb[32 * lo : 32 * hi])
    return engine.msm_device(d_points.data_ptr() + 96 * lo, d_t.data_ptr(), hi - lo)


@pytest.mark.parametrize("width", V.WIDTHS + (0,))
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n", [65537, (1 << 18) + 3])
def test_scale(engine, oracle, n, k, width):
    import torch

    sb, tb, total, _ = scale_inputs(n, k)
    d_s = dev(sb)
    d_out = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    with window(engine, width):
        engine.batch_mul_multi_device(scale_bases(k), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
        assert engine.last_mul_window() == (width or 8)  # the rule takes the wide tables from 2^19 outputs on
    assert not d_inf.any().item()
    assert weighted_sum(engine, d_out, tb, 0, n) == util.closed_form(oracle, total)


def test_passes_past_the_context_capacity(engine, oracle):
    """n = 2^20 + 1, k = 2, COLUMN-major, width 8, on an engine created for 2^16 points: two passes, the second of one
    output.  Column j starts 32 n bytes after column j - 1 in BOTH passes: an offset computed from the pass's length
    instead of the call's n reads the wrong scalars here."""
    import torch

    n = (1 << 20) + 1
    sb, tb, _, ti = scale_inputs(n, 2)
    rows = np.frombuffer(sb, dtype=np.uint8).reshape(n, 2, 32)
    cols = np.ascontiguousarray(rows.transpose(1, 0, 2)).tobytes()
    c0, c1 = cols[: 32 * n], cols[32 * n :]
    s0 = [int.from_bytes(c0[32 * i : 32 * i + 32], "little") for i in (n - 1,)]
    s1 = [int.from_bytes(c1[32 * i : 32 * i + 32], "little") for i in (n - 1,)]
    last_total = SCALE_B[0] * s0[0] + SCALE_B[1] * s1[0]
    _, _, total, _ = scale_inputs(n, 2)
    d_s = dev(cols)
    d_out = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    with msm.MsmEngine(1 << 16) as small:
        small.set_mul_window(8)
        small.batch_mul_multi_device(scale_bases(2), d_s.data_ptr(), n, d_out.data_ptr(), 0, "wire", 32, 32 * n)
        assert small.last_mul_window() == 8
        assert small.mul_multi_table_builds() == 2 and small.mul_table_builds() == 0
    # the session engine holds 2^20 points: the first 2^20 outputs in one MSM, then the last output on its own
    assert weighted_sum(engine, d_out, tb, 0, 1 << 20) == util.closed_form(oracle, total - ti[n - 1] * last_total)
    assert bytes(d_out[96 * (n - 1) :].cpu().numpy()) == util.closed_form(oracle, last_total)


# ---- the table slots ----
def test_slots_are_kept_per_position(engine):
    rows = MV.many_rows(3, 64, 0x510751)
    g, h, h2, f = (R.mul(R.G, m) for m in (0x51A7E0, 0x51A7E1, 0x51A7E2, 0x51A7E3))
    two = [row[:2] for row in rows]
    e_gh = msm.batch_mul_multi_host(MV.bases_bytes((g, h)), MV.pack(two)[0])
    e_gh2 = msm.batch_mul_multi_host(MV.bases_bytes((g, h2)), MV.pack(two)[0])
    e_gh2f = msm.batch_mul_multi_host(MV.bases_bytes((g, h2, f)), MV.pack(rows)[0])
    e_g = msm.batch_mul_host(V.base_bytes(g), R.encode_scalars([row[0] for row in rows]))
    single = engine.mul_table_builds()
    with window(engine, 8):
        before = engine.mul_multi_table_builds()
        assert run_rows(engine, (g, h), two) == e_gh
        assert engine.mul_multi_table_builds() == before + 2  # cold: both slots
        assert run_rows(engine, (g, h), two) == e_gh
        assert run_rows(engine, (g, h), two, out_form="mont_flag")[1] == e_gh[1]
        assert engine.mul_multi_table_builds() == before + 2  # the same again: none
        assert run_rows(engine, (g, h2), two) == e_gh2
        assert engine.mul_multi_table_builds() == before + 3  # slot 1 alone
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.mul_multi_table_builds() == before + 4  # slot 2 alone
        assert run_rows(engine, (g,), [row[:1] for row in rows]) == e_g
        assert engine.mul_multi_table_builds() == before + 4  # k = 1 on slot 0: none; slots 1 and 2 are left as they are
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.mul_multi_table_builds() == before + 4
        # a refused call (a coordinate of p at position 1) changes nothing: not the counter, not a later result
        bad = MV.bases_bytes((g,)) + (R.P).to_bytes(48, "little") + R.G[1].to_bytes(48, "little") + MV.bases_bytes((f,))
        with pytest.raises(msm.MsmError) as e:
            run_device(engine, bad, MV.pack(rows)[0], len(rows))
        assert e.value.code == EINVAL
        assert engine.mul_multi_table_builds() == before + 4
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.mul_multi_table_builds() == before + 4
        engine.set_mul_window(16)
        assert run_rows(engine, (g, h2), two) == e_gh2
        assert engine.mul_multi_table_builds() == before + 6  # the width is part of the key: the slots used, not slot 2
        engine.set_mul_window(8)
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.mul_multi_table_builds() == before + 8  # slots 0 and 1 back at width 8; slot 2 was never touched
    assert engine.mul_table_builds() == single  # the single-base table did not move throughout


def test_neighbours_survive(engine, oracle):
    """The resident MSM bases, a check call and the single-base table on either side of the new call."""
    n = 1000
    points = util.oracle_gen_points(oracle, n, 0x1234567, 0x89AB)
    ks = R.encode_scalars(R.rand_scalars(0x4E51, n))
    d_p, d_k = dev(points), dev(ks)
    exp = util.oracle_msm(oracle, points, ks)
    engine.set_bases_device(d_p.data_ptr(), n)
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp
    rows = MV.many_rows(2, 300, 0x4E53)
    pts = (R.mul(R.G, 0xD00D), R.FIXED_BASE)
    e_multi = msm.batch_mul_multi_host(MV.bases_bytes(pts), MV.pack(rows)[0])
    other = V.base_bytes(R.mul(R.G, 0xD00F))  # the single-base call's base: another one
    buf = R.encode_scalars([row[0] for row in rows])
    e_single = msm.batch_mul_host(other, buf)

    def single():
        import torch

        d_s = dev(buf)
        d_out = torch.full((96 * 300,), 0xEE, dtype=torch.uint8, device="cuda")
        d_inf = torch.full((300,), 0xEE, dtype=torch.uint8, device="cuda")
        engine.batch_mul_device(other, d_s.data_ptr(), 300, d_out.data_ptr(), d_inf.data_ptr())
        return bytes(d_out.cpu().numpy()), bytes(d_inf.cpu().numpy())

    for width in V.WIDTHS:
        with window(engine, width):
            assert single() == e_single
            builds = engine.mul_table_builds()
            assert run_rows(engine, pts, rows) == e_multi
            assert single() == e_single
            assert engine.mul_table_builds() == builds  # the same result and no extra single-base build
        assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp
    rep = engine.check_points_device(d_p.data_ptr(), n)  # a check call in between: neither state touches the other
    assert rep.ok
    assert run_rows(engine, pts, rows) == e_multi
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp


# ---- Montgomery scalars ----
@pytest.mark.parametrize("width", V.WIDTHS)
def test_montgomery_scalars(engine, width):
    n = 257
    values = ([0, 1, r - 1, r, r + 1, 2**256 - 1, 2**255] + V.random_scalars(0x30A8, 2 * n))[: 2 * n]
    rows = list(zip(values[:n], values[n:]))
    reduced = [tuple(v * pow(2**256, -1, r) % r for v in row) for row in rows]
    pts = THREE[:2]
    exp = msm.batch_mul_multi_host(MV.bases_bytes(pts), MV.pack(reduced)[0])
    with window(engine, width):
        assert run_rows(engine, pts, reduced) == exp
        engine.set_input_format("wire", "mont")
        try:
            assert run_rows(engine, pts, rows) == exp
            assert run_rows(engine, pts, rows, "columns") == exp
            assert engine.batch_mul_multi(MV.bases_bytes(pts), MV.pack(rows)[0]) == exp
        finally:
            engine.set_input_format("wire", "wire")


# ---- MONT_FLAG records feed set_bases / msm on a mont_flag context ----
@pytest.mark.parametrize("width", V.WIDTHS)
def test_mont_flag_round_trip(engine, oracle, width):
    import torch

    n = 257
    bs = (1, MV.M)  # (G, [M]G)
    rows = [tuple(s % r for s in row) for row in MV.many_rows(2, n, 0xF1A7)]
    identities = {0, 63, 64, 128, 256}
    for k, i in enumerate(sorted(identities)):
        rows[i] = (MV.M * (k + 2), r - (k + 2))
    weights = R.rand_scalars(0x7E17, n)
    d_s, d_t = dev(MV.pack(rows)[0]), dev(R.encode_scalars(weights))
    d_out = torch.empty(104 * n, dtype=torch.uint8, device="cuda")
    with window(engine, width):
        engine.batch_mul_multi_device(MV.bases_bytes(THREE[:2]), d_s.data_ptr(), n, d_out.data_ptr(), 0, "mont_flag")
    exp = util.closed_form(oracle, sum(t * (row[0] * bs[0] + row[1] * bs[1]) for row, t in zip(rows, weights)))
    engine.set_input_format("mont_flag", "wire")
    try:
        assert engine.msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == exp
        engine.set_bases_device(d_out.data_ptr(), n)
        assert engine.msm_fixed_base_device(d_t.data_ptr(), n) == exp
    finally:
        engine.set_input_format("wire", "wire")
    flags = bytes(d_out.cpu().numpy()[96::104])
    assert flags == bytes(1 if i in identities else 0 for i in range(n))


# ---- the host-buffer call ----
@pytest.mark.parametrize("width", V.WIDTHS)
@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_host_buffer_call(engine, size_reference, layout, width):
    rows, wire, flags = size_reference[3]
    n = 1025
    bases = MV.bases_bytes(THREE)
    buf = MV.pack(rows[:n], layout)[0]
    with window(engine, width):
        assert engine.batch_mul_multi(bases, buf, "wire", layout) == (wire[: 96 * n], flags[:n])
        assert engine.batch_mul_multi(bases, buf, "mont_flag", layout) == (V.mont_flag_records(wire[: 96 * n], flags[:n]), flags[:n])
        assert engine.batch_mul_multi(bases, b"", "wire", layout) == (b"", b"")
        assert engine.last_mul_window() == width


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_host_buffer_call_past_one_piece(layout):
    """k = 16, n = 65 537: the host-buffer call works in pieces of 2^20 / k = 65 536 rows, so its loop runs twice and the
    second piece is ONE row.  Records and flags are the device call's on the same inputs, byte for byte (the tests above
    pin the device call), on poisoned buffers: a piece that is not repacked, uploaded or downloaded shows.  One width
    for the whole call: the width a device call of n rows picks, and 16 builds on a fresh engine -- a second width for the
    second piece would build 16 more."""
    k, n = 16, 65537
    bases = MV.bases_bytes([R.mul(R.G, 0xB16B00 + j) for j in range(k)])
    s = np.random.default_rng(0x16B45E5).integers(0, 256, size=(n, k, 32), dtype=np.uint8)
    s[7] = 0
    s[65535] = 0  # identity outputs: one early, one in the last row of the first piece
    if layout == "rows":
        buf, out_stride, base_stride = s.tobytes(), 32 * k, 32
    else:
        buf, out_stride, base_stride = np.ascontiguousarray(s.transpose(1, 0, 2)).tobytes(), 32, 32 * n
    out, inf = ctypes.create_string_buffer(b"\xee" * (96 * n), 96 * n), ctypes.create_string_buffer(b"\xee" * n, n)
    with msm.MsmEngine(1 << 10) as fresh:
        rc = msm.load_library().msm377_g1_batch_mul_multi(fresh._ctx, bases, k, buf, n, out_stride, base_stride, V.WIRE, ctypes.addressof(out), ctypes.addressof(inf))
        assert rc == 0
        host_width = fresh.last_mul_window()
        assert fresh.mul_multi_table_builds() == 16 and fresh.mul_table_builds() == 0
        wire, flags = run_device(fresh, bases, buf, n, out_stride, base_stride)
        assert fresh.last_mul_window() == host_width
        assert fresh.mul_multi_table_builds() == 16
    assert inf.raw == flags and flags[7] == 1 and flags[65535] == 1 and flags[n - 1] == 0
    assert out.raw == wire


# ---- arguments ----
def test_arguments(engine):
    import torch

    lib = msm.load_library()
    ctx = engine._ctx
    d_s = dev(R.encode_scalars(list(range(3, 3 + 36))))
    d_out = torch.full((208,), 0xA5, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
    builds, single = engine.mul_multi_table_builds(), engine.mul_table_builds()
    ms = [0xE1A70 + j for j in range(17)]
    fresh = MV.bases_bytes([R.mul(R.G, m) for m in ms])

    def call(bases, k, s, n, out_stride, base_stride, form, out):
        return lib.msm377_g1_batch_mul_multi_device(ctx, bases, k, s, n, out_stride, base_stride, form, out, d_inf.data_ptr())

    s, o = d_s.data_ptr(), d_out.data_ptr()
    assert call(fresh, 2, s, 0, 64, 32, V.WIRE, o) == 0  # n = 0: no launch, no table
    assert call(None, 2, None, 0, 64, 32, V.MONT_FLAG, None) == 0
    assert call(fresh, 0, s, 0, 64, 32, V.WIRE, o) == EINVAL  # the shape is checked first, also for n = 0
    assert call(fresh, 0, s, 2, 64, 32, V.WIRE, o) == EINVAL
    assert call(fresh, 17, s, 2, 32 * 17, 32, V.WIRE, o) == EINVAL
    assert call(fresh, 2, s, 2, 0, 32, V.WIRE, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 0, V.WIRE, o) == EINVAL
    assert call(fresh, 2, s, 2, 48, 32, V.WIRE, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 48, V.WIRE, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 32, V.MONT, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 32, 3, o) == EINVAL
    assert call(None, 2, s, 2, 64, 32, V.WIRE, o) == EINVAL
    assert call(fresh, 2, None, 2, 64, 32, V.WIRE, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 32, V.WIRE, None) == EINVAL
    assert call(fresh, 2, s + 4, 2, 64, 32, V.WIRE, o) == EINVAL  # alignment
    noncanonical = fresh[:96] + (R.P).to_bytes(48, "little") + R.G[1].to_bytes(48, "little")
    assert call(noncanonical, 2, s, 2, 64, 32, V.WIRE, o) == EINVAL
    assert lib.msm377_g1_batch_mul_multi(ctx, fresh, 2, None, 2, 64, 32, V.WIRE, None, None) == EINVAL
    assert lib.msm377_g1_batch_mul_multi(ctx, fresh, 17, None, 0, 64, 32, V.WIRE, None, None) == EINVAL
    assert lib.msm377_g1_batch_mul_multi(ctx, fresh, 2, None, 0, 64, 32, V.WIRE, None, None) == 0
    assert engine.mul_multi_table_builds() == builds and engine.mul_table_builds() == single
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 208 and bytes(d_inf.cpu().numpy()) == b"\xa5" * 16
    # the largest k, d_out_inf null, padded rows of 18 scalars
    got, flags = run_device(engine, fresh[: 96 * 16], bytes(d_s.cpu().numpy()), 2, 32 * 18, 32, flags=False)
    exp = [R.mul(R.G, sum(ms[j] * (3 + 18 * i + j) for j in range(16))) for i in range(2)]
    assert got == R.encode_points(exp) and flags == b"\xee\xee"
    assert engine.mul_multi_table_builds() == builds + 16 and engine.mul_table_builds() == single
