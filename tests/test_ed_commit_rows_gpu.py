"""Edwards-BLS12 row commitments on the GPU (include/msm377.h "Edwards-BLS12 row commitments";
csrc/kernels/ed_commit_rows.hpp): out[i] = sum_j [s_ij]G_j over a resident generator set through msm377_ed_set_generators /
msm377_ed_commit_rows_device / msm377_ed_commit_rows.  Expected values: tests/pyref.py (the relations set, the table
records), the host twin (which tests/test_ed_commit_rows_host.py pins to pyref), generators with known logarithms
(tests/ed_commit_rows_vectors.py) and the CPU oracle's Edwards MSM; at scale, one MSM over the outputs with random weights
against the closed form.  No expected value comes from the device call.  Every test drops the set before it returns and
leaves the engine at the rule (width 0) and at (wire, wire)."""
import contextlib
import ctypes

import numpy as np
import pytest

import commit_rows_vectors as CR
import ed_batch_mul_vectors as EV
import ed_commit_rows_vectors as ECR
import pyref as R
import record_model as RM
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, EPOINT, ESTATE

pytestmark = pytest.mark.gpu

ORD = R.ED_SUBGROUP
# around one, two and three segments, an uneven last one, and the one- against the two-level fold (S = 16, 17, 18)
KS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 257, 272, 273)
NS = (1, 63, 64, 65, 255, 256, 257, 1025)  # around a wave, a workgroup, a product tree
WIDE_KS = (1, 17, 33)


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


@contextlib.contextmanager
def generators(engine, gens: bytes, window_bits=0):
    """The set for the length of a test; dropped on the way out whatever happens."""
    try:
        engine.ed_set_generators(gens, window_bits)
        yield
    finally:
        engine.ed_set_generators(None)
        assert engine.ed_generators() == (0, 0)


def run_device(engine, buf: bytes, n, k, out_stride=None, base_stride=32):
    """The records of one device call on a freshly poisoned output buffer, which must stay poisoned behind them."""
    import torch

    d_s = dev(buf)
    d_out = torch.full((64 * n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.ed_commit_rows_device(d_s.data_ptr(), n, k, d_out.data_ptr(), out_stride, base_stride)
    out = bytes(d_out.cpu().numpy())
    assert out[64 * n :] == b"\xee" * 64
    return out[: 64 * n]


def run_rows(engine, rows, layout="rows"):
    buf, out_stride, base_stride = ECR.pack(rows, layout)
    return run_device(engine, buf, len(rows), len(rows[0]), out_stride, base_stride)


def code_of(call, *args, **kw):
    with pytest.raises(msm.MsmError) as e:
        call(*args, **kw)
    return e.value.code


def records(wire):
    return [wire[i : i + 64] for i in range(0, len(wire), 64)]


# ---- GPU == host twin ----
_twin = {}


def twin_reference(k):
    """(generator bytes, sliding buffer, wire) of the host twin over max(NS) sliding rows (full-width, short and zero
    scalars: ECR.mixed_buffer); every size takes a prefix.  One reference per k, computed when first asked for and shared
    by both widths."""
    if k not in _twin:
        n = max(NS)
        _, gens = ECR.known_logs(k)
        buf = ECR.mixed_buffer(n + k - 1, 0x51E5 + k, 8 if k <= 64 else 32)  # (the twin prices 280 000 terms at k = 273)
        _twin[k] = (gens, buf, _sliding_twin(gens, buf, n, k))
    return _twin[k]


def _sliding_twin(gens, buf, n, k):
    """The twin on the sliding layout itself (out_stride = base_stride = 32): no n x k copy of the buffer."""
    out = ctypes.create_string_buffer(64 * n)
    assert msm.load_library().msm377_ed_commit_rows_host(gens, k, ECR.sliding_bytes(buf), n, 32, 32, ctypes.addressof(out)) == 0
    return out.raw


@pytest.mark.parametrize("k,width", [(k, 8) for k in KS] + [(k, 16) for k in WIDE_KS])
def test_sizes_against_host_twin(engine, k, width):
    gens, buf, wire = twin_reference(k)
    data = ECR.sliding_bytes(buf)
    with generators(engine, gens, width):
        assert engine.ed_generators() == (k, width)
        for n in NS:
            got = run_device(engine, data, n, k, 32, 32)  # sliding rows: row i = buf[i : i + k]
            assert got == wire[: 64 * n], n


# ---- relations between the generators, exceptional generators: the walk's and the fold's cases ----
@pytest.mark.parametrize("width", EV.WIDTHS)
def test_relations(engine, width):
    gens = R.ed_encode_points(list(ECR.relation_generators()))
    names = [name for name, _ in ECR.relation_rows()]
    rows = [row for _, row in ECR.relation_rows()]
    wire = ECR.relation_expected()
    assert ECR.plan(ECR.REL_K)[:2] == (18, 16)  # the layout of the set assumes segments of 16 and fold groups 0..15, 16..17
    if width == 16:  # 16-bit tables stop at 64 generators: the set's first 64 (four segments, one fold level), rows cut to match
        k = 64
        keep = [i for i, row in enumerate(rows) if not any(row[k:])]
        assert {"opposite_partials_in_group", "multiple_cancels_in_group", "equal_partials_in_group", "order2_twice", "order4_pair"} <= {names[i] for i in keep}
        gens, names, rows = gens[: 64 * k], [names[i] for i in keep], [rows[i][:k] for i in keep]
        wire = b"".join(records(wire)[i] for i in keep)
    with generators(engine, gens, width):
        for layout in ("rows", "columns"):
            got = run_rows(engine, rows, layout)
            bad = [names[i] for i in range(len(rows)) if records(got)[i] != records(wire)[i]]
            assert not bad, (layout, bad)


# ---- layouts, k below the set ----
def test_layouts_and_a_prefix_of_the_set(engine):
    """Resident k = 33, calls with k = 20 (two segments of 10): rows, columns, padded and sliding layouts of one matrix give
    identical bytes; scalars past k are never read."""
    n, k, resident = 257, 20, 33
    _, gens = ECR.known_logs(resident)
    buf = ECR.mixed_buffer(n + k - 1, 0x1A70)
    rows = ECR.sliding_rows(buf, n, k)
    exp = msm.ed_commit_rows_host(gens[: 64 * k], ECR.pack(rows)[0])
    poison = EV.random_scalars(0xBAD5EED, resident - k)
    wide_rows = [row + tuple(p | 1 for p in poison) for row in rows]  # 33 scalars a row; the last 13 belong to no generator of the call
    with generators(engine, gens):
        for layout in ("rows", "columns", "padded"):
            assert run_rows(engine, rows, layout) == exp, layout
        assert run_device(engine, ECR.sliding_bytes(buf), n, k, 32, 32) == exp
        data, out_stride, base_stride = ECR.pack(wide_rows)
        assert run_device(engine, data, n, k, out_stride, base_stride) == exp
        assert run_device(engine, data, n, resident, out_stride, base_stride) != exp  # (the poison does count at k = 33)


@pytest.mark.parametrize("width", EV.WIDTHS)
def test_one_generator_is_the_single_base_call(engine, width):
    """Resident k = 1: byte for byte what msm377_ed_batch_mul_multi_device returns with k = 1 at that width."""
    import torch

    n = 257
    scalars = (EV.EDGE + EV.random_scalars(0x0B1, n))[:n]
    buf = R.encode_scalars(scalars)
    base = R.ed_encode_points([dict(EV.bases())["P_plus_order4_a"]])
    engine.set_mul_window(width)
    try:
        with generators(engine, base, width):
            d_s = dev(buf)
            d_out = torch.full((64 * n,), 0xEE, dtype=torch.uint8, device="cuda")
            engine.ed_batch_mul_multi_device(base, d_s.data_ptr(), n, d_out.data_ptr())
            assert engine.last_mul_window() == width
            single = bytes(d_out.cpu().numpy())
            assert run_device(engine, buf, n, 1) == single
    finally:
        engine.set_mul_window(0)
    assert single == msm.ed_batch_mul_multi_host(base, buf) and single[:64] == ECR.IDENTITY_WIRE


# ---- large k ----
def weights(n, seed):
    t = np.random.default_rng(seed).integers(1, 2**63, size=n, dtype=np.uint64)
    tw = np.zeros((n, 4), dtype=np.uint64)
    tw[:, 0] = t
    return t.tolist(), tw.tobytes()


def closed_form(total):
    return R.ed_encode_result(R.ed_mul(R.ED_G, total % ORD))


def check_sparse_sliding(engine, k, n, gap, probes, seed):
    """Sparse sliding rows over known-logarithm generators: exact records at ``probes`` and one MSM over all n outputs with
    random weights against the closed form."""
    import torch

    logs, _ = ECR.known_logs(k)
    buf, where = ECR.sparse_sliding(n, k, seed, gap)
    d_s = dev(ECR.sliding_bytes(buf))
    d_out = torch.full((64 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.ed_commit_rows_device(d_s.data_ptr(), n, k, d_out.data_ptr(), 32, 32)
    probes = sorted(set(p for p in probes if 0 <= p < n))
    wire = ECR.multiples_of_g(ECR.closed_sliding(logs, buf, where, probes, k))
    out = d_out.cpu().numpy()
    for t, i in enumerate(probes):
        assert bytes(out[64 * i : 64 * i + 64]) == wire[64 * t : 64 * t + 64], i
    ti, tb = weights(n, seed)
    total = 0
    for p in where:  # sum_i t_i sum_p buf[p] g_(p - i), turned inside out
        lo, hi = max(0, p - k + 1), min(n - 1, p)
        total += buf[p] * sum(ti[i] * logs[p - i] for i in range(lo, hi + 1))
    d_t = dev(tb)
    assert engine.ed_msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == closed_form(total)


def test_4096_generators(engine):
    """k = 4 096 (256 segments, 16 fold groups of 16) at width 8, n = rows per pass + 257: two passes.  Three non-zero
    full-width scalars a row, 1 365 positions apart and so in different segments and fold groups; all-zero walks are skipped
    wave-uniformly."""
    k = ECR.GEN_MAX
    segments, _, rows_per_pass = msm.commit_rows_plan(k)
    assert segments == 256
    n = rows_per_pass + 257
    _, gens = ECR.known_logs(k)
    with generators(engine, gens):
        assert engine.ed_generators() == (k, 8)
        probes = [0, 63, 64, 127, 255, 256, rows_per_pass - 64, rows_per_pass - 1, rows_per_pass, rows_per_pass + 63, rows_per_pass + 64, n - 64, n - 1]
        check_sparse_sliding(engine, k, n, k // 3, probes, 0x4096)


def test_1024_generators_dense(engine, oracle):
    """k = 1 024 (64 segments, four fold groups), n = 8, dense full-width scalars below the order: each output is the
    oracle's Edwards MSM of (generators, row)."""
    k, n = 1024, 8
    _, gens = ECR.known_logs(k)
    rows = [tuple(v % ORD for v in EV.random_scalars(0xDE45E + i, k)) for i in range(n)]
    exp = b"".join(util.oracle_ed_msm(oracle, gens, R.encode_scalars(list(row))) for row in rows)
    with generators(engine, gens):
        assert run_rows(engine, rows) == exp
        assert run_rows(engine, rows, "columns") == exp


def test_pass_boundary_with_two_segments(engine):
    """k = 32 (two segments of 16), n = 2^19 + 257: the second pass starts at row 2^19.  Two non-zero full-width scalars a
    row, 16 positions apart: one in each segment."""
    k = 32
    segments, per_segment, rows_per_pass = msm.commit_rows_plan(k)
    assert (segments, per_segment, rows_per_pass) == (2, 16, 2**19)
    n = rows_per_pass + 257
    _, gens = ECR.known_logs(k)
    with generators(engine, gens):
        probes = [0, 63, 64, 255, 256, rows_per_pass - 64, rows_per_pass - 1, rows_per_pass, rows_per_pass + 63, rows_per_pass + 64, n - 64, n - 1]
        check_sparse_sliding(engine, k, n, 16, probes, 0x32)


# ---- the state of the set ----
def test_state(engine, oracle):
    import torch

    k = 17
    logs, gens = ECR.known_logs(k)
    logs2, gens2 = ECR.known_logs(k, seed=0x2222)
    rows = ECR.sliding_rows(ECR.mixed_buffer(65 + k - 1, 0x57A7E), 65, k)
    data, out_stride, base_stride = ECR.pack(rows)
    exp, exp2 = ECR.closed_rows(logs, rows), ECR.closed_rows(logs2, rows)
    assert exp != exp2
    call = lambda kk=k: run_device(engine, data, 65, kk, out_stride, base_stride)  # noqa: E731
    # a G1 set beside it, for the length of the test
    g1_logs, g1_gens = CR.known_logs(k)
    g1_rows = CR.sliding_rows(CR.sliding_buffer(33, k, 0x61), 33, k)
    g1_data = CR.pack(g1_rows)[0]
    g1_exp = CR.closed_rows(g1_logs, g1_rows)

    def g1_call():
        d_s = dev(g1_data)
        d_out = torch.full((96 * 33,), 0xEE, dtype=torch.uint8, device="cuda")
        d_inf = torch.full((48,), 0xEE, dtype=torch.uint8, device="cuda")
        engine.commit_rows_device(d_s.data_ptr(), 33, k, d_out.data_ptr(), d_inf.data_ptr())
        return bytes(d_out.cpu().numpy()), bytes(d_inf.cpu().numpy()[:33])

    engine.ed_set_generators(None)
    engine.set_generators(None)
    try:
        assert engine.ed_generators() == (0, 0)
        assert code_of(call) == ESTATE  # before any set
        assert code_of(engine.ed_commit_rows, data, k) == ESTATE
        engine.set_generators(g1_gens)
        assert code_of(call) == ESTATE  # a G1 set is not this curve's
        engine.ed_set_generators(gens)
        assert engine.ed_generators() == (k, 8) and engine.generators() == (k, 8) and call() == exp and g1_call() == g1_exp
        assert code_of(call, k + 1) == ESTATE  # above the resident k
        assert call() == exp
        engine.ed_set_generators(gens2)  # a second set is honoured
        assert call() == exp2
        engine.ed_set_generators(b"")
        assert engine.ed_generators() == (0, 0) and code_of(call) == ESTATE  # after a dropped set
        assert engine.generators() == (k, 8) and g1_call() == g1_exp
        # failed sets leave none, and leave the G1 set intact
        engine.ed_set_generators(gens)
        bad = gens[: 64 * 5] + R.ed_encode_points([ECR.off_curve_point()]) + gens[64 * 6 :]
        with pytest.raises(msm.MsmError) as e:
            engine.ed_set_generators(bad)
        assert (e.value.code, e.value.index) == (EPOINT, 5) and "not on the curve" in str(e.value)
        assert engine.ed_generators() == (0, 0) and code_of(call) == ESTATE
        gx, gy = R.ED_G
        noncanon = (gx + R.Q).to_bytes(32, "little") + gy.to_bytes(32, "little")
        with pytest.raises(msm.MsmError) as e:
            engine.ed_set_generators(gens[: 64 * 3] + noncanon + gens[64 * 4 : 64 * 5] + R.ed_encode_points([ECR.off_curve_point()]) + gens[64 * 6 :])
        assert (e.value.code, e.value.index) == (EPOINT, 3) and "not below q" in str(e.value)  # the lowest failing index, and its reason
        engine.ed_set_generators(gens)
        _, many = ECR.known_logs(65)
        assert code_of(engine.ed_set_generators, many, 16) == EINVAL  # 16-bit tables stop at 64 generators
        assert engine.ed_generators() == (0, 0) and code_of(call) == ESTATE
        engine.ed_set_generators(gens)
        assert code_of(engine.ed_set_generators, gens, 12) == EINVAL and engine.ed_generators() == (0, 0)
        assert engine.generators() == (k, 8) and g1_call() == g1_exp
        engine.ed_set_generators(many[: 64 * 64], 16)
        assert engine.ed_generators() == (64, 16) and call() == ECR.closed_rows(ECR.known_logs(65)[0], rows)
        # dropping or failing the G1 set leaves this one alone
        engine.set_generators(None)
        assert engine.ed_generators() == (64, 16) and call() == ECR.closed_rows(ECR.known_logs(65)[0], rows)

        # the neighbours: what they return with both sets resident is what they return with neither
        engine.ed_set_generators(None)
        n = 1000
        points = util.oracle_gen_points(oracle, n, 0x1234567, 0x89AB)
        ks = R.encode_scalars(R.rand_scalars(0x4E51, n))
        d_p, d_k = dev(points), dev(ks)
        exp_msm = util.oracle_msm(oracle, points, ks)
        ed_points = util.oracle_ed_gen_points(oracle, n, 0x7654321, 0xBA98)
        ed_ks = R.encode_scalars(R.rand_scalars(0x4E52, n, ORD >> 2))
        d_ep, d_ek = dev(ed_points), dev(ed_ks)
        exp_ed_msm = util.oracle_ed_msm(oracle, ed_points, ed_ks)
        ed_pts = (R.ED_G, R.ed_mul(R.ED_G, EV.M))
        mrows = EV.many_rows(2, 300, 0x4E53)
        mbuf = EV.pack(mrows)[0]

        def neighbours():
            d_m = dev(mbuf)
            d_out = torch.full((64 * 300,), 0xEE, dtype=torch.uint8, device="cuda")
            out = [engine.msm_device(d_p.data_ptr(), d_k.data_ptr(), n)]
            engine.set_bases_device(d_p.data_ptr(), n)
            out.append(engine.msm_fixed_base_device(d_k.data_ptr(), n))
            engine.ed_batch_mul_multi_device(EV.bases_bytes(ed_pts), d_m.data_ptr(), 300, d_out.data_ptr())
            out.append(bytes(d_out.cpu().numpy()))
            engine.ed_batch_mul_var_device(d_ep.data_ptr(), d_ek.data_ptr(), 300, d_out.data_ptr())
            out.append(bytes(d_out.cpu().numpy()))
            out.append(engine.ed_msm_device(d_ep.data_ptr(), d_ek.data_ptr(), n))
            out.append(engine.check_points_device(d_p.data_ptr(), n).ok)
            out.append(engine.ed_check_points_device(d_ep.data_ptr(), n).ok)
            return out

        without = neighbours()
        assert without[0] == exp_msm and without[1] == exp_msm and without[4] == exp_ed_msm and without[5] and without[6]
        assert without[2] == msm.ed_batch_mul_multi_host(EV.bases_bytes(ed_pts), mbuf) and without[3] == msm.ed_batch_mul_var_host(ed_points[: 64 * 300], ed_ks[: 32 * 300])
        engine.set_generators(g1_gens)
        engine.ed_set_generators(gens)
        builds = lambda: (engine.mul_table_builds(), engine.mul_multi_table_builds(), engine.ed_mul_table_builds())  # noqa: E731
        before = builds()
        assert call() == exp and g1_call() == g1_exp
        assert neighbours() == without
        assert call() == exp and g1_call() == g1_exp  # ... and both sets survive them
        assert builds() == before  # warm tables: no build, and none by commit calls
        engine.ed_set_generators(gens2)
        assert call() == exp2 and g1_call() == g1_exp
        assert builds() == before
        last = engine.last_mul_window()
        engine.set_mul_window(16)  # the width belongs to the set
        try:
            assert call() == exp2 and engine.ed_generators() == (k, 8)
        finally:
            engine.set_mul_window(0)
        assert engine.last_mul_window() == last
    finally:
        engine.ed_set_generators(None)
        engine.set_generators(None)


# ---- refusals ----
def test_refusals(engine):
    import torch

    lib = msm.load_library()
    ctx = engine._ctx
    logs, gens = ECR.known_logs(17)
    d_s = dev(R.encode_scalars(list(range(3, 3 + 40))))
    d_out = torch.full((144,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(s, n, k, out_stride, base_stride, out):
        return lib.msm377_ed_commit_rows_device(ctx, s, n, k, out_stride, base_stride, out)

    s, o = d_s.data_ptr(), d_out.data_ptr()
    engine.ed_set_generators(None)
    try:
        assert call(s, 0, 2, 64, 32, o) == 0  # n = 0 without a set
        assert lib.msm377_ed_commit_rows(ctx, None, 0, 2, 64, 32, None) == 0
        assert call(s, 2, 2, 64, 32, o) == ESTATE
        engine.ed_set_generators(gens)
        assert call(s, 0, 2, 64, 32, o) == 0
        assert call(None, 0, 2, 64, 32, None) == 0
        assert call(s, 0, 0, 64, 32, o) == EINVAL  # the shape is checked first, also for n = 0
        assert call(s, 2, 0, 64, 32, o) == EINVAL
        assert call(s, 2, 4097, 32, 32, o) == EINVAL
        assert call(s, 2, 18, 32, 32, o) == ESTATE
        assert call(s, 2, 2, 0, 32, o) == EINVAL
        assert call(s, 2, 2, 64, 0, o) == EINVAL
        assert call(s, 2, 2, 48, 32, o) == EINVAL
        assert call(s, 2, 2, 64, 48, o) == EINVAL
        assert call(None, 2, 2, 64, 32, o) == EINVAL
        assert call(s, 2, 2, 64, 32, None) == EINVAL
        assert call(s + 4, 2, 2, 64, 32, o) == EINVAL  # alignment
        assert call(s, 2, 2, 64, 32, o + 8) == EINVAL
        assert lib.msm377_ed_commit_rows(ctx, None, 2, 2, 64, 32, None) == EINVAL
        assert lib.msm377_ed_commit_rows(ctx, None, 0, 4097, 64, 32, None) == EINVAL
        assert lib.msm377_ed_set_generators(None, gens, 17, 0) == EINVAL
        host_out = ctypes.create_string_buffer(b"\xa5" * 128, 128)
        for forms in (("mont", "wire"), ("wire", "mont"), ("mont_flag", "mont")):  # the Edwards-BLS12 calls take the wire format only
            engine.set_input_format(*forms)
            try:
                assert call(s, 2, 2, 64, 32, o) == EINVAL
                assert lib.msm377_ed_commit_rows(ctx, bytes(128), 2, 2, 64, 32, ctypes.addressof(host_out)) == EINVAL
                assert lib.msm377_ed_set_generators(ctx, gens, 17, 0) == EINVAL
            finally:
                engine.set_input_format("wire", "wire")
        assert bytes(d_out.cpu().numpy()) == b"\xa5" * 144 and host_out.raw == b"\xa5" * 128
        assert engine.ed_generators() == (17, 8)
        # padded rows of 19 scalars
        got = run_device(engine, bytes(d_s.cpu().numpy()), 2, 17, 32 * 19, 32)
        assert got == ECR.closed_rows(logs, [tuple(range(3 + 19 * i, 3 + 19 * i + 17)) for i in range(2)])
    finally:
        engine.ed_set_generators(None)


# ---- the host-buffer call ----
def test_host_buffer_call(engine):
    n, k = 257, 33
    gens, buf, wire = twin_reference(k)
    rows = ECR.sliding_rows(buf, n, k)
    exp = wire[: 64 * n]
    with generators(engine, gens):
        assert run_rows(engine, rows) == exp
        for layout in ("rows", "columns"):
            assert engine.ed_commit_rows(ECR.pack(rows, layout)[0], k, layout) == exp, layout
        lib = msm.load_library()
        for layout in ("padded", "sliding"):  # the C call: any strides
            data, out_stride, base_stride = (ECR.sliding_bytes(buf), 32, 32) if layout == "sliding" else ECR.pack(rows, layout)
            out = ctypes.create_string_buffer(64 * n)
            assert lib.msm377_ed_commit_rows(engine._ctx, data, n, k, out_stride, base_stride, ctypes.addressof(out)) == 0
            assert out.raw == exp, layout
        assert engine.ed_commit_rows(b"", k) == b""


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_host_buffer_call_past_one_piece(engine, layout):
    """k = 4 096, n = 257: the host-buffer call works in pieces of 2^20 / k = 256 rows, so its loop runs twice and the second
    piece is ONE row.  Records are the device call's on the same inputs, byte for byte (the tests above pin the device
    call), on a poisoned buffer: a piece that is not repacked, uploaded or downloaded shows.  Dense full-width scalars; two
    all-zero rows."""
    k, n = ECR.GEN_MAX, 257
    _, gens = ECR.known_logs(k)
    s = np.random.default_rng(0xC0441715).integers(0, 256, size=(n, k, 32), dtype=np.uint8)
    s[7] = 0
    s[255] = 0  # identity outputs: one early, one in the last row of the first piece
    if layout == "rows":
        buf, out_stride, base_stride = s.tobytes(), 32 * k, 32
    else:
        buf, out_stride, base_stride = np.ascontiguousarray(s.transpose(1, 0, 2)).tobytes(), 32, 32 * n
    out = ctypes.create_string_buffer(b"\xee" * (64 * n), 64 * n)
    with generators(engine, gens):
        assert msm.load_library().msm377_ed_commit_rows(engine._ctx, buf, n, k, out_stride, base_stride, ctypes.addressof(out)) == 0
        wire = run_device(engine, buf, n, k, out_stride, base_stride)
    assert out.raw == wire
    rec = records(wire)
    assert rec[7] == rec[255] == ECR.IDENTITY_WIRE and rec[n - 1] != ECR.IDENTITY_WIRE and b"\xee" * 8 not in wire


# ---- the tables themselves ----
def record_words(pt):
    return [int(w) for coord in RM.ed_make_base(pt) for w in coord] + [0] * 5


@pytest.mark.parametrize("width", EV.WIDTHS)
def test_generator_tables(engine, width):
    """The first, a middle and the carry record of generators 0, 16 and k - 1 of a 33-generator set, word for word
    record_model.ed_make_base([d 2^(c w)]G_j); ESTATE beyond the set and without one."""
    k = 33
    logs, gens = ECR.known_logs(k)
    W, half = EV.windows(width), 1 << (width - 1)
    with generators(engine, gens, width):
        for j in (0, 16, k - 1):
            info, _ = engine.ed_read_generator_table(j, info_only=True)
            assert (info.width, info.rows, info.records, info.key) == (width, W + 1, W * half + 1, bytes(96))
            for w, d in ((0, 1), (W // 2, half - 1), (W, 1)):  # record w * half + d - 1 is [d 2^(c w)]G_j; the last one the carry's
                _, words = engine.ed_read_generator_table(j, first=w * half + d - 1, count=1)
                assert words[0].tolist() == record_words(R.ed_mul(R.ED_G, logs[j] * (d << (width * w)) % ORD)), (j, w, d)
        assert code_of(engine.ed_read_generator_table, k, info_only=True) == ESTATE
        assert code_of(engine.ed_read_generator_table, 0, first=W * half + 1, count=1) == EINVAL
    assert code_of(engine.ed_read_generator_table, 0, info_only=True) == ESTATE
