"""Row commitments on the GPU (include/msm377.h "row commitments"; csrc/kernels/commit_rows.hpp): out[i] = sum_j [s_ij]G_j
over a resident generator set through msm377_g1_set_generators / msm377_g1_commit_rows_device / msm377_g1_commit_rows.
Expected values: tests/pyref.py (the relations set), the host twin (which tests/test_commit_rows_host.py pins to pyref),
generators with known logarithms (tests/commit_rows_vectors.py) and the CPU oracle's MSM; at scale, one MSM over the
outputs with random weights against the closed form.  No expected value comes from the device call.  Every test drops
the set before it returns and leaves the engine at the rule (width 0) and at (wire, wire)."""
import contextlib
import time

import numpy as np
import pytest

import batch_mul_multi_vectors as MV
import batch_mul_vectors as V
import commit_rows_vectors as CR
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, ESTATE

pytestmark = pytest.mark.gpu

r = R.R_ORDER
KS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49)  # around one, two and three segments and an uneven last one
NS = (1, 63, 64, 65, 255, 256, 257, 1025)     # around a wave, a workgroup, a product tree
WIDE_KS = (1, 17, 33)


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


@contextlib.contextmanager
def generators(engine, gens: bytes, window_bits=0):
    """The set for the length of a test; dropped on the way out whatever happens."""
    try:
        engine.set_generators(gens, window_bits)
        yield
    finally:
        engine.set_generators(None)
        assert engine.generators() == (0, 0)


def run_device(engine, buf: bytes, n, k, out_stride=None, base_stride=32, out_form="wire", flags=True):
    """(records, flag bytes) of one device call on freshly poisoned output buffers."""
    import torch

    stride = 104 if out_form == "mont_flag" else 96
    d_s = dev(buf)
    d_out = torch.full((max(16, stride * n),), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((max(16, n),), 0xEE, dtype=torch.uint8, device="cuda")
    engine.commit_rows_device(d_s.data_ptr(), n, k, d_out.data_ptr(), d_inf.data_ptr() if flags else 0, out_form, out_stride, base_stride)
    return bytes(d_out.cpu().numpy()[: stride * n]), bytes(d_inf.cpu().numpy()[:n])


def run_rows(engine, rows, layout="rows", out_form="wire"):
    buf, out_stride, base_stride = CR.pack(rows, layout)
    return run_device(engine, buf, len(rows), len(rows[0]), out_stride, base_stride, out_form)


def code_of(call, *args, **kw):
    with pytest.raises(msm.MsmError) as e:
        call(*args, **kw)
    return e.value.code


# ---- GPU == host twin ----
_twin = {}


def twin_reference(k):
    """(generator bytes, sliding buffer, wire, flags) of the host twin over max(NS) sliding rows of full-width scalars;
    every size takes a prefix.  One reference per k, computed when first asked for."""
    if k not in _twin:
        n = max(NS)
        _, gens = CR.known_logs(k)
        buf = CR.sliding_buffer(n, k, 0x51E5 + k)
        wire, flags = msm.commit_rows_host(gens, CR.pack(CR.sliding_rows(buf, n, k))[0])
        _twin[k] = (gens, buf, wire, flags)
    return _twin[k]


@pytest.mark.parametrize("k,width", [(k, 8) for k in KS] + [(k, 16) for k in WIDE_KS])
def test_sizes_against_host_twin(engine, k, width):
    gens, buf, wire, flags = twin_reference(k)
    data = CR.sliding_bytes(buf)
    with generators(engine, gens, width):
        assert engine.generators() == (k, width)
        for n in NS:
            got, got_flags = run_device(engine, data, n, k, 32, 32)  # sliding rows: row i = buf[i : i + k]
            assert got_flags == flags[:n], n
            assert got == wire[: 96 * n], n


# ---- relations between the generators, exceptional generators: the fold's cases ----
@pytest.mark.parametrize("width", V.WIDTHS)
def test_relations(engine, width):
    gens = R.encode_points(list(CR.relation_generators()))
    names = [name for name, _ in CR.relation_rows()]
    rows = [row for _, row in CR.relation_rows()]
    wire, flags = CR.relation_expected()
    assert CR.plan(CR.REL_K)[:2] == (3, 16)  # the layout of the set assumes segments 0..15, 16..31, 32..47
    with generators(engine, gens, width):
        got, got_flags = run_rows(engine, rows)
        bad = [names[i] for i in range(len(rows)) if got_flags[i] != flags[i] or got[96 * i : 96 * i + 96] != wire[96 * i : 96 * i + 96]]
        assert not bad, bad
        got, got_flags = run_rows(engine, rows, out_form="mont_flag")
        assert got_flags == flags
        assert got == V.mont_flag_records(wire, flags)
        assert bytes(got[104 * i + 96] for i in range(len(flags))) == flags  # the record's own flag byte
        assert run_rows(engine, rows, "columns") == (wire, flags)
    assert flags[names.index("three_cancel")] == 1 and flags[names.index("three_neighbour")] == 0


# ---- layouts, Montgomery scalars, k below the set ----
def test_layouts_and_a_prefix_of_the_set(engine):
    """Resident k = 33, calls with k = 20 (two segments of 10): rows, columns, padded and sliding layouts of one matrix
    give identical bytes; Montgomery scalars equal wire scalars after import; scalars past k are never read."""
    n, k, resident = 257, 20, 33
    _, gens = CR.known_logs(resident)
    buf = CR.sliding_buffer(n, k, 0x1A70)
    rows = CR.sliding_rows(buf, n, k)
    exp = msm.commit_rows_host(gens[: 96 * k], CR.pack(rows)[0])
    inv = pow(2**256, -1, r)
    reduced = [tuple(v * inv % r for v in row) for row in rows]
    exp_mont = msm.commit_rows_host(gens[: 96 * k], CR.pack(reduced)[0])
    poison = V.random_scalars(0xBAD5EED, resident - k)
    wide_rows = [row + tuple(p | 1 for p in poison) for row in rows]  # 33 scalars a row; the last 13 belong to no generator of the call
    with generators(engine, gens):
        for layout in ("rows", "columns", "padded"):
            assert run_rows(engine, rows, layout) == exp, layout
        assert run_device(engine, CR.sliding_bytes(buf), n, k, 32, 32) == exp
        data, out_stride, base_stride = CR.pack(wide_rows)
        assert run_device(engine, data, n, k, out_stride, base_stride) == exp
        assert run_device(engine, data, n, resident, out_stride, base_stride) != exp  # (the poison does count at k = 33)
        assert run_rows(engine, reduced) == exp_mont
        engine.set_input_format("wire", "mont")
        try:
            assert run_rows(engine, rows) == exp_mont
            assert run_rows(engine, rows, "columns") == exp_mont
            assert engine.commit_rows(CR.pack(rows)[0], k) == exp_mont
        finally:
            engine.set_input_format("wire", "wire")
        assert run_rows(engine, rows) == exp


@pytest.mark.parametrize("width", V.WIDTHS)
def test_one_generator_is_the_single_base_call(engine, width):
    """Resident k = 1: byte for byte what msm377_g1_batch_mul_device returns at that width, records and flags."""
    import torch

    n = 257
    scalars = (V.EDGE + V.random_scalars(0x0B1, n))[:n]
    buf = R.encode_scalars(scalars)
    base = V.base_bytes(dict(V.bases())["G_plus_torsion"])
    engine.set_mul_window(width)
    try:
        with generators(engine, base, width):
            for out_form, stride in (("wire", 96), ("mont_flag", 104)):
                d_s = dev(buf)
                d_out = torch.full((stride * n,), 0xEE, dtype=torch.uint8, device="cuda")
                d_inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
                engine.batch_mul_device(base, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), out_form)
                single = (bytes(d_out.cpu().numpy()), bytes(d_inf.cpu().numpy()))
                assert run_device(engine, buf, n, 1, out_form=out_form) == single
    finally:
        engine.set_mul_window(0)
    assert single[1][0] == 1 and single[1][1] == 0  # scalars 0 and 1


# ---- large k ----
def weights(n, seed):
    t = np.random.default_rng(seed).integers(1, 2**63, size=n, dtype=np.uint64)
    tw = np.zeros((n, 4), dtype=np.uint64)
    tw[:, 0] = t
    return t.tolist(), tw.tobytes()


def check_sparse_sliding(engine, oracle, k, n, gap, probes, seed):
    """Sparse sliding rows over known-logarithm generators: exact records at ``probes`` and one MSM over all n outputs with
    random weights against the closed form."""
    import torch

    logs, _ = CR.known_logs(k)
    buf, where = CR.sparse_sliding(n, k, seed, gap)
    d_s = dev(CR.sliding_bytes(buf))
    d_out = torch.full((96 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.commit_rows_device(d_s.data_ptr(), n, k, d_out.data_ptr(), d_inf.data_ptr(), "wire", 32, 32)
    probes = sorted(set(p for p in probes if 0 <= p < n))
    wire, flags = CR.multiples_of_g(CR.closed_sliding(logs, buf, where, probes, k))
    out = d_out.cpu().numpy()
    inf = bytes(d_inf.cpu().numpy())
    for t, i in enumerate(probes):
        assert inf[i] == flags[t] and bytes(out[96 * i : 96 * i + 96]) == wire[96 * t : 96 * t + 96], i
    ti, tb = weights(n, seed)
    total = 0
    for p in where:  # sum_i t_i sum_p buf[p] g_(p - i), turned inside out
        lo, hi = max(0, p - k + 1), min(n - 1, p)
        total += buf[p] * sum(ti[i] * logs[p - i] for i in range(lo, hi + 1))
    d_t = dev(tb)
    assert engine.msm_device(d_out.data_ptr(), d_t.data_ptr(), n) == util.closed_form(oracle, total % r)


def test_4096_generators(engine, oracle):
    """k = 4 096 (256 segments) at width 8, n = rows per pass + 257: two passes.  Three non-zero full-width scalars a row,
    1 365 positions apart and so in different segments; all-zero walks are skipped wave-uniformly."""
    k = CR.GEN_MAX
    segments, _, rows_per_pass = msm.commit_rows_plan(k)
    assert segments == 256
    n = rows_per_pass + 257
    _, gens = CR.known_logs(k)
    t0 = time.perf_counter()
    with generators(engine, gens):
        print("set_generators(k = 4096, c = 8): %.1f ms" % (1e3 * (time.perf_counter() - t0)))
        assert engine.generators() == (k, 8)
        probes = [0, 63, 64, 127, 255, 256, rows_per_pass - 64, rows_per_pass - 1, rows_per_pass, rows_per_pass + 63, rows_per_pass + 64, n - 64, n - 1]
        check_sparse_sliding(engine, oracle, k, n, k // 3, probes, 0x4096)


def test_1024_generators_dense(engine, oracle):
    """k = 1 024, n = 8, dense full-width scalars below r: each output is the oracle's MSM of (generators, row)."""
    k, n = 1024, 8
    _, gens = CR.known_logs(k)
    rows = [tuple(v % r for v in V.random_scalars(0xDE45E + i, k)) for i in range(n)]
    exp = b"".join(util.oracle_msm(oracle, gens, R.encode_scalars(list(row))) for row in rows)
    with generators(engine, gens):
        got, flags = run_rows(engine, rows)
        assert flags == bytes(n)
        assert got == exp
        assert run_rows(engine, rows, "columns") == (exp, bytes(n))


def test_pass_boundary_with_two_segments(engine, oracle):
    """k = 32 (two segments of 16), n = 2^19 + 257: the second pass starts at row 2^19.  Two non-zero full-width scalars a
    row, 16 positions apart: one in each segment."""
    k = 32
    segments, per_segment, rows_per_pass = msm.commit_rows_plan(k)
    assert (segments, per_segment, rows_per_pass) == (2, 16, 2**19)
    n = rows_per_pass + 257
    _, gens = CR.known_logs(k)
    with generators(engine, gens):
        probes = [0, 63, 64, 255, 256, rows_per_pass - 64, rows_per_pass - 1, rows_per_pass, rows_per_pass + 63, rows_per_pass + 64, n - 64, n - 1]
        check_sparse_sliding(engine, oracle, k, n, 16, probes, 0x32)


# ---- the state of the set ----
def test_state(engine, oracle):
    import torch

    k = 17
    logs, gens = CR.known_logs(k)
    logs2, gens2 = CR.known_logs(k, seed=0x2222)
    rows = CR.sliding_rows(CR.sliding_buffer(65, k, 0x57A7E), 65, k)
    data, out_stride, base_stride = CR.pack(rows)
    exp, exp2 = CR.closed_rows(logs, rows), CR.closed_rows(logs2, rows)
    assert exp != exp2
    call = lambda kk=k: run_device(engine, data, 65, kk, out_stride, base_stride)
    engine.set_generators(None)
    try:
        assert engine.generators() == (0, 0)
        assert code_of(call) == ESTATE  # before any set
        assert code_of(engine.commit_rows, data, k) == ESTATE
        engine.set_generators(gens)
        assert engine.generators() == (k, 8) and call() == exp
        assert code_of(call, k + 1) == ESTATE  # above the resident k
        assert call() == exp
        engine.set_generators(gens2)  # a second set is honoured
        assert call() == exp2
        engine.set_generators(b"")
        assert engine.generators() == (0, 0) and code_of(call) == ESTATE  # after a dropped set
        engine.set_generators(gens)
        bad = gens[:96] + (R.P).to_bytes(48, "little") + R.G[1].to_bytes(48, "little") + gens[192:]
        assert code_of(engine.set_generators, bad) == EINVAL  # a coordinate of p: the good set is gone too
        assert engine.generators() == (0, 0) and code_of(call) == ESTATE
        engine.set_generators(gens)
        _, many = CR.known_logs(65)
        assert code_of(engine.set_generators, many, 16) == EINVAL  # 16-bit tables stop at 64 generators
        assert engine.generators() == (0, 0) and code_of(call) == ESTATE
        engine.set_generators(gens)
        assert code_of(engine.set_generators, gens, 12) == EINVAL and engine.generators() == (0, 0)
        engine.set_generators(many[: 96 * 64], 16)
        assert engine.generators() == (64, 16) and call() == CR.closed_rows(CR.known_logs(65)[0], rows)

        # the neighbours: what they return with a set resident is what they return without
        engine.set_generators(None)
        n = 1000
        points = util.oracle_gen_points(oracle, n, 0x1234567, 0x89AB)
        ks = R.encode_scalars(R.rand_scalars(0x4E51, n))
        d_p, d_k = dev(points), dev(ks)
        exp_msm = util.oracle_msm(oracle, points, ks)
        pts = (R.mul(R.G, 0xD00D), R.FIXED_BASE)
        mrows = MV.many_rows(2, 300, 0x4E53)
        mbuf = MV.pack(mrows)[0]
        sbuf = R.encode_scalars([row[0] for row in mrows])
        other = V.base_bytes(R.mul(R.G, 0xD00F))

        def neighbours():
            d_s, d_m = dev(sbuf), dev(mbuf)
            d_out = torch.full((96 * 300,), 0xEE, dtype=torch.uint8, device="cuda")
            d_inf = torch.full((300,), 0xEE, dtype=torch.uint8, device="cuda")
            out = [engine.msm_device(d_p.data_ptr(), d_k.data_ptr(), n)]
            engine.set_bases_device(d_p.data_ptr(), n)
            out.append(engine.msm_fixed_base_device(d_k.data_ptr(), n))
            engine.batch_mul_device(other, d_s.data_ptr(), 300, d_out.data_ptr(), d_inf.data_ptr())
            out.append((bytes(d_out.cpu().numpy()), bytes(d_inf.cpu().numpy())))
            engine.batch_mul_multi_device(MV.bases_bytes(pts), d_m.data_ptr(), 300, d_out.data_ptr(), d_inf.data_ptr())
            out.append((bytes(d_out.cpu().numpy()), bytes(d_inf.cpu().numpy())))
            out.append(engine.check_points_device(d_p.data_ptr(), n).ok)
            return out

        without = neighbours()
        assert without[0] == exp_msm and without[1] == exp_msm and without[4]
        assert without[2] == msm.batch_mul_host(other, sbuf) and without[3] == msm.batch_mul_multi_host(MV.bases_bytes(pts), mbuf)
        engine.set_generators(gens)
        single, multi = engine.mul_table_builds(), engine.mul_multi_table_builds()
        assert call() == exp
        assert neighbours() == without
        assert call() == exp  # ... and the set survives them, the resident MSM bases included
        assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp_msm
        assert (engine.mul_table_builds(), engine.mul_multi_table_builds()) == (single, multi)  # warm tables: no build, and none by commit calls
        engine.set_generators(gens2)
        assert call() == exp2
        assert (engine.mul_table_builds(), engine.mul_multi_table_builds()) == (single, multi)
        last = engine.last_mul_window()
        engine.set_mul_window(16)  # the width belongs to the set
        try:
            assert call() == exp2 and engine.generators() == (k, 8)
        finally:
            engine.set_mul_window(0)
        assert engine.last_mul_window() == last
    finally:
        engine.set_generators(None)


# ---- refusals ----
def test_refusals(engine):
    import torch

    lib = msm.load_library()
    ctx = engine._ctx
    logs, gens = CR.known_logs(17)
    d_s = dev(R.encode_scalars(list(range(3, 3 + 40))))
    d_out = torch.full((208,), 0xA5, dtype=torch.uint8, device="cuda")
    d_inf = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(s, n, k, out_stride, base_stride, form, out):
        return lib.msm377_g1_commit_rows_device(ctx, s, n, k, out_stride, base_stride, form, out, d_inf.data_ptr())

    s, o = d_s.data_ptr(), d_out.data_ptr()
    engine.set_generators(None)
    try:
        assert call(s, 0, 2, 64, 32, V.WIRE, o) == 0  # n = 0 without a set
        assert lib.msm377_g1_commit_rows(ctx, None, 0, 2, 64, 32, V.WIRE, None, None) == 0
        assert call(s, 2, 2, 64, 32, V.WIRE, o) == ESTATE
        engine.set_generators(gens)
        assert call(s, 0, 2, 64, 32, V.WIRE, o) == 0
        assert call(None, 0, 2, 64, 32, V.MONT_FLAG, None) == 0
        assert call(s, 0, 0, 64, 32, V.WIRE, o) == EINVAL  # the shape is checked first, also for n = 0
        assert call(s, 2, 0, 64, 32, V.WIRE, o) == EINVAL
        assert call(s, 2, 4097, 32, 32, V.WIRE, o) == EINVAL
        assert call(s, 2, 18, 32, 32, V.WIRE, o) == ESTATE
        assert call(s, 2, 2, 0, 32, V.WIRE, o) == EINVAL
        assert call(s, 2, 2, 64, 0, V.WIRE, o) == EINVAL
        assert call(s, 2, 2, 48, 32, V.WIRE, o) == EINVAL
        assert call(s, 2, 2, 64, 48, V.WIRE, o) == EINVAL
        assert call(s, 2, 2, 64, 32, V.MONT, o) == EINVAL
        assert call(s, 2, 2, 64, 32, 3, o) == EINVAL
        assert call(None, 2, 2, 64, 32, V.WIRE, o) == EINVAL
        assert call(s, 2, 2, 64, 32, V.WIRE, None) == EINVAL
        assert call(s + 4, 2, 2, 64, 32, V.WIRE, o) == EINVAL  # alignment
        assert call(s, 2, 2, 64, 32, V.WIRE, o + 8) == EINVAL
        assert call(s, 2, 2, 64, 32, V.MONT_FLAG, o + 4) == EINVAL
        assert lib.msm377_g1_commit_rows(ctx, None, 2, 2, 64, 32, V.WIRE, None, None) == EINVAL
        assert lib.msm377_g1_commit_rows(ctx, None, 0, 4097, 64, 32, V.WIRE, None, None) == EINVAL
        assert lib.msm377_g1_set_generators(None, gens, 17, 0) == EINVAL
        assert bytes(d_out.cpu().numpy()) == b"\xa5" * 208 and bytes(d_inf.cpu().numpy()) == b"\xa5" * 16
        assert engine.generators() == (17, 8)
        # d_out_inf null, padded rows of 19 scalars
        got, flags = run_device(engine, bytes(d_s.cpu().numpy()), 2, 17, 32 * 19, 32, flags=False)
        assert (got, b"\0\0") == CR.closed_rows(logs, [tuple(range(3 + 19 * i, 3 + 19 * i + 17)) for i in range(2)]) and flags == b"\xee\xee"
    finally:
        engine.set_generators(None)


# ---- the host-buffer call ----
def test_host_buffer_call(engine):
    n, k = 257, 33
    gens, buf, wire, flags = twin_reference(k)
    rows = CR.sliding_rows(buf, n, k)
    exp = (wire[: 96 * n], flags[:n])
    with generators(engine, gens):
        assert run_rows(engine, rows) == exp
        for layout in ("rows", "columns"):
            data = CR.pack(rows, layout)[0]
            assert engine.commit_rows(data, k, "wire", layout) == exp, layout
            assert engine.commit_rows(data, k, "mont_flag", layout) == (V.mont_flag_records(*exp), exp[1]), layout
        lib = msm.load_library()
        import ctypes

        for layout in ("padded", "sliding"):  # the C call: any strides
            data, out_stride, base_stride = (CR.sliding_bytes(buf), 32, 32) if layout == "sliding" else CR.pack(rows, layout)
            out, inf = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
            assert lib.msm377_g1_commit_rows(engine._ctx, data, n, k, out_stride, base_stride, V.WIRE, ctypes.addressof(out), ctypes.addressof(inf)) == 0
            assert (out.raw, inf.raw) == exp, layout
        assert engine.commit_rows(b"", k) == (b"", b"")


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_host_buffer_call_past_one_piece(engine, layout):
    """k = 4 096 (the set of test_4096_generators), n = 257: the host-buffer call works in pieces of 2^20 / k = 256 rows, so
    its loop runs twice and the second piece is ONE row.  Records and flags are the device call's on the same inputs,
    byte for byte (the tests above pin the device call), on poisoned buffers: a piece that is not repacked, uploaded or
    downloaded shows.  Dense full-width scalars; two all-zero rows."""
    import ctypes

    k, n = CR.GEN_MAX, 257
    _, gens = CR.known_logs(k)
    s = np.random.default_rng(0xC0441715).integers(0, 256, size=(n, k, 32), dtype=np.uint8)
    s[7] = 0
    s[255] = 0  # identity outputs: one early, one in the last row of the first piece
    if layout == "rows":
        buf, out_stride, base_stride = s.tobytes(), 32 * k, 32
    else:
        buf, out_stride, base_stride = np.ascontiguousarray(s.transpose(1, 0, 2)).tobytes(), 32, 32 * n
    out, inf = ctypes.create_string_buffer(b"\xee" * (96 * n), 96 * n), ctypes.create_string_buffer(b"\xee" * n, n)
    with generators(engine, gens):
        rc = msm.load_library().msm377_g1_commit_rows(engine._ctx, buf, n, k, out_stride, base_stride, V.WIRE, ctypes.addressof(out), ctypes.addressof(inf))
        assert rc == 0
        wire, flags = run_device(engine, buf, n, k, out_stride, base_stride)
    assert inf.raw == flags and flags[7] == 1 and flags[255] == 1 and flags[n - 1] == 0
    assert out.raw == wire
