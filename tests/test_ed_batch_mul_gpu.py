"""Edwards-BLS12 batch multiplication on the GPU (include/msm377.h "Edwards-BLS12 batch multiplication";
csrc/kernels/ed_batch_mul.hpp): out[i] = sum_j [s_ij]B_j through msm377_ed_batch_mul_multi_device /
msm377_ed_batch_mul_multi for both window widths and the rule.  Expected values: tests/pyref.py (every base class, every
relation between bases), the host twin (which tests/test_ed_batch_mul_host.py pins to pyref, and whose output is probed
against pyref again here), msm377_ed_generate_bases_device (the parent's own many-point call) and, at scale, one
Edwards MSM over the outputs with random weights against a closed form.  No expected value comes from the call under
test.  Every test leaves the engine at the rule (width 0) and at (wire, wire)."""
import contextlib
import ctypes
import functools
import random

import numpy as np
import pytest

import ed_batch_mul_vectors as EV
import pyref as R
import record_model as RM
import webgpu_msm_bls12_377_amd as msm
from check_vectors import ed_low_order_points
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

pytestmark = pytest.mark.gpu

ORD = R.ED_SUBGROUP
BLOCK = 1024  # outputs per workgroup product tree of the normalisation (4 per thread, 256 threads)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)  # around a wave, a workgroup, a thread's outputs, a tree
ESTATE = -5  # MSM377_ESTATE


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


def run_device(engine, bases: bytes, buf: bytes, n, out_stride=None, base_stride=32):
    """The records of one device call on a freshly poisoned output buffer, which must stay poisoned behind them."""
    import torch

    d_s = dev(buf)
    d_out = torch.full((64 * n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.ed_batch_mul_multi_device(bases, d_s.data_ptr(), n, d_out.data_ptr(), out_stride, base_stride)
    out = bytes(d_out.cpu().numpy())
    assert out[64 * n :] == b"\xee" * 64
    return out[: 64 * n]


def run_rows(engine, points, rows, layout="rows"):
    buf, out_stride, base_stride = EV.pack(rows, layout)
    return run_device(engine, EV.bases_bytes(points), buf, len(rows), out_stride, base_stride)


def closed_form(total):
    return R.ed_encode_result(R.ed_mul(R.ED_G, total % ORD))


@functools.lru_cache(maxsize=None)
def three():
    """G, [M]G and a point outside the subgroup."""
    return (R.ED_G, R.ed_mul(R.ED_G, EV.M), dict(EV.bases())["P_plus_order4_a"])


# ---- GPU == host twin (== pyref at a probe set) ----
@pytest.fixture(scope="module")
def size_reference():
    """k -> (rows, wire) of the host twin for the largest size; every size takes a prefix (row-major rows)."""
    out = {}
    probe = [0, 1, 2, 3, 4, 5, 6, 7, 8, 64, 1024, 4096]
    for k in (1, 2, 3):
        rows = EV.many_rows(k, max(SIZES), 0xEDF1BA + k)
        wire = msm.ed_batch_mul_multi_host(EV.bases_bytes(three()[:k]), EV.pack(rows)[0])
        exp = EV.expected(three()[:k], [rows[i] for i in probe])[0]
        assert b"".join(wire[64 * i : 64 * i + 64] for i in probe) == exp
        out[k] = (rows, wire)
    return out


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("width", EV.WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin(engine, size_reference, n, width, k):
    rows, wire = size_reference[k]
    with window(engine, width):
        got = run_rows(engine, three()[:k], rows[:n])
        assert engine.last_mul_window() == width
    assert got == wire[: 64 * n]


# ---- the parent's own many-point call as a yardstick ----
@pytest.mark.parametrize("width", EV.WIDTHS)
def test_generator_equivalence(engine, width):
    """Base ED_G under the SplitMix64(seed) outputs, zero-extended: byte for byte msm377_ed_generate_bases_device."""
    import torch

    n, seed = 4097, 0xED5EED
    d_ref = torch.full((64 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    engine.ed_generate_bases_device(seed, n, d_ref.data_ptr())
    g = R.splitmix64(seed)
    scalars = [next(g) or 1 for _ in range(n)]
    with window(engine, width):
        got = run_device(engine, EV.bases_bytes((R.ED_G,)), R.encode_scalars(scalars), n)
    assert got == bytes(d_ref.cpu().numpy())
    assert got[:64] == R.ed_encode_result(R.ed_mul(R.ED_G, scalars[0]))


# ---- every base class, every relation between bases ----
@pytest.mark.parametrize("width", EV.WIDTHS)
@pytest.mark.parametrize("name", [name for name, _ in EV.bases()])
def test_every_base_class(engine, name, width):
    pt = dict(EV.bases())[name]
    rows = [(s,) for s in EV.single_scalars() + EV.digit_scalars(width)[-4:]]
    wire, _ = EV.expected((pt,), rows)
    with window(engine, width):
        assert run_rows(engine, (pt,), rows) == wire


@pytest.mark.parametrize("width", EV.WIDTHS)
@pytest.mark.parametrize("name", [name for name, _ in EV.tuples()])
def test_every_relation_between_bases(engine, name, width):
    points = dict(EV.tuples())[name]
    rows = EV.relation_rows(len(points))
    wire, pts = EV.expected(points, rows)
    with window(engine, width):
        assert run_rows(engine, points, rows) == wire
    if name in ("G_negG", "G_mG", "order4_pair"):  # an identity output whose terms are not the identity
        i = {"G_negG": 0, "G_mG": 2, "order4_pair": 4}[name]
        assert pts[i] == R.ED_ID and pts[i + 1] != R.ED_ID and wire[64 * i : 64 * i + 64] == EV.IDENTITY_WIRE


@pytest.mark.parametrize("width", EV.WIDTHS)
def test_only_low_order_bases(engine, width):
    """k = 4: the identity, the point of order 2 and both points of order 4; every term is [s mod 4] of its base."""
    low = [R.ED_ID] + ed_low_order_points()
    n = 300
    rows = EV.many_rows(4, n, 0x10A0)
    pts = []
    for row in rows:
        acc = R.ED_ID
        for b, s in zip(low, row):
            acc = R.ed_add(acc, R.ed_mul(b, s % 4))
        pts.append(acc)
    with window(engine, width):
        got = run_rows(engine, low, rows)
    assert got == R.ed_encode_points(pts)
    assert len(set(pts)) == 4  # every output is a low-order point, and all four occur


@functools.lru_cache(maxsize=None)
def planted_identities():
    """(points, rows, twin records): identity outputs at lanes 0, 63, 64, 255, 256, at the ends of product trees, at every
    third output of one workgroup and at all four outputs of one thread, each a sum that cancels with neither term the
    identity; the twin's records are checked to be (0, 1) exactly there and probed against pyref at their neighbours."""
    n = 3 * BLOCK + 7
    pts = three()[:2]
    rows = EV.many_rows(2, n, 0x1DE48)[9:] + EV.many_rows(2, 9, 0x1DE49, bits=128)
    ts = EV.random_scalars(0x1DE4A, 3, bits=230)
    where = [0, 63, 64, 255, 256, n - 1, 2 * BLOCK, 3 * BLOCK] + list(range(BLOCK, 2 * BLOCK, 3))
    where += [2 * BLOCK + 5 + 256 * j for j in range(4)]  # all four outputs of one thread
    for k, i in enumerate(where):
        t = ts[k % 3] + k
        rows[i] = (EV.M * t, 4 * ORD - t)  # [M t]G + [4 ORD - t][M]G = O, neither term O
    wire = msm.ed_batch_mul_multi_host(EV.bases_bytes(pts), EV.pack(rows)[0])
    planted = set(where)
    for i in range(n):
        assert (wire[64 * i : 64 * i + 64] == EV.IDENTITY_WIRE) == (i in planted), i
    probe = [1, 62, 65, 254, 257, BLOCK - 1, BLOCK + 1, 2 * BLOCK + 1, n - 2]
    assert b"".join(wire[64 * i : 64 * i + 64] for i in probe) == EV.expected(pts, [rows[i] for i in probe])[0]
    return pts, rows, wire


@pytest.mark.parametrize("width", EV.WIDTHS)
def test_identity_outputs_leave_their_neighbours_exact(engine, width):
    """One output's Z does not leak into another through the shared inversion."""
    pts, rows, wire = planted_identities()
    with window(engine, width):
        assert run_rows(engine, pts, rows) == wire


# ---- layouts ----
@pytest.mark.parametrize("width", EV.WIDTHS)
def test_layouts(engine, size_reference, width):
    """Rows, columns and padded rows of one matrix: identical bytes.  n = 257, k = 3."""
    rows, wire = size_reference[3]
    n = 257
    with window(engine, width):
        for layout in ("rows", "columns", "padded"):
            assert run_rows(engine, three(), rows[:n], layout) == wire[: 64 * n], layout


@pytest.mark.parametrize("width", EV.WIDTHS)
def test_sliding_rows(engine, width):
    """out_stride = base_stride = 32: row i is scalars i, i + 1, i + 2 of ONE buffer of n + 2 scalars."""
    n = 257
    flat = (EV.EDGE + EV.random_scalars(0x511DE, n + 2))[: n + 2]
    rows = [tuple(flat[i : i + 3]) for i in range(n)]
    wire = msm.ed_batch_mul_multi_host(EV.bases_bytes(three()), EV.pack(rows)[0])
    with window(engine, width):
        assert run_device(engine, EV.bases_bytes(three()), R.encode_scalars(flat), n, 32, 32) == wire


# ---- scale: every output enters one Edwards MSM with a random weight ----
SCALE_B = (0xED5CA1E0B0, 0xED5CA1E0B1F, 0xED5CA1E0B22)  # B_j = [b_j]G


@functools.lru_cache(maxsize=None)
def scale_bases(k):
    return EV.bases_bytes([R.ed_mul(R.ED_G, b) for b in SCALE_B[:k]])


@functools.lru_cache(maxsize=2)
def scale_inputs(n, k):
    """(row-major scalar bytes s_ij, any 256-bit value; weight bytes t_i below 2^63; t_i; sum_j b_j s_ij per output)."""
    rng = np.random.default_rng(0xED5CA + 16 * n + k)
    s = rng.integers(0, 256, size=(n, k, 32), dtype=np.uint8)
    t = rng.integers(1, 2**63, size=n, dtype=np.uint64)
    tw = np.zeros((n, 4), dtype=np.uint64)
    tw[:, 0] = t
    sb = s.tobytes()
    per = [sum(SCALE_B[j] * int.from_bytes(sb[32 * (k * i + j) : 32 * (k * i + j) + 32], "little") for j in range(k)) for i in range(n)]
    return sb, tw.tobytes(), t.tolist(), per


def weighted_sum(engine, d_points, tb, lo, hi):
    d_t = dev(tb[32 * lo : 32 * hi])
    return engine.ed_msm_device(d_points.data_ptr() + 64 * lo, d_t.data_ptr(), hi - lo)


@pytest.mark.parametrize("width", EV.WIDTHS + (0,))
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n", [65537, (1 << 18) + 3])
def test_scale(engine, n, k, width):
    import torch

    sb, tb, ti, per = scale_inputs(n, k)
    d_s = dev(sb)
    d_out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    with window(engine, width):
        engine.ed_batch_mul_multi_device(scale_bases(k), d_s.data_ptr(), n, d_out.data_ptr())
        assert engine.last_mul_window() == (width or 8)  # the inherited rule takes the wide tables from 2^19 outputs on
    assert weighted_sum(engine, d_out, tb, 0, n) == closed_form(sum(t * p for t, p in zip(ti, per)))
    out = bytes(d_out.cpu().numpy())
    for lo in (0, n - 64):
        twin = msm.ed_batch_mul_multi_host(scale_bases(k), sb[32 * k * lo : 32 * k * (lo + 64)])
        assert out[64 * lo : 64 * (lo + 64)] == twin, lo


def test_passes_past_the_context_capacity(engine):
    """n = 2^20 + 257, k = 1, on an engine created for 2^16 points: two passes, the second of 257 outputs."""
    import torch

    n = (1 << 20) + 257
    sb, tb, ti, per = scale_inputs(n, 1)
    d_s = dev(sb)
    d_out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    with msm.MsmEngine(1 << 16) as small:
        small.set_mul_window(8)
        small.ed_batch_mul_multi_device(scale_bases(1), d_s.data_ptr(), n, d_out.data_ptr())
        assert small.last_mul_window() == 8
        assert small.ed_mul_table_builds() == 1 and small.mul_multi_table_builds() == 0 and small.mul_table_builds() == 0
    # the session engine holds 2^20 points: the first 2^20 outputs in one MSM, the last 257 against the twin
    assert weighted_sum(engine, d_out, tb, 0, 1 << 20) == closed_form(sum(t * p for t, p in zip(ti[: 1 << 20], per)))
    twin = msm.ed_batch_mul_multi_host(scale_bases(1), sb[32 * (1 << 20) :])
    assert bytes(d_out[64 * (1 << 20) :].cpu().numpy()) == twin


# ---- the table slots ----
def test_slots_are_kept_per_position(engine):
    rows = EV.many_rows(3, 64, 0x510751)
    g, h, h2, f = (R.ed_mul(R.ED_G, m) for m in (0x51A7E0, 0x51A7E1, 0x51A7E2, 0x51A7E3))
    two = [row[:2] for row in rows]
    twin = lambda pts, rs: msm.ed_batch_mul_multi_host(EV.bases_bytes(pts), EV.pack(rs)[0])
    e_gh, e_hg, e_gh2, e_gh2f = twin((g, h), two), twin((h, g), two), twin((g, h2), two), twin((g, h2, f), rows)
    g1_single, g1_multi = engine.mul_table_builds(), engine.mul_multi_table_builds()
    with window(engine, 8):
        before = engine.ed_mul_table_builds()
        assert run_rows(engine, (g, h), two) == e_gh
        assert engine.ed_mul_table_builds() == before + 2  # cold: both slots
        assert run_rows(engine, (g, h), two) == e_gh
        assert engine.ed_mul_table_builds() == before + 2  # the same again: none
        assert run_rows(engine, (h, g), two) == e_hg
        assert engine.ed_mul_table_builds() == before + 4  # two bases swapped: two slots
        assert run_rows(engine, (g, h), two) == e_gh
        assert engine.ed_mul_table_builds() == before + 6
        assert run_rows(engine, (g, h2), two) == e_gh2
        assert engine.ed_mul_table_builds() == before + 7  # slot 1 alone
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.ed_mul_table_builds() == before + 8  # slot 2 alone
        assert run_rows(engine, (g, h2), two) == e_gh2
        assert engine.ed_mul_table_builds() == before + 8  # k = 2 after k = 3: none; slot 2 is left as it is
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.ed_mul_table_builds() == before + 8
        # a refused call (an off-curve base at position 1) changes nothing: not the counter, not a later result
        bad = EV.bases_bytes((g, (h2[0], h2[1] ^ 1), f))
        with pytest.raises(msm.MsmError) as e:
            run_device(engine, bad, EV.pack(rows)[0], len(rows))
        assert e.value.code == EINVAL
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.ed_mul_table_builds() == before + 8
        engine.set_mul_window(16)
        assert run_rows(engine, (g, h2), two) == e_gh2
        assert engine.ed_mul_table_builds() == before + 10  # the width is part of the key: the slots used, not slot 2
        engine.set_mul_window(8)
        assert run_rows(engine, (g, h2, f), rows) == e_gh2f
        assert engine.ed_mul_table_builds() == before + 12  # slots 0 and 1 back at width 8; slot 2 was never touched
    assert (engine.mul_table_builds(), engine.mul_multi_table_builds()) == (g1_single, g1_multi)


# ---- the tables themselves ----
def record_words(pt):
    return [int(w) for coord in RM.ed_make_base(pt) for w in coord] + [0] * 5


@pytest.mark.parametrize("width", EV.WIDTHS)
@pytest.mark.parametrize("which", ["subgroup", "order4"])
def test_table_read_back(engine, which, width):
    """Rows 0, 1, W - 1, the carry entry and a seeded sample, word for word record_model.ed_make_base([d 2^(c w)]B); an
    order-4 base's table holds identity records (1, 1, 0)."""
    base, order = (R.ed_mul(R.ED_G, 0x7AB1E), ORD) if which == "subgroup" else (ed_low_order_points()[1], 4)
    other = R.ED_G
    with window(engine, width):
        run_rows(engine, (other, base), [(1, 1)])  # the table under test sits in slot 1
    info, _ = engine.ed_read_mul_table(1, info_only=True)
    W, half = EV.windows(width), 1 << (width - 1)
    assert (info.width, info.rows, info.records) == (width, W + 1, W * half + 1)
    assert info.key == EV.bases_bytes((base,)) + bytes(32)
    rnd = random.Random("ed table %s %d" % (which, width))
    picks = [(w, d) for w in (0, 1, W - 1) for d in (1, 2, half)] + [(rnd.randrange(W), rnd.randrange(1, half + 1)) for _ in range(6)]
    for w, d in picks:
        _, words = engine.ed_read_mul_table(1, first=w * half + d - 1, count=1)
        assert words[0].tolist() == record_words(R.ed_mul(base, (d << (width * w)) % order)), (w, d)
    _, words = engine.ed_read_mul_table(1, first=W * half, count=1)  # the carry's entry
    assert words[0].tolist() == record_words(R.ed_mul(base, (1 << (width * W)) % order))
    _, row0 = engine.ed_read_mul_table(1, first=0, count=half)
    assert not row0[:, 27:].any()  # pad words
    if which == "order4":
        ident = record_words(R.ED_ID)
        assert ident[:9] == ident[9:18] and not any(ident[18:])  # (1, 1, 0) in Montgomery limbs
        assert row0[3].tolist() == ident and row0[7].tolist() == ident  # [4]B, [8]B
    with pytest.raises(msm.MsmError) as e:
        engine.ed_read_mul_table(1, first=info.records, count=1)
    assert e.value.code == EINVAL
    with pytest.raises(msm.MsmError) as e:
        engine.ed_read_mul_table(16, info_only=True)
    assert e.value.code == EINVAL


def test_read_back_of_a_slot_never_built():
    with msm.MsmEngine(1 << 10) as fresh:
        with pytest.raises(msm.MsmError) as e:
            fresh.ed_read_mul_table(0, info_only=True)
        assert e.value.code == ESTATE


# ---- neighbours ----
def test_neighbours_survive(engine):
    """A G1 batch_mul_multi, a commit_rows over a resident generator set, a fixed-base MSM over resident bases and an
    Edwards MSM give the same bytes before and after interleaved Edwards batch calls; no G1 build counter moves."""
    import torch

    n = 1000
    d_p = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0x4E16, n, d_p.data_ptr())
    g1 = bytes(d_p.cpu().numpy())
    ks = R.encode_scalars(R.rand_scalars(0x4E51, n))
    d_k = dev(ks)
    d_e = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    engine.ed_generate_bases_device(0x4E17, n, d_e.data_ptr())
    d_ek = dev(R.encode_scalars(R.rand_scalars(0x4E52, n, ORD)))
    rows = R.encode_scalars(EV.random_scalars(0x4E53, 2 * 300))
    ed_rows = EV.many_rows(2, 300, 0x4E54)
    ed_pts = three()[:2]
    e_ed = msm.ed_batch_mul_multi_host(EV.bases_bytes(ed_pts), EV.pack(ed_rows)[0])

    engine.set_generators(g1[: 96 * 4], 8)
    engine.set_bases_device(d_p.data_ptr(), n)
    g1_calls = lambda: (engine.msm_fixed_base_device(d_k.data_ptr(), n), engine.batch_mul_multi(g1[96 * 8 : 96 * 10], rows), engine.commit_rows(rows, 2))
    try:
        first = g1_calls()
        counters = lambda: (engine.mul_table_builds(), engine.mul_multi_table_builds())
        for width in EV.WIDTHS:
            with window(engine, width):
                assert g1_calls() == first  # (the G1 slots follow the width: their own rebuild, counted before the Edwards calls)
                before = counters()
                assert run_rows(engine, ed_pts, ed_rows) == e_ed
                assert counters() == before
                assert g1_calls() == first
                assert run_rows(engine, ed_pts, ed_rows) == e_ed
                assert counters() == before  # neither the Edwards calls nor the G1 calls between them built a G1 table
        assert engine.generators() == (4, 8)
        ed_first = engine.ed_msm_device(d_e.data_ptr(), d_ek.data_ptr(), n)
        assert run_rows(engine, ed_pts, ed_rows) == e_ed  # (at the rule's width again: the slots follow it)
        builds = engine.ed_mul_table_builds()
        assert engine.ed_msm_device(d_e.data_ptr(), d_ek.data_ptr(), n) == ed_first
        assert run_rows(engine, ed_pts, ed_rows) == e_ed
        assert engine.ed_mul_table_builds() == builds  # an Edwards MSM in between costs no rebuild
        rep = engine.ed_check_points_device(d_e.data_ptr(), n)
        assert rep.ok
        assert run_rows(engine, ed_pts, ed_rows) == e_ed
    finally:
        engine.set_generators(None)


# ---- the host-buffer call ----
@pytest.mark.parametrize("width", EV.WIDTHS)
@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_host_buffer_call(engine, size_reference, layout, width):
    rows, wire = size_reference[3]
    n = 1025
    bases = EV.bases_bytes(three())
    with window(engine, width):
        assert engine.ed_batch_mul_multi(bases, EV.pack(rows[:n], layout)[0], layout) == wire[: 64 * n]
        assert engine.ed_batch_mul_multi(bases, b"", layout) == b""
        assert engine.last_mul_window() == width
        one, wire1 = size_reference[1]
        assert engine.ed_batch_mul(bases[:64], EV.pack(one[:65])[0]) == wire1[: 64 * 65]


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_host_buffer_call_past_one_piece(layout):
    """k = 16, n = 65 537: the host-buffer call works in pieces of 2^20 / k = 65 536 rows, so its loop runs twice and the
    second piece is ONE row.  The records are the device call's on the same inputs, byte for byte (the tests above pin the
    device call), on a poisoned buffer: a piece that is not repacked, uploaded or downloaded shows.  One width for the
    whole call: the width a device call of n rows picks, and 16 builds on a fresh engine -- a second width for the second
    piece would build 16 more."""
    k, n = 16, 65537
    bases = EV.bases_bytes([R.ed_mul(R.ED_G, 0xEDB16B00 + j) for j in range(k)])
    s = np.random.default_rng(0xED16B45).integers(0, 256, size=(n, k, 32), dtype=np.uint8)
    s[7] = 0
    s[65535] = 0  # identity outputs: one early, one in the last row of the first piece
    if layout == "rows":
        buf, out_stride, base_stride = s.tobytes(), 32 * k, 32
    else:
        buf, out_stride, base_stride = np.ascontiguousarray(s.transpose(1, 0, 2)).tobytes(), 32, 32 * n
    out = ctypes.create_string_buffer(b"\xee" * (64 * n), 64 * n)
    with msm.MsmEngine(1 << 10) as fresh:
        assert msm.load_library().msm377_ed_batch_mul_multi(fresh._ctx, bases, k, buf, n, out_stride, base_stride, ctypes.addressof(out)) == 0
        host_width = fresh.last_mul_window()
        assert fresh.ed_mul_table_builds() == 16 and fresh.mul_multi_table_builds() == 0 and fresh.mul_table_builds() == 0
        wire = run_device(fresh, bases, buf, n, out_stride, base_stride)
        assert fresh.last_mul_window() == host_width
        assert fresh.ed_mul_table_builds() == 16
    assert out.raw == wire
    assert wire[64 * 7 : 64 * 8] == wire[64 * 65535 : 64 * 65536] == EV.IDENTITY_WIRE


# ---- arguments ----
def test_arguments(engine):
    import torch

    lib = msm.load_library()
    ctx = engine._ctx
    d_s = dev(R.encode_scalars(list(range(3, 3 + 36))))
    d_out = torch.full((144,), 0xA5, dtype=torch.uint8, device="cuda")
    builds = engine.ed_mul_table_builds()
    ms = [0xEDE1A70 + j for j in range(17)]
    fresh = EV.bases_bytes([R.ed_mul(R.ED_G, m) for m in ms])
    gx, gy = R.ED_G

    def call(bases, k, s, n, out_stride, base_stride, out):
        return lib.msm377_ed_batch_mul_multi_device(ctx, bases, k, s, n, out_stride, base_stride, out)

    s, o = d_s.data_ptr(), d_out.data_ptr()
    assert call(fresh, 2, s, 0, 64, 32, o) == 0  # n = 0: no launch, no table
    assert call(None, 2, None, 0, 64, 32, None) == 0
    assert call(fresh, 0, s, 0, 64, 32, o) == EINVAL  # the shape is checked first, also for n = 0
    assert call(fresh, 0, s, 2, 64, 32, o) == EINVAL
    assert call(fresh, 17, s, 2, 32 * 17, 32, o) == EINVAL
    assert call(fresh, 2, s, 2, 0, 32, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 0, o) == EINVAL
    assert call(fresh, 2, s, 2, 48, 32, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 48, o) == EINVAL
    assert call(None, 2, s, 2, 64, 32, o) == EINVAL
    assert call(fresh, 2, None, 2, 64, 32, o) == EINVAL
    assert call(fresh, 2, s, 2, 64, 32, None) == EINVAL
    assert call(fresh, 2, s + 4, 2, 64, 32, o) == EINVAL  # alignment
    assert call(fresh, 2, s, 2, 64, 32, o + 8) == EINVAL
    assert call(fresh[:64] + R.ed_encode_points([(gx + R.Q, gy)]), 2, s, 2, 64, 32, o) == EINVAL  # a coordinate of q or more
    assert call(fresh[:64] + R.ed_encode_points([(gx, gy ^ 1)]), 2, s, 2, 64, 32, o) == EINVAL  # off the curve
    assert lib.msm377_ed_batch_mul_multi(ctx, fresh, 2, None, 2, 64, 32, None) == EINVAL
    assert lib.msm377_ed_batch_mul_multi(ctx, fresh, 17, None, 0, 64, 32, None) == EINVAL
    assert lib.msm377_ed_batch_mul_multi(ctx, fresh, 2, None, 0, 64, 32, None) == 0
    for forms in (("wire", "mont"), ("mont", "wire"), ("mont_flag", "mont")):  # like every msm377_ed_* call
        engine.set_input_format(*forms)
        try:
            assert call(fresh, 2, s, 2, 64, 32, o) == EINVAL
            assert lib.msm377_ed_batch_mul_multi(ctx, fresh, 2, ctypes.c_char_p(bytes(128)), 2, 64, 32, ctypes.addressof(ctypes.create_string_buffer(128))) == EINVAL
        finally:
            engine.set_input_format("wire", "wire")
    assert engine.ed_mul_table_builds() == builds
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 144
    # the largest k, padded rows of 18 scalars
    got = run_device(engine, fresh[: 64 * 16], bytes(d_s.cpu().numpy()), 2, 32 * 18, 32)
    exp = [R.ed_mul(R.ED_G, sum(ms[j] * (3 + 18 * i + j) for j in range(16))) for i in range(2)]
    assert got == R.ed_encode_points(exp)
    assert engine.ed_mul_table_builds() == builds + 16
