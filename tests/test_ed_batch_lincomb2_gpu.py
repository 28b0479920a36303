"""Edwards-BLS12 pairwise linear combination on the GPU (include/msm377.h "Edwards-BLS12 pairwise linear combination";
csrc/kernels/ed_batch_lincomb2.hpp): out[i] = [a_i]P_i + [b_i]Q_i through msm377_ed_batch_lincomb2_device /
msm377_ed_batch_lincomb2.  Expected values: the host twin (which tests/test_ed_batch_lincomb2_host.py pins to tests/pyref.py
and to the reference's vectors), pyref itself, and the model tests/ed_walk_lincomb2_model.py for the stash and both tables.
No expected value comes from the device call.  Every test leaves the engine at (wire, wire)."""
import ctypes

import numpy as np
import pytest

import batch_mul_vectors as V
import ed_batch_lincomb2_vectors as LV
import ed_batch_mul_var_vectors as VV
import ed_walk_lincomb2_model as WLM
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import engine as E
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, EPOINT, ESTATE

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
PASS = LV.PASS
GOOD = (64, 64, 32, 32)


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


def poisoned(nbytes, value=0xEE):
    import torch

    return torch.full((max(16, nbytes),), value, dtype=torch.uint8, device="cuda")


def run_device(engine, p, q, a, b, n=None, strides=GOOD):
    """The records of one device call on a freshly poisoned (0xEE) output buffer."""
    n = len(p) // 64 if n is None else n
    d = [dev(x) for x in (p, q, a, b)]
    d_out = poisoned(64 * n)
    engine.ed_batch_lincomb2_device(*(t.data_ptr() for t in d), n, d_out.data_ptr(), *strides)
    return bytes(d_out.cpu().numpy()[: 64 * n])


def code_of(call, *args):
    with pytest.raises(msm.MsmError) as err:
        call(*args)
    return err.value


# ---- GPU == host twin ----
@pytest.fixture(scope="module")
def cases():
    """n -> (p, q, a, b bytes, the twin's records): two draws of every_curve_point, shifted edge scalars, the relations."""
    out = {}
    for n in SIZES:
        enc = LV.encode(*LV.case(n)[:4])
        out[n] = enc + (msm.ed_batch_lincomb2_host(*enc),)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin(engine, cases, n):
    *enc, wire = cases[n]
    assert run_device(engine, *enc) == wire


def test_probe_against_pyref(engine, cases):
    """The relations, the planted classes and the low-order points of the 257-pair case by pyref itself, not the twin."""
    ps, qs, as_, bs, relations = LV.case(257)
    got = run_device(engine, *cases[257][:4])
    assert len(relations) == 9 and set(relations.values()) == set(LV.RELATIONS)
    for i in LV.special_lanes(257):
        assert got[64 * i : 64 * i + 64] == R.ed_encode_result(LV.combine(ps[i], qs[i], as_[i], bs[i])), (i, relations.get(i))


# ---- strides ----
@pytest.mark.parametrize("zero", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1)], ids=["schnorr", "q", "both scalars", "all four"])
def test_strides_equal_the_expanded_form(engine, cases, zero):
    n = 257
    enc = list(cases[n][:4])
    enc[2] = R.encode_scalars([VV.MASK256]) + enc[2][32:]  # the ONE scalar of a stride-0 array: full width, a final carry
    enc[3] = R.encode_scalars([R.ED_SUBGROUP + 1]) + enc[3][32:]
    args = [buf[:size] if z else buf for buf, size, z in zip(enc, GOOD, zero)]
    expanded = [LV.expand(buf, size, n) if z else buf for buf, size, z in zip(enc, GOOD, zero)]
    exp = msm.ed_batch_lincomb2_host(*expanded)
    assert run_device(engine, *expanded) == exp
    assert run_device(engine, *args, n=n, strides=tuple(0 if z else s for s, z in zip(GOOD, zero))) == exp


# ---- waves that are skipped ----
def test_skipped_waves_a_late_riser_and_plain_addition(engine, cases):
    n = 5 * 64
    pb, qb = cases[513][0][: 64 * n], cases[513][1][: 64 * n]
    a, b = VV.random_scalars("l2 zero wave a", n), VV.random_scalars("l2 zero wave b", n)
    for i in list(range(64, 128)) + list(range(192, 256)) + list(range(256, n)):
        a[i] = b[i] = 0
    b[256 + 17] = 0x1D  # wave 4: one late riser, in b only
    ab, bb = R.encode_scalars(a), R.encode_scalars(b)
    wire = msm.ed_batch_lincomb2_host(pb, qb, ab, bb)
    assert wire[64 * 64 : 64 * 128] == LV.IDENTITY_WIRE * 64 and wire[64 * 192 : 64 * 256] == LV.IDENTITY_WIRE * 64
    assert run_device(engine, pb, qb, ab, bb) == wire
    ones = R.encode_scalars([1])
    ps, qs = LV.case(513)[:2]
    got = run_device(engine, pb, qb, ones, ones, n=n, strides=(64, 64, 0, 0))  # a = b = 1: only the last step runs
    assert got == b"".join(R.ed_encode_result(R.ed_add(ps[i], qs[i])) for i in range(n))


# ---- the pass boundary ----
@pytest.mark.parametrize("n", [PASS - 1, PASS, PASS + 1])
def test_pass_boundary(engine, oracle, n):
    """One pass, one full pass, two passes (the second of ONE pair), against the one-thread twin."""
    pb, qb, ab, bb, relations = LV.boundary_case(n, lambda m, a0, d: util.oracle_ed_gen_points(oracle, m, a0, d))
    got = run_device(engine, pb, qb, ab, bb)
    wire = msm.ed_batch_lincomb2_host(pb, qb, ab, bb)
    assert got[-64 * 16 :] == wire[-64 * 16 :]
    assert got == wire
    for lane, name in relations.items():
        if name in ("Q = -P, a = b", "Q = [m]P, a + b m = 0", "both the identity", "a = b = 0"):
            assert wire[64 * lane : 64 * lane + 64] == LV.IDENTITY_WIRE, (lane, name)
    info, _, _ = engine.read_walk_stash(info_only=True)
    assert (info.kind, info.n, info.pass_offset, info.m) == (E.WALK_ED_BATCH_LINCOMB2, n, PASS if n > PASS else 0, n - PASS if n > PASS else n)


# ---- in place ----
def test_in_place(engine, cases):
    n = 513
    pb, qb, ab, bb, wire = cases[n]
    for over in (0, 1):
        d = [dev(x) for x in (pb, qb, ab, bb)]
        engine.ed_batch_lincomb2_device(*(t.data_ptr() for t in d), n, d[over].data_ptr())
        assert bytes(d[over].cpu().numpy()) == wire, over
        assert bytes(d[1 - over].cpu().numpy()) == (qb, pb)[over]  # the other array is only read
    h = 300  # the fold in place: p = G, q = G + h records, out = G
    d_g, d_a, d_b = dev(pb[: 64 * h] + qb[: 64 * h]), dev(ab), dev(bb)
    engine.ed_batch_lincomb2_device(d_g.data_ptr(), d_g.data_ptr() + 64 * h, d_a.data_ptr(), d_b.data_ptr(), h, d_g.data_ptr())
    assert bytes(d_g.cpu().numpy()) == wire[: 64 * h] + qb[: 64 * h]
    d_p = dev(pb)  # p == q as the same pointer
    d_out = poisoned(64 * n)
    engine.ed_batch_lincomb2_device(d_p.data_ptr(), d_p.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr())
    assert bytes(d_out.cpu().numpy()) == msm.ed_batch_lincomb2_host(pb, pb, ab, bb)
    d_one = poisoned(64 * n, 0xA5)  # the outputs over the ONE point of a stride-0 array
    d_one[:64] = d_p[:64]
    for strides, args in (((0, 64, 32, 32), (d_one, d_p)), ((64, 0, 32, 32), (d_p, d_one))):
        err = code_of(engine.ed_batch_lincomb2_device, args[0].data_ptr(), args[1].data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_one.data_ptr(), *strides)
        assert err.code == EINVAL
    assert bytes(d_one.cpu().numpy()) == pb[:64] + b"\xa5" * (64 * (n - 1))


# ---- refusals ----
@pytest.mark.parametrize("where", ["p only", "q only", "both", "second pass of q"])
def test_off_curve_point_is_refused(engine, where):
    import torch

    n = PASS + 5
    bad_p, bad_q, array, index = {"p only": (9, None, "p", 9), "q only": (None, 70, "q", 70), "both": (300, 200, "q", 200), "second pass of q": (None, PASS + 2, "q", PASS + 2)}[where]
    d_p, d_q = torch.empty(64 * n, dtype=torch.uint8, device="cuda"), torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    engine.ed_generate_bases_device(0xBADC0DE, n, d_p.data_ptr())
    engine.ed_generate_bases_device(0xC0FFEE, n, d_q.data_ptr())
    off = dev(R.ed_encode_points([LV.off_curve_point()]))
    for d_x, bad in ((d_p, bad_p), (d_q, bad_q)):
        if bad is not None:
            d_x[64 * bad : 64 * bad + 64] = off
    d_s = dev(R.encode_scalars([5]))
    d_out = poisoned(64 * n, 0xA5)
    err = code_of(engine.ed_batch_lincomb2_device, d_p.data_ptr(), d_q.data_ptr(), d_s.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), 64, 64, 0, 0)
    assert (err.code, err.array, err.index) == (EPOINT, array, index) and "not on the curve" in str(err)
    assert bool((d_out == 0xA5).all().item())


def test_noncanonical_equal_indices_and_a_stride_0_point(engine, cases):
    n = 257
    pb, qb, ab, bb, _ = cases[n]
    gx, gy = R.ED_G
    noncanonical, off = R.ed_encode_points([(gx + R.Q, gy)]), R.ed_encode_points([LV.off_curve_point()])

    def plant(buf, at):
        out = bytearray(buf)
        for i, rec in at.items():
            out[64 * i : 64 * i + 64] = rec
        return bytes(out)

    for in_p, in_q, array, index, text in (
        ({200: noncanonical}, {}, "p", 200, "not below q"),
        ({130: off}, {130: noncanonical}, "p", 130, "not on the curve"),  # equal indices: p
        ({70: noncanonical}, {69: off, 256: off}, "q", 69, "not on the curve"),
    ):
        pp, qq = plant(pb, in_p), plant(qb, in_q)
        d = [dev(x) for x in (pp, qq, ab, bb)]
        d_out = poisoned(64 * n, 0xA5)
        err = code_of(engine.ed_batch_lincomb2_device, *(t.data_ptr() for t in d), n, d_out.data_ptr())
        assert (err.code, err.array, err.index) == (EPOINT, array, index) and text in str(err), (in_p, in_q)
        assert bool((d_out == 0xA5).all().item())
        host = code_of(engine.ed_batch_lincomb2, pp, qq, ab, bb)
        assert (host.code, host.array, host.index) == (EPOINT, array, index)
        twin = code_of(msm.ed_batch_lincomb2_host, pp, qq, ab, bb)
        assert (twin.code, twin.array, twin.index) == (EPOINT, array, index)
    d = [dev(x) for x in (pb, off, ab, bb)]  # a stride-0 array is ONE point, index 0
    d_out = poisoned(64 * n, 0xA5)
    err = code_of(engine.ed_batch_lincomb2_device, *(t.data_ptr() for t in d), n, d_out.data_ptr(), 64, 0, 32, 32)
    assert (err.code, err.array, err.index) == (EPOINT, "q", 0)
    assert bool((d_out == 0xA5).all().item())


def test_arguments(engine):
    lib = msm.load_library()
    ctx = engine._ctx
    pb, qb, ab, bb = LV.encode([R.ED_G, R.ed_mul(R.ED_G, 5)], [R.ed_mul(R.ED_G, 7), R.ED_G], [3, 4], [1, 2])
    exp = R.ed_encode_points([R.ed_mul(R.ED_G, 10), R.ed_mul(R.ED_G, 22)])
    d = [dev(x + bytes(16)) for x in (pb, qb, ab, bb)]
    d_out = poisoned(160, 0xA5)
    ptrs, o = [t.data_ptr() for t in d], d_out.data_ptr()
    call = lib.msm377_ed_batch_lincomb2_device
    assert call(ctx, *ptrs, 0, *GOOD, o) == 0  # n = 0: no launch
    assert call(ctx, None, None, None, None, 0, 0, 0, 0, 0, None) == 0
    for pos in range(4):
        for stride in (1, 4, 16, 31, 33, 96, 32 if pos < 2 else 64):
            strides = list(GOOD)
            strides[pos] = stride
            assert call(ctx, *ptrs, 2, *strides, o) == EINVAL, (pos, stride)
    assert call(ctx, *ptrs, 0, 64, 64, 16, 32, o) == EINVAL  # the strides are checked first
    for hole in range(4):
        args = list(ptrs)
        args[hole] = None
        assert call(ctx, *args, 2, *GOOD, o) == EINVAL, hole
        args[hole] = ptrs[hole] + 8
        assert call(ctx, *args, 2, *GOOD, o) == EINVAL, hole
    assert call(ctx, *ptrs, 2, *GOOD, None) == EINVAL
    assert call(ctx, *ptrs, 2, *GOOD, o + 8) == EINVAL
    for forms in (("mont", "wire"), ("wire", "mont"), ("mont_flag", "wire")):
        engine.set_input_format(*forms)
        try:
            assert call(ctx, *ptrs, 2, *GOOD, o) == EINVAL, forms
            assert lib.msm377_ed_batch_lincomb2(ctx, pb, qb, ab, bb, 2, *GOOD, None) == EINVAL
        finally:
            engine.set_input_format("wire", "wire")
    assert lib.msm377_ed_batch_lincomb2(ctx, None, None, None, None, 2, *GOOD, None) == EINVAL
    assert lib.msm377_ed_batch_lincomb2(ctx, None, None, None, None, 2, 64, 64, 8, 32, None) == EINVAL
    assert lib.msm377_ed_batch_lincomb2(ctx, None, None, None, None, 0, *GOOD, None) == 0
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 160
    assert call(ctx, *ptrs, 2, *GOOD, o) == 0
    assert bytes(d_out.cpu().numpy()) == exp + b"\xa5" * 32


# ---- the host-buffer call ----
def test_host_buffer_call_equals_device_call(engine, cases):
    pb, qb, ab, bb, wire = cases[513]
    assert engine.ed_batch_lincomb2(pb, qb, ab, bb) == wire
    assert engine.ed_batch_lincomb2(b"", b"", b"", b"") == b""
    one_p, one_b = pb[64 * 5 : 64 * 6], R.encode_scalars([VV.MASK256])
    assert engine.ed_batch_lincomb2(one_p, qb, ab, one_b) == msm.ed_batch_lincomb2_host(one_p * 513, qb, ab, one_b * 513)  # the Schnorr shape


def test_host_buffer_call_past_one_piece(engine):
    """n = 2^20 + 1: the host-buffer call works in pieces of 2^20 pairs, so its loop runs twice and the second piece is ONE
    pair; a call of several pieces checks all of them before the first one runs.  Records equal the device call's on the same
    inputs byte for byte (the tests above pin the device call to the twin); a point off the curve in the SECOND piece of q is
    refused with its index in the whole array and nothing written, although the first piece is fine.  ONE 40-bit scalar each
    for all pairs: the walk skips its leading steps."""
    import torch

    n = (1 << 20) + 1
    arrays = []
    for seed in (0x9A5507, 0x5EED02):
        d_x = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        engine.ed_generate_bases_device(seed, n, d_x.data_ptr())
        arrays.append(bytes(d_x.cpu().numpy()))
        del d_x
    pb, qb = arrays
    one_a, one_b = R.encode_scalars([0xD0E50F7AB1]), R.encode_scalars([0xB1A5ED0C75])
    lib = msm.load_library()
    out = ctypes.create_string_buffer(b"\xee" * (64 * n), 64 * n)
    assert lib.msm377_ed_batch_lincomb2(engine._ctx, pb, qb, one_a, one_b, n, 64, 64, 0, 0, ctypes.addressof(out)) == 0
    assert out.raw == run_device(engine, pb, qb, one_a, one_b, n=n, strides=(64, 64, 0, 0))
    last = [R.ed_encode_result(LV.combine(LV.decode(pb[-64:]), LV.decode(qb[-64:]), 0xD0E50F7AB1, 0xB1A5ED0C75))]
    assert out.raw[-64:] == last[0]  # the one pair of the second piece, by pyref
    bad = qb[: 64 << 20] + R.ed_encode_points([LV.off_curve_point()])
    ctypes.memset(out, 0xA5, 64 * n)
    err = code_of(engine._check, lib.msm377_ed_batch_lincomb2(engine._ctx, pb, bad, one_a, one_b, n, 64, 64, 0, 0, ctypes.addressof(out)), "msm377_ed_batch_lincomb2")
    assert (err.code, err.array, err.index) == (EPOINT, "q", 1 << 20)
    assert out.raw == b"\xa5" * (64 * n)


# ---- stash and tables against the model ----
def test_walk_stash_and_tables_against_the_model(engine, cases):
    n = 257
    *enc, wire = cases[n]
    ps, qs, as_, bs, relations = LV.case(n)
    assert run_device(engine, *enc) == wire
    info, rows, products = engine.read_walk_stash()
    want = dict(kind=E.WALK_ED_BATCH_LINCOMB2, form=E.WALK_FORM_ED, point_words=36, product_words=9, product_pad=3, n=n, pass_offset=0, m=n, width=4, k=2, segments=1, stride=0)
    assert info._asdict() == want and info.kind == 8
    lanes = sorted(set(relations) | set(range(1, 40)))  # the relations block and the edge scalars, shifted against each other
    decoded = WLM.check_stash(rows, products, ps, qs, as_, bs, lanes, "n = 257: ")
    assert b"".join(R.ed_encode_result(p) for p in decoded) == wire  # the tie: the records are these points
    tinfo, words_p = engine.ed_read_walk_table(0)
    _, words_q = engine.ed_read_walk_table(1)
    assert (tinfo.m, tinfo.tables, tinfo.entries) == (n, 2, 8)
    WLM.check_tables(words_p, words_q, ps, qs, "n = 257: ")
    _, first = engine.ed_read_walk_tables()  # the one-table read-back: table 0
    assert np.array_equal(first, words_p)
    _, part = engine.ed_read_walk_table(1, first=250, count=7)
    assert np.array_equal(part, words_q[:, 250:257])
    assert code_of(engine.ed_read_walk_table, 2).code == EINVAL
    assert code_of(engine.read_walk_tables).code == ESTATE  # msm377_g1_read_walk_tables: not a G1 pass
    engine.ed_batch_mul_var(enc[0], enc[2])
    assert engine.ed_read_walk_table(0, info_only=True)[0].tables == 1  # after a variable-base call: its one table
    assert code_of(engine.ed_read_walk_table, 1).code == EINVAL
    engine.ed_batch_mul(R.ed_encode_points([R.ED_G]), R.encode_scalars([1, 2]))
    assert code_of(engine.ed_read_walk_table, 0).code == ESTATE  # not a per-point-table pass


# ---- state isolation ----
def test_other_state_survives(engine, oracle, cases):
    *enc, wire = cases[257]
    n = 1000
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
    fixed = R.encode_scalars(VV.edge_scalars())
    ed_bases = R.ed_encode_points([R.ed_mul(R.ED_G, 0xD00E + j) for j in range(16)])
    ed_fixed = R.encode_scalars(VV.random_scalars("l2 slots", 16 * 8))
    ed_fixed_exp = engine.ed_batch_mul_multi(ed_bases, ed_fixed)  # fills the 16 Edwards slots
    slots = [engine.ed_read_mul_table(j) for j in range(16)]
    g1_base = V.base_bytes(R.mul(R.G, 0xD00E))
    g1_fixed_exp = msm.batch_mul_host(g1_base, fixed)
    assert engine.batch_mul(g1_base, fixed) == g1_fixed_exp
    builds = (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds())
    assert run_device(engine, *enc) == wire
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == builds
    assert engine.last_check() == report
    for j, (info, words) in enumerate(slots):
        now_info, now_words = engine.ed_read_mul_table(j)
        assert now_info == info and np.array_equal(now_words, words), j
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp  # the resident bases
    assert engine.ed_batch_mul_multi(ed_bases, ed_fixed) == ed_fixed_exp and engine.batch_mul(g1_base, fixed) == g1_fixed_exp
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == builds
    assert run_device(engine, *enc) == wire  # and the other way round


def test_n_zero_touches_nothing(engine, cases):
    *enc, wire = cases[65]
    assert run_device(engine, *enc) == wire
    lib = msm.load_library()
    assert lib.msm377_ed_batch_lincomb2_device(engine._ctx, None, None, None, None, 0, *GOOD, None) == 0
    out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    assert lib.msm377_ed_batch_lincomb2(engine._ctx, *enc, 0, *GOOD, ctypes.addressof(out)) == 0
    assert out.raw == b"\xa5" * 64
