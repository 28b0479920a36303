"""Edwards-BLS12 k-term linear combination on the GPU (include/msm377.h "Edwards-BLS12 k-term linear combination";
csrc/kernels/ed_batch_lincomb.hpp): out[i] = sum_j [s_ij]P_ij through msm377_ed_batch_lincomb_device /
msm377_ed_batch_lincomb.  Expected values: the host twin (which tests/test_ed_batch_lincomb_host.py pins to tests/pyref.py
and to the older twins), pyref itself, the older device calls for k = 1 and k = 2, and the model
tests/ed_walk_lincomb_model.py for the stash and the k tables.  No expected value comes from the call under test.  Every
test leaves the engine at (wire, wire)."""
import ctypes

import numpy as np
import pytest

import batch_mul_vectors as V
import ed_batch_lincomb_vectors as KV
import ed_batch_mul_var_vectors as VV
import ed_walk_lincomb_model as WKM
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import engine as E
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, EPOINT, ESTATE

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257)  # a lane, a wave and a workgroup, each with its neighbours
TERMS = (1, 2, 3, 5, 8)  # 3 and 5: a one-term last table round; 8 at 257: four rounds, a full 64 KB workgroup and a ragged one
PASS = KV.PASS


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


def poisoned(nbytes, value=0xEE):
    import torch

    return torch.full((max(16, nbytes),), value, dtype=torch.uint8, device="cuda")


def full(k):
    return [(64, 32)] * k


def device_terms(points, scalars, strides):
    """(the tensors, the terms of the call) for k point and k scalar buffers."""
    d = [(dev(p), dev(s)) for p, s in zip(points, scalars)]
    return d, [(p.data_ptr(), s.data_ptr(), ps, ss) for (p, s), (ps, ss) in zip(d, strides)]


def run_device(engine, points, scalars, n=None, strides=None):
    """The records of one device call on a freshly poisoned (0xEE) output buffer."""
    n = len(points[0]) // 64 if n is None else n
    d, terms = device_terms(points, scalars, strides or full(len(points)))
    d_out = poisoned(64 * n)
    engine.ed_batch_lincomb_device(terms, n, d_out.data_ptr())
    return bytes(d_out.cpu().numpy()[: 64 * n])


def code_of(call, *args):
    with pytest.raises(msm.MsmError) as err:
        call(*args)
    return err.value


_CASES = {}


def case(n, k):
    """(k point buffers, k scalar buffers, the twin's records) of the (n, k) case: computed once, never changed."""
    if (n, k) not in _CASES:
        pb, sb = KV.encode(*KV.case(n, k)[:2])
        _CASES[n, k] = (pb, sb, msm.ed_batch_lincomb_host(pb, sb))
    return _CASES[n, k]


# ---- GPU == host twin ----
@pytest.mark.parametrize("k", TERMS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_host_twin(engine, n, k):
    pb, sb, wire = case(n, k)
    assert run_device(engine, pb, sb) == wire
    assert engine.read_walk_stash(info_only=True)[0].k == k


def test_probe_against_pyref(engine):
    """The relations block and the planted classes of the 257-output, three-term case by pyref itself, not the twin."""
    points, scalars, relations = KV.case(257, 3)
    pb, sb, _ = case(257, 3)
    got = run_device(engine, pb, sb)
    assert sorted(relations.values()) == sorted(KV.relations(3))
    lanes = sorted(set(relations) | {i for i in KV.LANES if i < 257})
    assert b"".join(got[64 * i : 64 * i + 64] for i in lanes) == KV.expected(points, scalars, lanes)
    for i, name in relations.items():
        if name in KV.SUM_IS_IDENTITY:
            assert got[64 * i : 64 * i + 64] == KV.IDENTITY_WIRE, name


# ---- k = 1 and k = 2: the new kernels, the older calls' bytes ----
def test_one_and_two_terms_equal_the_older_calls_byte_for_byte(engine):
    n = 257
    for k in (1, 2):
        pb, sb, wire = case(n, k)
        d = [dev(x) for x in pb + sb]
        d_old = poisoned(64 * n)
        if k == 1:
            engine.ed_batch_mul_var_device(d[0].data_ptr(), d[1].data_ptr(), n, d_old.data_ptr())
        else:
            engine.ed_batch_lincomb2_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_old.data_ptr())
        assert engine.read_walk_stash(info_only=True)[0].kind in (E.WALK_ED_BATCH_MUL_VAR, E.WALK_ED_BATCH_LINCOMB2)
        assert run_device(engine, pb, sb) == bytes(d_old.cpu().numpy()) == wire
        info = engine.read_walk_stash(info_only=True)[0]
        assert (info.kind, info.k) == (E.WALK_ED_BATCH_LINCOMB, k) and info.kind == 10  # the new kernels ran: no forward


# ---- strides ----
@pytest.mark.parametrize("zero", [{(1, "p")}, {(1, "s")}, {(1, "p"), (1, "s")}, {(0, "p"), (2, "s")}], ids=["point", "scalar", "both", "schnorr as one sum"])
def test_strides_equal_the_expanded_form(engine, zero):
    n, k = 257, 3
    pb, sb, _ = case(n, k)
    sb = list(sb)
    sb[1] = R.encode_scalars([VV.MASK256]) + sb[1][32:]  # the ONE scalar of a stride-0 term: full width, a final carry
    sb[2] = R.encode_scalars([R.ED_SUBGROUP + 1]) + sb[2][32:]
    strides = [(0 if (t, "p") in zero else 64, 0 if (t, "s") in zero else 32) for t in range(k)]
    args_p = [b[:64] if (t, "p") in zero else b for t, b in enumerate(pb)]
    args_s = [b[:32] if (t, "s") in zero else b for t, b in enumerate(sb)]
    expanded_p = [KV.expand(b, 64, n) if len(b) == 64 else b for b in args_p]
    expanded_s = [KV.expand(b, 32, n) if len(b) == 32 else b for b in args_s]
    exp = msm.ed_batch_lincomb_host(expanded_p, expanded_s)
    assert run_device(engine, expanded_p, expanded_s) == exp
    assert run_device(engine, args_p, args_s, n=n, strides=strides) == exp


# ---- waves that are skipped ----
def test_skipped_waves_a_late_riser_and_plain_addition(engine):
    n, k = 4 * 64, 3
    pb, _, _ = case(257, k)
    pb = [b[: 64 * n] for b in pb]
    scalars = [VV.random_scalars("lk zero wave %d" % t, n) for t in range(k)]
    for t in range(k):
        for i in range(64, 128):  # wave 1: every scalar below 2^16, one lane at full width
            scalars[t][i] &= 0xFFFF
        for i in range(128, 192):  # wave 2: only the last term is not zero
            if t < k - 1:
                scalars[t][i] = 0
        for i in range(192, n):  # wave 3: all zero but one late riser, in the last term only
            scalars[t][i] = 0
    scalars[1][64 + 29] = VV.MASK256
    scalars[k - 1][192 + 17] = 0x1D
    sb = [R.encode_scalars(s) for s in scalars]
    wire = msm.ed_batch_lincomb_host(pb, sb)
    assert wire[64 * 192 : 64 * (192 + 17)] == KV.IDENTITY_WIRE * 17 and wire[64 * (192 + 18) : 64 * n] == KV.IDENTITY_WIRE * (n - 192 - 18)
    assert wire[64 * 128 : 64 * 192] == msm.ed_batch_mul_var_host(pb[k - 1][64 * 128 : 64 * 192], sb[k - 1][32 * 128 : 32 * 192])
    assert run_device(engine, pb, sb) == wire
    ones = [R.encode_scalars([1])] * k
    points = KV.case(257, k)[0]
    got = run_device(engine, pb, ones, n=n, strides=[(64, 0)] * k)  # every scalar 1: only the last step runs
    assert got == KV.expected([p[:n] for p in points], [[1] * n] * k)


# ---- the pass boundary ----
@pytest.mark.parametrize("n", [PASS - 1, PASS, PASS + 1])
def test_pass_boundary(engine, oracle, n):
    """One pass, one full pass, two passes (the second of ONE output) at k = 3, against the one-thread twin."""
    k = 3
    pb, sb, relations = KV.boundary_case(n, k, lambda m, a0, d: util.oracle_ed_gen_points(oracle, m, a0, d))
    got = run_device(engine, pb, sb)
    wire = msm.ed_batch_lincomb_host(pb, sb)
    assert got[-64 * 32 :] == wire[-64 * 32 :]
    assert got == wire
    assert sorted(set(relations.values())) == sorted(KV.relations(k))
    for lane, name in relations.items():
        if name in KV.SUM_IS_IDENTITY:
            assert wire[64 * lane : 64 * lane + 64] == KV.IDENTITY_WIRE, (lane, name)
    info, _, _ = engine.read_walk_stash(info_only=True)
    assert (info.kind, info.n, info.pass_offset, info.m, info.k) == (E.WALK_ED_BATCH_LINCOMB, n, PASS if n > PASS else 0, n - PASS if n > PASS else n, k)


# ---- the table allocation grows and stays ----
def test_table_growth_on_one_context():
    """k = 3, then k = 8, then k = 3 on a context of its own: the same bytes each time, and a refused call in between leaves
    the next one correct."""
    n = 257
    with msm.MsmEngine(1 << 10) as own:
        for k in (3, 8, 3):
            pb, sb, wire = case(n, k)
            assert run_device(own, pb, sb) == wire, k
            if k == 8:
                bad = list(pb)
                bad[7] = pb[7][: 64 * 100] + R.ed_encode_points([KV.off_curve_point()]) + pb[7][64 * 101 :]
                d, terms = device_terms(bad, sb, full(k))
                d_out = poisoned(64 * n, 0xA5)
                err = code_of(own.ed_batch_lincomb_device, terms, n, d_out.data_ptr())
                assert (err.code, err.term, err.index) == (EPOINT, 7, 100) and bool((d_out == 0xA5).all().item())
                assert code_of(own.read_walk_stash).code == ESTATE
                assert run_device(own, pb, sb) == wire


# ---- in place ----
def test_in_place(engine):
    n, k = 257, 3
    pb, sb, wire = case(n, k)
    for over in (0, 2):
        d, terms = device_terms(pb, sb, full(k))
        engine.ed_batch_lincomb_device(terms, n, d[over][0].data_ptr())
        assert bytes(d[over][0].cpu().numpy()) == wire, over
        for t in range(k):
            if t != over:
                assert bytes(d[t][0].cpu().numpy()) == pb[t]  # the other arrays are only read
    h = 200  # the fold in place: term 0 = G, term 1 = G + h records, out = G
    d_g, d_s, d_p2 = dev(pb[0][: 64 * h] + pb[1][: 64 * h]), [dev(s) for s in sb], dev(pb[2])
    terms = [(d_g.data_ptr(), d_s[0].data_ptr(), 64, 32), (d_g.data_ptr() + 64 * h, d_s[1].data_ptr(), 64, 32), (d_p2.data_ptr(), d_s[2].data_ptr(), 64, 32)]
    engine.ed_batch_lincomb_device(terms, h, d_g.data_ptr())
    assert bytes(d_g.cpu().numpy()) == wire[: 64 * h] + pb[1][: 64 * h]
    d_p = dev(pb[0])  # every term the same pointer
    d_out = poisoned(64 * n)
    engine.ed_batch_lincomb_device([(d_p.data_ptr(), s.data_ptr(), 64, 32) for s in d_s], n, d_out.data_ptr())
    assert bytes(d_out.cpu().numpy()) == msm.ed_batch_lincomb_host([pb[0]] * k, sb)
    d_one = poisoned(64 * n, 0xA5)  # the outputs over the ONE point of a stride-0 term
    d_one[:64] = d_p[:64]
    for t in range(k):
        terms = [(d_one.data_ptr() if j == t else d_p.data_ptr(), d_s[j].data_ptr(), 0 if j == t else 64, 32) for j in range(k)]
        assert code_of(engine.ed_batch_lincomb_device, terms, n, d_one.data_ptr()).code == EINVAL, t
    assert bytes(d_one.cpu().numpy()) == pb[0][:64] + b"\xa5" * (64 * (n - 1))


# ---- refusals ----
@pytest.mark.parametrize("where", ["term 0 only", "term 2 only", "equal indices", "lowest index", "stride-0 point", "second pass of term 1"])
def test_point_off_the_curve_is_refused(engine, where):
    import torch

    k = 3
    n = PASS + 5 if where == "second pass of term 1" else 257
    gx, gy = R.ED_G
    off, noncanonical = dev(R.ed_encode_points([KV.off_curve_point()])), dev(R.ed_encode_points([(gx + R.Q, gy)]))
    plant, term, index, text = {
        "term 0 only": ({(0, 9): off}, 0, 9, "not on the curve"),
        "term 2 only": ({(2, 256): noncanonical}, 2, 256, "not below q"),
        "equal indices": ({(2, 130): off, (1, 130): noncanonical}, 1, 130, "not below q"),  # the lowest term wins
        "lowest index": ({(0, 200): off, (2, 69): off, (1, 70): noncanonical}, 2, 69, "not on the curve"),
        "stride-0 point": ({(1, 0): off, (0, 3): off}, 1, 0, "not on the curve"),  # ONE point: index 0 of its term
        "second pass of term 1": ({(1, PASS + 2): off}, 1, PASS + 2, "not on the curve"),
    }[where]
    d_pts = [torch.empty(64 * n, dtype=torch.uint8, device="cuda") for _ in range(k)]
    for t, d_x in enumerate(d_pts):
        engine.ed_generate_bases_device(0xBADC0DE + t, n, d_x.data_ptr())
    for (t, i), rec in plant.items():
        d_pts[t][64 * i : 64 * i + 64] = rec
    d_s = dev(R.encode_scalars([5]))
    strides = [(0 if where == "stride-0 point" and t == 1 else 64, 0) for t in range(k)]
    d_out = poisoned(64 * n, 0xA5)
    err = code_of(engine.ed_batch_lincomb_device, [(d_x.data_ptr(), d_s.data_ptr(), ps, ss) for d_x, (ps, ss) in zip(d_pts, strides)], n, d_out.data_ptr())
    assert (err.code, err.term, err.index, err.array) == (EPOINT, term, index, None) and text in str(err)
    assert bool((d_out == 0xA5).all().item())
    if n == 257:  # the host-buffer call and the twin say the same
        pts = [bytes(d_x.cpu().numpy()) for d_x in d_pts]
        pts = [p[:64] if ps == 0 else p for p, (ps, _) in zip(pts, strides)]
        for call in (engine.ed_batch_lincomb, msm.ed_batch_lincomb_host):
            again = code_of(call, pts, [R.encode_scalars([5])] * k)
            assert (again.code, again.term, again.index) == (EPOINT, term, index)


def test_arguments(engine):
    lib = msm.load_library()
    ctx = engine._ctx
    pb = [R.ed_encode_points([R.ED_G, R.ed_mul(R.ED_G, 5)]), R.ed_encode_points([R.ed_mul(R.ED_G, 7), R.ED_G]), R.ed_encode_points([R.ED_G, R.ED_G])]
    sb = [R.encode_scalars([3, 4]), R.encode_scalars([1, 2]), R.encode_scalars([6, 0])]
    exp = R.ed_encode_points([R.ed_mul(R.ED_G, 16), R.ed_mul(R.ED_G, 22)])
    d, good = device_terms([x + bytes(16) for x in pb], [x + bytes(16) for x in sb], full(3))
    d_out = poisoned(160, 0xA5)
    o = d_out.data_ptr()
    call = lib.msm377_ed_batch_lincomb_device
    terms = E._lincomb_terms
    before = (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds())
    assert call(ctx, terms(good), 3, 0, o) == 0  # n = 0: no launch
    assert call(ctx, terms(good), 3, 0, None) == 0
    nine = [good[0]] * 9
    for n in (0, 2):  # the shape is checked first, whatever n
        assert call(ctx, terms(good), 0, n, o) == EINVAL and call(ctx, terms(nine), 9, n, o) == EINVAL and call(ctx, None, 3, n, o) == EINVAL
    for t in range(3):
        for which, strides in ((2, (1, 4, 16, 32, 63, 65, 96, 128)), (3, (1, 4, 16, 31, 33, 64))):
            for stride in strides:
                bad = [list(x) for x in good]
                bad[t][which] = stride
                assert call(ctx, terms(bad), 3, 2, o) == EINVAL and call(ctx, terms(bad), 3, 0, o) == EINVAL, (t, which, stride)
        for which in (0, 1):
            bad = [list(x) for x in good]
            bad[t][which] = 0
            assert call(ctx, terms(bad), 3, 2, o) == EINVAL, (t, which)  # null
            bad[t][which] = good[t][which] + 8
            assert call(ctx, terms(bad), 3, 2, o) == EINVAL, (t, which)  # misaligned
    assert call(ctx, terms(good), 3, 2, None) == EINVAL
    assert call(ctx, terms(good), 3, 2, o + 8) == EINVAL
    host_terms, keep = E._lincomb_host_terms(pb, sb, full(3))
    for forms in (("mont", "wire"), ("wire", "mont"), ("mont_flag", "wire")):
        engine.set_input_format(*forms)
        try:
            assert call(ctx, terms(good), 3, 2, o) == EINVAL, forms
            assert lib.msm377_ed_batch_lincomb(ctx, host_terms, 3, 2, None) == EINVAL
        finally:
            engine.set_input_format("wire", "wire")
    assert lib.msm377_ed_batch_lincomb(ctx, host_terms, 3, 2, None) == EINVAL
    assert lib.msm377_ed_batch_lincomb(ctx, None, 3, 2, None) == EINVAL and lib.msm377_ed_batch_lincomb(ctx, host_terms, 9, 0, None) == EINVAL
    assert lib.msm377_ed_batch_lincomb(ctx, host_terms, 3, 0, None) == 0
    assert bytes(d_out.cpu().numpy()) == b"\xa5" * 160
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == before  # no counter moved
    assert call(ctx, terms(good), 3, 2, o) == 0
    assert bytes(d_out.cpu().numpy()) == exp + b"\xa5" * 32
    del keep


# ---- the host-buffer call ----
def test_host_buffer_call_equals_device_call(engine):
    n, k = 257, 5
    pb, sb, wire = case(n, k)
    assert engine.ed_batch_lincomb(pb, sb) == wire
    assert engine.ed_batch_lincomb([b""], [b""]) == b""
    pb3, sb3, _ = case(n, 3)
    one_p, one_s = pb3[0][64 * 5 : 64 * 6], R.encode_scalars([VV.MASK256])
    schnorr = engine.ed_batch_lincomb([one_p, pb3[1], pb3[2]], [sb3[0], sb3[1], one_s])  # term 0 ONE point, term 2 ONE scalar
    assert schnorr == msm.ed_batch_lincomb_host([one_p * n, pb3[1], pb3[2]], [sb3[0], sb3[1], one_s * n])


def test_host_buffer_call_past_one_piece(engine):
    """n = 2^20 + 3 at k = 2: the host-buffer call works in pieces of 2^20 outputs, so its loop runs twice and the second
    piece is three outputs; a call of several pieces checks all of them before the first one runs.  Records equal the device
    call's on the same inputs byte for byte (the tests above pin the device call to the twin); a point off the curve in the
    SECOND piece of term 1 is refused with its index in the whole array and nothing written, although the first piece is
    fine.  ONE 16-bit scalar per term for all outputs: the walk skips its leading steps."""
    import torch

    n = (1 << 20) + 3
    arrays = []
    for seed in (0x9A5507, 0x5EED02):
        d_x = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        engine.ed_generate_bases_device(seed, n, d_x.data_ptr())
        arrays.append(bytes(d_x.cpu().numpy()))
        del d_x
    s0, s1 = 0xD0E5, 0xB1A5
    ones = [R.encode_scalars([s0]), R.encode_scalars([s1])]
    lib = msm.load_library()
    out = ctypes.create_string_buffer(b"\xee" * (64 * n), 64 * n)
    terms, keep = E._lincomb_host_terms(arrays, ones, [(64, 0), (64, 0)])
    assert lib.msm377_ed_batch_lincomb(engine._ctx, terms, 2, n, ctypes.addressof(out)) == 0
    assert out.raw == run_device(engine, arrays, ones, n=n, strides=[(64, 0), (64, 0)])
    last = KV.combine([KV.decode(a[-64:]) for a in arrays], [s0, s1])
    assert out.raw[-64:] == R.ed_encode_result(last)  # the last output of the second piece, by pyref
    bad = [arrays[0], arrays[1][: 64 * ((1 << 20) + 1)] + R.ed_encode_points([KV.off_curve_point()]) + arrays[1][64 * ((1 << 20) + 2) :]]
    terms, keep = E._lincomb_host_terms(bad, ones, [(64, 0), (64, 0)])
    ctypes.memset(out, 0xA5, 64 * n)
    err = code_of(engine._check, lib.msm377_ed_batch_lincomb(engine._ctx, terms, 2, n, ctypes.addressof(out)), "msm377_ed_batch_lincomb")
    assert (err.code, err.term, err.index) == (EPOINT, 1, (1 << 20) + 1)
    assert out.raw == b"\xa5" * (64 * n)
    del keep


# ---- stash and tables against the model ----
@pytest.mark.parametrize("k", [3, 8])
def test_walk_stash_and_tables_against_the_model(engine, k):
    n = 257 if k == 3 else 65
    pb, sb, wire = case(n, k)
    points, scalars, relations = KV.case(n, k)
    assert run_device(engine, pb, sb) == wire
    info, rows, products = engine.read_walk_stash()
    want = dict(kind=E.WALK_ED_BATCH_LINCOMB, form=E.WALK_FORM_ED, point_words=36, product_words=9, product_pad=3, n=n, pass_offset=0, m=n, width=4, k=k, segments=1, stride=0)
    assert info._asdict() == want and info.kind == 10
    lanes = sorted(set(relations) | set(range(1, 12)))  # the relations block and the first edge scalars, shifted from term to term
    decoded = WKM.check_stash(rows, products, points, scalars, lanes, "n = %d, k = %d: " % (n, k))
    assert b"".join(R.ed_encode_result(p) for p in decoded) == wire  # the tie: the records are these points
    words = []
    for t in range(k):
        tinfo, w = engine.ed_read_walk_table(t)
        assert (tinfo.m, tinfo.tables, tinfo.entries) == (n, k, 8)
        words.append(w)
    WKM.check_tables(words, points, "n = %d, k = %d: " % (n, k))
    _, first = engine.ed_read_walk_tables()  # the one-table read-back: table 0
    assert np.array_equal(first, words[0])
    _, part = engine.ed_read_walk_table(k - 1, first=n - 7, count=7)
    assert np.array_equal(part, words[k - 1][:, n - 7 : n])
    assert code_of(engine.ed_read_walk_table, k).code == EINVAL
    assert code_of(engine.read_walk_tables).code == ESTATE  # msm377_g1_read_walk_tables: not a G1 pass
    engine.ed_batch_lincomb2(pb[0], pb[1], sb[0], sb[1])
    assert engine.ed_read_walk_table(0, info_only=True)[0].tables == 2  # after a pairwise call: its two tables
    assert code_of(engine.ed_read_walk_table, 2).code == EINVAL
    engine.ed_batch_mul(R.ed_encode_points([R.ED_G]), R.encode_scalars([1, 2]))
    assert code_of(engine.ed_read_walk_table, 0).code == ESTATE  # not a per-point-table pass


# ---- state isolation ----
def test_other_state_survives(engine, oracle):
    pb, sb, wire = case(257, 3)
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
    ed_fixed = R.encode_scalars(VV.random_scalars("lk slots", 16 * 8))
    ed_fixed_exp = engine.ed_batch_mul_multi(ed_bases, ed_fixed)  # fills the 16 Edwards slots
    slots = [engine.ed_read_mul_table(j) for j in range(16)]
    g1_base = V.base_bytes(R.mul(R.G, 0xD00E))
    g1_fixed_exp = msm.batch_mul_host(g1_base, fixed)
    assert engine.batch_mul(g1_base, fixed) == g1_fixed_exp
    ed_gens = R.ed_encode_points([R.ed_mul(R.ED_G, 0x6E0 + j) for j in range(4)])
    g1_gens = b"".join(V.base_bytes(R.mul(R.G, 0x6E0 + j)) for j in range(4))
    rows = R.encode_scalars(VV.random_scalars("lk rows", 4 * 8))
    engine.ed_set_generators(ed_gens)
    engine.set_generators(g1_gens)
    ed_rows_exp, g1_rows_exp = engine.ed_commit_rows(rows, 4), engine.commit_rows(rows, 4)
    builds = (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds())
    assert run_device(engine, pb, sb) == wire
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == builds
    assert engine.last_check() == report
    for j, (info, words) in enumerate(slots):
        now_info, now_words = engine.ed_read_mul_table(j)
        assert now_info == info and np.array_equal(now_words, words), j
    assert engine.msm_fixed_base_device(d_k.data_ptr(), n) == exp  # the resident bases
    assert engine.ed_batch_mul_multi(ed_bases, ed_fixed) == ed_fixed_exp and engine.batch_mul(g1_base, fixed) == g1_fixed_exp
    assert engine.ed_commit_rows(rows, 4) == ed_rows_exp and engine.commit_rows(rows, 4) == g1_rows_exp  # both generator sets
    assert (engine.ed_mul_table_builds(), engine.mul_table_builds(), engine.mul_multi_table_builds()) == builds
    assert run_device(engine, pb, sb) == wire  # and the other way round
    assert engine.ed_batch_lincomb2(pb[0], pb[1], sb[0], sb[1]) == msm.ed_batch_lincomb2_host(pb[0], pb[1], sb[0], sb[1])  # the pairwise call afterwards
    engine.ed_set_generators(None)
    engine.set_generators(None)


def test_n_zero_touches_nothing(engine):
    pb, sb, wire = case(65, 3)
    assert run_device(engine, pb, sb) == wire
    lib = msm.load_library()
    terms, keep = E._lincomb_host_terms(pb, sb, full(3))
    assert lib.msm377_ed_batch_lincomb_device(engine._ctx, terms, 3, 0, None) == 0
    out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    assert lib.msm377_ed_batch_lincomb(engine._ctx, terms, 3, 0, ctypes.addressof(out)) == 0
    assert out.raw == b"\xa5" * 64
    assert code_of(engine.read_walk_stash).code == ESTATE  # a call of n = 0 ran no pass: the description is gone
    del keep
