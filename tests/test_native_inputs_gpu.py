"""Native input forms on the GPU (include/msm377.h "native input forms"): Montgomery points, infinity flags and Montgomery
scalars through every G1 call that honours msm377_ctx_set_input_format.  Expected values come from the committed
goldens, from pyref, or from the wire-format call on the same logical inputs (which other tests pin to the oracle);
the re-encoding is done by the Python-integer codecs of host/codecs.py.  Every test leaves the engine at (wire, wire)."""
import contextlib
import random

import pytest

import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import CHECK_ALL, CHECK_CANONICAL, CHECK_CURVE, EINVAL, EPOINT, ESTATE, combine_partials_bytes

pytestmark = pytest.mark.gpu

A0, D = 0x0123456789ABCDEF0123456789ABCDEF, 0xFEDCBA9876543
IDENTITY = R.encode_result(None)
FORMS = (("mont", "wire"), ("wire", "mont"), ("mont", "mont"), ("mont_flag", "mont"))
GARBAGE = b"\xff" * 96


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


@contextlib.contextmanager
def forms(engine, points, scalars):
    engine.set_input_format(points, scalars)
    try:
        yield
    finally:
        engine.set_input_format("wire", "wire")


def native(points_wire: bytes, scalars_wire: bytes, pform: str, sform: str, flagged=(), flag_byte=1):
    """The same logical inputs in the named forms; points at `flagged` become identity records with garbage coordinates
    (mont_flag only)."""
    pts = R.decode_points(points_wire)
    buf = bytearray(msm.encode_points_native(pts, pform))
    for i in flagged:
        buf[104 * i : 104 * i + 96] = GARBAGE
        buf[104 * i + 96] = flag_byte
        buf[104 * i + 97 : 104 * i + 104] = b"\x5a" * 7
    return bytes(buf), msm.encode_scalars_native(R.decode_scalars(scalars_wire), sform)


def without(points_wire: bytes, scalars_wire: bytes, flagged):
    keep = [i for i in range(len(scalars_wire) // 32) if i not in set(flagged)]
    return b"".join(points_wire[96 * i : 96 * i + 96] for i in keep), b"".join(scalars_wire[32 * i : 32 * i + 32] for i in keep)


@pytest.fixture(scope="module")
def pool(oracle):
    """1025 points P_i = [A0 + i D]G and scalars below r; every small case takes a prefix."""
    n = 1025
    return util.oracle_gen_points(oracle, n, A0, D), R.encode_scalars(R.rand_scalars(0x1A71FE, n))


def wire_msm(engine, points: bytes, scalars: bytes) -> bytes:
    n = len(scalars) // 32
    if n == 0:
        return IDENTITY
    d_p, d_s = dev(points), dev(scalars)
    return engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n)


# ---- golden vectors ----
def test_golden_vectors_in_every_form(engine, golden):
    for name, case in sorted(golden.items()):
        if not name.startswith("g1_"):
            continue
        n = case["n"]
        for pform, sform in FORMS:
            pb, sb = native(case["points"], case["scalars"], pform, sform)
            d_p, d_s = dev(pb), dev(sb)
            with forms(engine, pform, sform):
                assert engine.get_input_format() == (pform, sform)
                assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == case["expected"], (name, pform, sform, "device")
                assert engine.msm(pb, sb) == case["expected"], (name, pform, sform, "host")


# ---- block and mask boundaries ----
@pytest.mark.parametrize("narrow", [True, False])
@pytest.mark.parametrize("n", [33, 257, 1025])
def test_block_and_mask_boundaries(engine, pool, n, narrow):
    points, scalars = pool[0][: 96 * n], pool[1][: 32 * n]
    flagged = sorted({0, 31, 32, n // 2, n - 1})
    engine.set_narrow_max((1 << 16) if narrow else 0)
    try:
        full = wire_msm(engine, points, scalars)
        rest = wire_msm(engine, *without(points, scalars, flagged))
        for pform, sform, fl, exp in (("mont", "mont", (), full), ("mont_flag", "mont", (), full), ("mont_flag", "mont", flagged, rest), ("mont_flag", "wire", flagged, rest)):
            pb, sb = native(points, scalars, pform, sform, fl)
            d_p, d_s = dev(pb), dev(sb)
            with forms(engine, pform, sform), util.edwards_only(engine):
                assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp, (n, narrow, pform, sform, bool(fl))
            assert engine.last_geometry() == ((22, 11) if narrow else (16, 15))
    finally:
        engine.set_narrow_max(1 << 16)


def test_65537_generated_points(engine):
    """Past the narrow path and the 2^16 boundary: points from generate_bases_device, re-encoded on the host."""
    import torch

    n = 65537
    d_wire = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0xBA5E5, n, d_wire.data_ptr())
    points = bytes(d_wire.cpu().numpy())
    scalars = R.encode_scalars(R.rand_scalars(0x65537, n))
    d_sw = dev(scalars)
    flagged = [0, 255, 256, 65535, 65536]
    full = engine.msm_device(d_wire.data_ptr(), d_sw.data_ptr(), n)
    rest = wire_msm(engine, *without(points, scalars, flagged))
    for fl, exp in (((), full), (flagged, rest)):
        pb, sb = native(points, scalars, "mont_flag", "mont", fl)
        d_p, d_s = dev(pb), dev(sb)
        with forms(engine, "mont_flag", "mont"), util.edwards_only(engine):
            assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp
    assert engine.last_geometry() == (16, 15)


# ---- infinity ----
def test_flagged_points_contribute_nothing(engine, pool):
    n = 48
    points, scalars = pool[0][: 96 * n], pool[1][: 32 * n]
    flagged = [0, 5, 31, 32, 47]
    kept_p, kept_s = without(points, scalars, flagged)
    exp = wire_msm(engine, kept_p, kept_s)
    assert exp == R.encode_result(R.msm_naive(R.decode_points(kept_p), R.decode_scalars(kept_s)))
    for flag_byte in (1, 0xFF):
        for sform in ("wire", "mont"):
            pb, sb = native(points, scalars, "mont_flag", sform, flagged, flag_byte)
            d_p, d_s = dev(pb), dev(sb)
            with forms(engine, "mont_flag", sform):
                assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp, (flag_byte, sform)
                assert engine.msm(pb, sb) == exp, (flag_byte, sform)
    pb, sb = native(points, scalars, "mont_flag", "mont", range(n))
    d_p, d_s = dev(pb), dev(sb)
    with forms(engine, "mont_flag", "mont"):
        assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == IDENTITY


# ---- scalars ----
def test_montgomery_scalars_at_their_edges(engine, pool):
    """Montgomery forms of 0, 1 and r - 1, and raw values of r and more up to 2^256 - 1: all accepted, never ESCALAR."""
    Q = R.R_ORDER
    raw = [0, (1 << 256) % Q, ((Q - 1) << 256) % Q, (1 << 256) - 1, Q, (1 << 256) - Q, 1, Q - 1]
    n = len(raw)
    points = pool[0][: 96 * n]
    meaning = msm.decode_scalars_native(b"".join(v.to_bytes(32, "little") for v in raw), "mont")
    assert meaning[:3] == [0, 1, Q - 1] and meaning[3] == ((1 << 256) - 1) * pow(1 << 256, -1, Q) % Q
    exp = R.encode_result(R.msm_naive(R.decode_points(points), meaning))
    sb = b"".join(v.to_bytes(32, "little") for v in raw)
    for pform in ("wire", "mont"):
        pb = msm.encode_points_native(R.decode_points(points), pform)
        d_p, d_s = dev(pb), dev(sb)
        with forms(engine, pform, "mont"):
            assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp
            assert engine.msm(pb, sb) == exp


# ---- resident bases ----
@pytest.mark.parametrize("table", ["plain", "precomputed16", "precomputed20"])
def test_resident_bases_with_flagged_points(engine, pool, table):
    n = 1025
    points, _ = pool
    flagged = [0, 31, 32, 600, 1024]
    batch = [R.encode_scalars(R.rand_scalars(0xBA7C0 + b, n)) for b in range(5)]
    exp = [wire_msm(engine, *without(points, sc, flagged)) for sc in batch]
    full = wire_msm(engine, points, batch[0])
    pb, _ = native(points, b"", "mont_flag", "wire", flagged)
    d_p = dev(pb)
    mont = [msm.encode_scalars_native(R.decode_scalars(sc), "mont") for sc in batch]
    d_s = [dev(sc) for sc in mont]
    d_all = dev(b"".join(mont))
    try:
        with forms(engine, "mont_flag", "mont"):
            if table == "plain":
                engine.set_bases_device(d_p.data_ptr(), n)
            else:
                engine.set_precompute_window(16 if table == "precomputed16" else 20)
                engine.set_bases_precomputed_device(d_p.data_ptr(), n)
            with util.edwards_only(engine):
                # the mask persists across calls, and across the per-call import of other scalars
                assert engine.msm_fixed_base_device(d_s[0].data_ptr(), n) == exp[0]
                assert engine.msm_fixed_base_device(d_s[1].data_ptr(), n) == exp[1]
                assert engine.msm_fixed_base(mont[2]) == exp[2]
                assert engine.msm_fixed_base_batch_device(d_all.data_ptr(), n, 2) == exp[:2]
                assert engine.msm_fixed_base_batch_device(d_all.data_ptr(), n, 5) == exp  # two halves: the twin imports its own
        # wire scalars against the flagged set: the masked import runs all the same
        d_w = dev(batch[3])
        assert engine.msm_fixed_base_device(d_w.data_ptr(), n) == exp[3]
        assert engine.msm_fixed_base(batch[4]) == exp[4]
        # a wire base set afterwards: no stale mask
        d_pw = dev(points)
        engine.set_bases_device(d_pw.data_ptr(), n)
        d_w0 = dev(batch[0])
        assert engine.msm_fixed_base_device(d_w0.data_ptr(), n) == full
        # the host-buffer set-bases call in a native form
        with forms(engine, "mont_flag", "wire"):
            engine.set_bases(pb)
            assert engine.msm_fixed_base_device(d_w0.data_ptr(), n) == exp[0]
            # a failed set-bases call leaves no resident bases, as today
            with pytest.raises(msm.MsmError) as e:
                engine.set_bases_device(d_p.data_ptr(), engine.max_points + 1)
            assert e.value.code == EINVAL
            with pytest.raises(msm.MsmError) as e:
                engine.msm_fixed_base_device(d_w0.data_ptr(), n)
            assert e.value.code == ESTATE
    finally:
        engine.set_precompute_window(16)


# ---- check calls ----
def test_check_calls_under_flags(engine, pool):
    n = 300
    points = pool[0][: 96 * n]
    flagged = [0, 31, 32, 299]
    clean, _ = native(points, b"", "mont_flag", "wire", flagged)
    pts = R.decode_points(points)
    off_curve_at, noncanon_at = 77, 130
    bad = bytearray(clean)
    x, y = pts[off_curve_at]
    bad[104 * off_curve_at : 104 * off_curve_at + 104] = msm.encode_points_native([(x, (y + 1) % R.P)], "mont_flag")
    bad[104 * noncanon_at : 104 * noncanon_at + 48] = R.P.to_bytes(48, "little")  # the raw value p: not below p
    bad = bytes(bad)
    with forms(engine, "mont_flag", "wire"):
        for flags in (CHECK_CANONICAL, CHECK_CANONICAL | CHECK_CURVE, CHECK_ALL):
            d_c = dev(clean)
            for rep in (engine.check_points_device(d_c.data_ptr(), n, flags), engine.check_points(clean, flags)):
                assert rep.ok and rep.checked == n and (rep.noncanonical, rep.off_curve, rep.outside_subgroup) == (0, 0, 0), flags
        d_b = dev(bad)
        for rep in (engine.check_points_device(d_b.data_ptr(), n, CHECK_ALL), engine.check_points(bad, CHECK_ALL)):
            assert rep.checked == n and (rep.noncanonical, rep.off_curve, rep.outside_subgroup) == (1, 1, 0)
            assert (rep.first_bad, rep.first_bad_reason) == (off_curve_at, CHECK_CURVE)
        rep = engine.check_points_device(d_b.data_ptr(), n, CHECK_CANONICAL)
        assert (rep.noncanonical, rep.off_curve, rep.first_bad, rep.first_bad_reason) == (1, 0, noncanon_at, CHECK_CANONICAL)
        # base checks: a flagged set passes all three, the bad one is refused at its first finding
        engine.set_base_checks(CHECK_ALL)
        try:
            engine.set_bases_device(d_c.data_ptr(), n)
            assert engine.last_check().ok and engine.last_check().checked == n
            with pytest.raises(msm.MsmError) as e:
                engine.set_bases_device(d_b.data_ptr(), n)
            assert e.value.code == EPOINT and engine.last_check().first_bad == off_curve_at
        finally:
            engine.set_base_checks(0)
    # the wire-format check of the imported clean set agrees
    assert engine.check_points(msm.import_points_host(clean, "mont_flag")[0], CHECK_ALL).ok


# ---- refusals ----
def test_refusals(engine, pool, golden):
    n = 33
    d_p, d_s = dev(pool[0][: 96 * n]), dev(pool[1][: 32 * n])
    with forms(engine, "wire", "mont"):
        for call in (lambda: engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, 32, 253), lambda: engine.msm_short(pool[0][: 96 * n], pool[1][: 32 * n], 32, 253)):
            with pytest.raises(msm.MsmError) as e:
                call()
            assert e.value.code == EINVAL
    ed = golden["ed_n24_random"]
    d_ep, d_es = dev(ed["points"]), dev(ed["scalars"])
    for pform, sform in (("mont", "wire"), ("wire", "mont")):
        with forms(engine, pform, sform):
            with pytest.raises(msm.MsmError) as e:
                engine.ed_msm_device(d_ep.data_ptr(), d_es.data_ptr(), ed["n"])
            assert e.value.code == EINVAL
    assert engine.ed_msm_device(d_ep.data_ptr(), d_es.data_ptr(), ed["n"]) == ed["expected"]
    # an unknown form value: EINVAL, and the forms stay as they were
    engine.set_input_format("mont", "mont")
    try:
        for pf, sf in ((3, 0), (0, 2)):
            with pytest.raises(msm.MsmError) as e:
                engine.set_input_format(pf, sf)
            assert e.value.code == EINVAL
        assert engine.get_input_format() == ("mont", "mont")
    finally:
        engine.set_input_format("wire", "wire")


def test_short_scalars_with_native_points(engine, pool):
    """The short-scalar calls honour the point form: compact wire scalars, flagged points left out."""
    n = 257
    rng = random.Random(0x5407)
    ks = [rng.getrandbits(64) for _ in range(n)]
    flagged = [0, 64, 256]
    points = pool[0][: 96 * n]
    exp = wire_msm(engine, *without(points, R.encode_scalars(ks), flagged))
    pb, _ = native(points, b"", "mont_flag", "wire", flagged)
    sb = msm.encode_scalars(ks, 8)
    d_p, d_s = dev(pb), dev(sb)
    with forms(engine, "mont_flag", "wire"):
        assert engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, 8, 64) == exp
        assert engine.msm_short(pb, sb, 8, 64) == exp
        engine.set_bases_device(d_p.data_ptr(), n)
        assert engine.msm_fixed_base_short_device(d_s.data_ptr(), n, 8, 64) == exp


def test_window_partials_in_native_forms(engine, pool):
    n = 257
    points, scalars = pool[0][: 96 * n], pool[1][: 32 * n]
    flagged = [1, 63, 64, 256]
    exp = wire_msm(engine, *without(points, scalars, flagged))
    pb, sb = native(points, scalars, "mont_flag", "mont", flagged)
    d_p, d_s = dev(pb), dev(sb)
    with forms(engine, "mont_flag", "mont"):
        recs = engine.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 0, 16)
    assert combine_partials_bytes(recs) == exp


def test_compute_msm_options(golden):
    """compute_msm(point_form=..., scalar_form=...): the Python mirror of the node option; its engine goes back to wire."""
    case = golden["g1_n33_random"]
    ex, ey = R.decode_result(case["expected"])
    pb, sb = native(case["points"], case["scalars"], "mont_flag", "mont")
    assert msm.compute_msm(pb, sb, log_result=False, point_form="mont_flag", scalar_form="mont") == {"x": ex, "y": ey}
    assert msm.compute_msm(case["points"], case["scalars"], log_result=False) == {"x": ex, "y": ey}
    assert msm.compute_msm(b"", b"", log_result=False, point_form="mont", scalar_form="mont") == {"x": 0, "y": 1}
    with pytest.raises(ValueError):
        msm.compute_msm(pb[:-8], sb, log_result=False, point_form="mont_flag", scalar_form="mont")


# ---- the default format is untouched ----
def test_default_format_still_answers_the_goldens(engine, golden):
    assert engine.get_input_format() == ("wire", "wire")
    for name, case in sorted(golden.items()):
        if name.startswith("g1_"):
            assert wire_msm(engine, case["points"], case["scalars"]) == case["expected"], name
            assert engine.msm(case["points"], case["scalars"]) == case["expected"], name
