"""Native input forms, host side (include/msm377.h "native input forms"): msm377_g1_import_points_host,
msm377_import_scalars_host and msm377_g1_result_to_native against the Python-integer codecs of host/codecs.py -- a
third implementation that shares nothing with the C ones.  No GPU."""
import ctypes
import os
import random
import re

import pytest

import pyref as R
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

P, Q = R.P, R.R_ORDER
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mont_record(vx: int, vy: int, flag=None) -> bytes:
    """A record from RAW Montgomery values (not from the point they stand for)."""
    rec = vx.to_bytes(48, "little") + vy.to_bytes(48, "little")
    return rec if flag is None else rec + bytes([flag]) + bytes(7)


def edge_values():
    rng = random.Random(0x377)
    return [0, 1, P - 1, Q - 1] + [rng.randrange(P) for _ in range(60)]


@pytest.mark.parametrize("form", ["mont", "mont_flag"])
def test_point_import_matches_the_codecs(form):
    vals = edge_values()
    flag = 0 if form == "mont_flag" else None
    buf = b"".join(mont_record(vx, vy, flag) for vx, vy in zip(vals, reversed(vals)))
    wire, mask = msm.import_points_host(buf, form)
    assert R.decode_points(wire) == msm.decode_points_native(buf, form)
    # and by the definition itself: a value v means v * 2^-384 mod p
    inv = pow(1 << 384, -1, P)
    assert R.decode_points(wire) == [(vx * inv % P, vy * inv % P) for vx, vy in zip(vals, reversed(vals))]
    assert not any(mask)


def test_point_encoder_round_trips_through_the_importer():
    pts = [R.G, R.mul(R.G, 5), (0, 1), (P - 1, 1)]
    for form in ("mont", "mont_flag"):
        wire, _ = msm.import_points_host(msm.encode_points_native(pts, form), form)
        assert wire == R.encode_points(pts)
    assert msm.import_points_host(R.encode_points(pts), "wire")[0] == R.encode_points(pts)


def test_scalar_import_matches_the_codecs():
    rng = random.Random(0x256)
    raw = [0, 1, Q - 1, P % (1 << 256), Q, Q + 1, 2 * Q, (1 << 256) - 1, (1 << 255), (1 << 256) - Q] + [rng.getrandbits(256) for _ in range(60)]
    buf = b"".join(v.to_bytes(32, "little") for v in raw)
    got = R.decode_scalars(msm.import_scalars_host(buf, "mont"))
    assert got == msm.decode_scalars_native(buf, "mont")
    inv = pow(1 << 256, -1, Q)
    assert got == [v * inv % Q for v in raw]  # fully reduced, whatever the raw value
    assert all(k < Q for k in got)
    ks = [0, 1, Q - 1, 12345]
    assert msm.import_scalars_host(msm.encode_scalars_native(ks, "mont"), "mont") == R.encode_scalars(ks)
    assert msm.import_scalars_host(buf, "wire") == buf


def test_empty_inputs():
    assert msm.import_points_host(b"", "mont_flag") == (b"", [])
    assert msm.import_points_host(b"", "mont") == (b"", [])
    assert msm.import_scalars_host(b"", "mont") == b""
    lib = msm.load_library()
    assert lib.msm377_g1_import_points_host(None, 0, 2, None, None) == 0
    assert lib.msm377_import_scalars_host(None, 0, 1, None) == 0


@pytest.mark.parametrize("n", [33, 48, 65])
def test_flags_set_exactly_their_mask_bits(n):
    flagged = {0, 31, 32, n - 1}
    pts = [R.mul(R.G, i + 2) for i in range(n)]
    buf = bytearray(msm.encode_points_native(pts, "mont_flag"))
    for k, i in enumerate(sorted(flagged)):
        buf[104 * i : 104 * i + 96] = b"\xff" * 96  # garbage: never interpreted
        buf[104 * i + 96] = (1, 0xFF, 0x80, 2)[k]  # any non-zero byte flags
        buf[104 * i + 97 : 104 * i + 104] = b"\xaa" * 7  # ignored padding
    wire, mask = msm.import_points_host(bytes(buf), "mont_flag")
    assert len(mask) == (n + 31) // 32
    assert {i for i in range(n) if (mask[i >> 5] >> (i & 31)) & 1} == flagged
    assert all(w >> 32 == 0 for w in mask)
    got = R.decode_points(wire)
    for i in range(n):
        assert got[i] == (R.G if i in flagged else pts[i]), i
    assert msm.decode_points_native(bytes(buf), "mont_flag") == [None if i in flagged else pts[i] for i in range(n)]
    # a NULL mask pointer is accepted
    out = ctypes.create_string_buffer(96 * n)
    assert msm.load_library().msm377_g1_import_points_host(bytes(buf), n, 2, ctypes.addressof(out), None) == 0
    assert out.raw == wire


def test_a_coordinate_of_p_or_more_is_handed_on_unchanged():
    """Such a value is no Montgomery residue: the check calls must see it as the caller wrote it."""
    rec = mont_record(P, 5) + mont_record(7, (1 << 384) - 1)
    wire, _ = msm.import_points_host(rec, "mont")
    assert wire == rec


def test_result_to_native_round_trips():
    for pt in (R.G, R.mul(R.G, 0xABCDEF), (P - 1, 1)):
        rec = msm.result_to_native(R.encode_result(pt))
        assert len(rec) == 104 and rec[96:] == bytes(8)
        assert msm.decode_points_native(rec, "mont_flag") == [pt]
        assert msm.import_points_host(rec, "mont_flag")[0] == R.encode_result(pt)
    ident = msm.result_to_native(R.encode_result(None))
    assert ident[96] == 1 and ident[97:] == bytes(7)
    assert msm.decode_points_native(ident, "mont_flag") == [None]
    with pytest.raises(msm.MsmError) as e:
        msm.result_to_native(P.to_bytes(48, "little") + bytes(48))
    assert e.value.code == EINVAL


def test_bad_form_values_are_einval():
    lib = msm.load_library()
    out = ctypes.create_string_buffer(104)
    assert lib.msm377_g1_import_points_host(bytes(104), 1, 3, ctypes.addressof(out), None) == EINVAL
    assert lib.msm377_import_scalars_host(bytes(32), 1, 2, ctypes.addressof(out)) == EINVAL
    assert lib.msm377_g1_import_points_host(None, 1, 1, ctypes.addressof(out), None) == EINVAL
    assert lib.msm377_g1_result_to_native(None, ctypes.addressof(out)) == EINVAL
    assert lib.msm377_ctx_set_input_format(None, 0, 0) == EINVAL
    with pytest.raises(ValueError):
        msm.import_points_host(bytes(96), "affine")
    with pytest.raises(ValueError):
        msm.encode_points_native([None], "mont")


def test_header_declares_the_new_boundary():
    with open(os.path.join(ROOT, "include", "msm377.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = ctypes.CDLL(msm.library_path())
    for name in ("msm377_ctx_set_input_format", "msm377_ctx_get_input_format", "msm377_g1_import_points_host", "msm377_import_scalars_host",
                 "msm377_g1_result_to_native"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
    for macro, value in (("MSM377_POINTS_WIRE", 0), ("MSM377_POINTS_MONT", 1), ("MSM377_POINTS_MONT_FLAG", 2), ("MSM377_SCALARS_WIRE", 0), ("MSM377_SCALARS_MONT", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
