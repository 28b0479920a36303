"""Point validation on the host (msm377_g1_check_points_host / msm377_ed_check_points_host): canonical, on-curve and
subgroup verdicts against tests/pyref.py.  CPU only: no context, no device."""
import ctypes

import pytest

import check_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from check_vectors import as_tuple, expected_report


@pytest.fixture(scope="module")
def g1_set():
    return V.g1_crafted()


@pytest.fixture(scope="module")
def ed_set():
    return V.ed_crafted()


def test_golden_inputs_have_no_findings(golden):
    assert golden
    for name, case in golden.items():
        check = msm.ed_check_points_host if name.startswith("ed_") else msm.check_points_host
        rep = check(case["points"], msm.CHECK_ALL)
        assert as_tuple(rep) == (case["n"], 0, 0, 0, None, 0), name
        assert rep.ok


def test_crafted_sets_cover_every_class(g1_set, ed_set):
    for _, verdicts in (g1_set, ed_set):
        assert 48 <= len(verdicts) <= 96
        for cls in (0, V.CANONICAL, V.CURVE, V.SUBGROUP):
            assert verdicts.count(cls) >= 6, (cls, verdicts)
        assert verdicts[0] == 0


def test_g1_small_order_and_cofactor_points_are_outside_the_subgroup():
    small = V.g1_small_order_points()
    pts = small + [R.add(R.mul(R.G, 1000 + i), t) for i, t in enumerate(small)] + V.g1_lifted_points(3)
    for pt in pts:
        assert V.g1_verdict(*pt) == V.SUBGROUP  # pyref
    rep = msm.check_points_host(R.encode_points(pts), msm.CHECK_ALL)
    assert as_tuple(rep) == (len(pts), 0, 0, len(pts), 0, V.SUBGROUP)


def test_ed_low_order_points_are_outside_the_subgroup():
    low = V.ed_low_order_points()
    pts = low + [R.ed_add(R.ED_G, t) for t in low]
    for pt in pts:
        assert V.ed_verdict(*pt) == V.SUBGROUP
    rep = msm.ed_check_points_host(R.ed_encode_points(pts), msm.CHECK_ALL)
    assert as_tuple(rep) == (len(pts), 0, 0, len(pts), 0, V.SUBGROUP)
    assert msm.ed_check_points_host(R.ed_encode_points([R.ED_ID]), msm.CHECK_ALL).ok  # the neutral element is a subgroup point


@pytest.mark.parametrize("flags", [1, 3, 7])
def test_g1_crafted_report(g1_set, flags):
    blob, verdicts = g1_set
    assert as_tuple(msm.check_points_host(blob, flags)) == expected_report(verdicts, flags)


@pytest.mark.parametrize("flags", [1, 3, 7])
def test_ed_crafted_report(ed_set, flags):
    blob, verdicts = ed_set
    assert as_tuple(msm.ed_check_points_host(blob, flags)) == expected_report(verdicts, flags)


@pytest.mark.parametrize("flags,normal", [(2, 3), (4, 7), (5, 7), (6, 7)])
def test_flags_normalise(g1_set, ed_set, flags, normal):
    assert msm.check_points_host(g1_set[0], flags) == msm.check_points_host(g1_set[0], normal)
    assert msm.ed_check_points_host(ed_set[0], flags) == msm.ed_check_points_host(ed_set[0], normal)


def test_off_curve_is_fine_without_the_curve_flag_and_cofactor_without_the_subgroup_flag():
    off = R.encode_points([(1, 1)])
    assert msm.check_points_host(off, 1).ok
    assert as_tuple(msm.check_points_host(off, 3)) == (1, 0, 1, 0, 0, V.CURVE)
    cof = R.encode_points([(R.P - 1, 0)])
    assert msm.check_points_host(cof, 3).ok
    assert as_tuple(msm.check_points_host(cof, 7)) == (1, 0, 0, 1, 0, V.SUBGROUP)


def test_cascade_counts_a_point_once():
    """x = p + 1 is not canonical and (1, 1) is not on the curve: one finding, in the first class."""
    assert not R.on_curve((1, 1))
    blob = R.encode_points([R.G]) + (R.P + 1).to_bytes(48, "little") + (1).to_bytes(48, "little")
    assert as_tuple(msm.check_points_host(blob, 7)) == (2, 1, 0, 0, 1, V.CANONICAL)
    assert not R.ed_on_curve((1, 1))
    blob = R.ed_encode_points([R.ED_G]) + (R.Q + 1).to_bytes(32, "little") + (1).to_bytes(32, "little")
    assert as_tuple(msm.ed_check_points_host(blob, 7)) == (2, 1, 0, 0, 1, V.CANONICAL)


def test_first_bad_is_the_lowest_index():
    pts = [R.mul(R.G, k + 1) for k in range(8)]
    blob = bytearray(R.encode_points(pts))
    blob[96 * 6 : 96 * 7] = R.encode_points([(R.P - 1, 0)])  # outside the subgroup at 6
    blob[96 * 3 : 96 * 4] = R.encode_points([(1, 1)])  # off the curve at 3
    blob[96 * 5 : 96 * 5 + 48] = R.P.to_bytes(48, "little")  # non-canonical at 5
    assert as_tuple(msm.check_points_host(bytes(blob), 7)) == (8, 1, 1, 1, 3, V.CURVE)
    assert as_tuple(msm.check_points_host(bytes(blob), 1)) == (8, 1, 0, 0, 5, V.CANONICAL)


def test_argument_errors_and_the_empty_report():
    lib = msm.load_library()
    rep = ctypes.create_string_buffer(48)
    pts = R.encode_points([R.G])
    for fn, one in ((lib.msm377_g1_check_points_host, pts), (lib.msm377_ed_check_points_host, R.ed_encode_points([R.ED_G]))):
        assert fn(one, 1, 0, ctypes.addressof(rep)) == -1  # MSM377_EINVAL
        assert fn(one, 1, 8, ctypes.addressof(rep)) == -1
        assert fn(one, 1, 0x17, ctypes.addressof(rep)) == -1
        assert fn(one, 1, 7, None) == -1
        assert fn(None, 1, 7, ctypes.addressof(rep)) == -1
        assert fn(None, 0, 7, ctypes.addressof(rep)) == 0
    for check in (msm.check_points_host, msm.ed_check_points_host):
        assert as_tuple(check(b"", 7)) == (0, 0, 0, 0, None, 0)
        with pytest.raises(msm.MsmError) as e:
            check(b"", 0)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        msm.check_points_host(b"\0" * 95)


def test_report_struct_layout():
    """msm377_check_report is 48 bytes: five u64, two u32; first_bad of a clean report is UINT64_MAX."""
    lib = msm.load_library()
    rep = (ctypes.c_uint64 * 6)(*([0xAAAAAAAAAAAAAAAA] * 6))
    assert lib.msm377_g1_check_points_host(R.encode_points([R.G, (1, 1)]), 2, 7, ctypes.addressof(rep)) == 0
    assert list(rep) == [2, 0, 1, 0, 1, V.CURVE]  # reason in the low half of the last word, `reserved` = 0 in the high half
    assert lib.msm377_g1_check_points_host(R.encode_points([R.G]), 1, 7, ctypes.addressof(rep)) == 0
    assert list(rep) == [1, 0, 0, 0, V.NONE, 0]


def test_strerror_knows_epoint():
    lib = msm.load_library()
    text = lib.msm377_strerror(-8).decode()
    assert text and text != "unknown error"
    others = [lib.msm377_strerror(c).decode() for c in range(0, -8, -1)] + [lib.msm377_strerror(-9).decode()]
    assert text not in others
    assert "point" in str(msm.MsmError(-8, "x"))
