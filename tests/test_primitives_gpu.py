"""The gfx950 build of the field and curve primitives, and the arithmetic that exists only in the kernel headers, one
case per lane (or per lane quad) on the GPU: csrc/libmsm377_primtest.so, built by build() from
tests/native/primitives_device.hip.  Same operand tables as tests/test_primitives_host.py (tests/lazy_model.py).

Two separate demands: the device result equals the host build's BIT FOR BIT (one source, two compilers), and it meets
the Python contract.  A missing test library is a failure, not a skip.
"""
import numpy as np
import pytest

import lazy_model as M
import pyref as R

pytestmark = pytest.mark.gpu

FIELDS = ("Fp", "Fq")
# ragged ends: n mod 4, n mod 64 and n mod 256 all non-zero (the launchers use 256-thread blocks; a quad case takes 4 lanes)
RAGGED = (1, 3, 67, 259, 1031)


@pytest.fixture(scope="module")
def dev():
    return M.device_backend()  # a missing library fails here


@pytest.fixture(scope="module")
def host():
    return M.host_backend()


@pytest.fixture(scope="module", params=FIELDS)
def fm(request):
    return M.FieldModel(request.param)


def same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), (what, "first differing case", int(np.argwhere((a != b).reshape(len(a), -1).any(axis=1))[0][0]))


def all_lanes_agree(out4, what):
    """Every lane of a quad holds the full result: four identical copies per case."""
    for q in range(1, 4):
        same(out4[:, q], out4[:, 0], (what, "lane", q))
    return np.ascontiguousarray(out4[:, 0])


def test_field_ops_device_equals_host_and_contract(dev, host, fm):
    seen = set()
    for op, label, ins in M.field_cases(fm):
        got = dev.field(fm, op, ins)
        same(got, host.field(fm, op, ins), (fm.name, op, label))
        M.check_field_case(fm, op, label, ins, got)
        seen.add(op)
    assert seen == set(M.FIELD_OPS)
    # ragged launches: the last wave, the last block and the grid end inside the data
    op, label, ins = next(c for c in M.field_cases(fm, n_random=0) if c[0] == "mul_lz")
    big = [np.concatenate([x] * 60) for x in ins]
    for n in RAGGED:
        assert n % 4 and n % 64 and n % 256
        cut = [x[:n] for x in big]
        got = dev.field(fm, op, cut)
        same(got, host.field(fm, op, cut), (fm.name, "ragged", n))


def test_edwards_formulas_device_equals_host_and_contract(dev, host, fm):
    cm = M.CurveModel(fm)
    for op, case in M.te_point_cases(cm).items():
        out, flags = dev.te(fm, op, case[0], case[1], case[2])
        hout, hflags = host.te(fm, op, case[0], case[1], case[2])
        same(out, hout, (fm.name, op)), same(flags, hflags, (fm.name, op, "flags"))
        M.check_te_point_case(cm, op, case, out, flags)
    for name, case in M.te_poly_cases(cm).items():
        out, flags = dev.te(fm, name.split()[0], case[0], case[1], case[2])
        hout, hflags = host.te(fm, name.split()[0], case[0], case[1], case[2])
        same(out, hout, (fm.name, name)), same(flags, hflags, (fm.name, name, "flags"))
        M.check_te_poly_case(cm, name, case, out)
    rows, exp = M.te_zero_cases(fm)
    _, flags = dev.te(fm, "is_zero", rows, np.zeros_like(rows), np.zeros(len(rows), dtype=np.uint32))
    assert flags.tolist() == exp
    if fm.name == "Fp":
        for op, (rows, negs, exps) in M.te_from_base_cases(cm).items():
            out, flags = dev.te(fm, op, np.zeros_like(rows), rows, negs)
            same(out, host.te(fm, op, np.zeros_like(rows), rows, negs)[0], op)
            for i, o in enumerate(out.tolist()):
                cm.check_ext(o, exps[i], (op, i))
            assert not flags.any()


def test_xyzz_formulas_device_equals_host_and_contract(dev, host):
    fm = M.FieldModel("Fp")
    cases = M.g1_point_cases(fm)
    for op, case in cases.items():
        out = dev.g1(op, case[0], case[1], case[2])
        same(out, host.g1(op, case[0], case[1], case[2]), op)
        for i, o in enumerate(out.tolist()):
            M.check_g1_words(fm, o, case[3][i], (op, case[4][i]))
    for op, (a, b, exps, lows) in M.guard_false_positive_cases(fm).items():  # both guards' false-positive side
        M.check_guard_cases(dev, fm, op, a, b, lows)
        out = dev.g1(op, a, b, np.zeros(len(a), dtype=np.uint32))
        same(out, host.g1(op, a, b, np.zeros(len(a), dtype=np.uint32)), (op, "guard"))
        for i, o in enumerate(out.tolist()):
            M.check_g1_words(fm, o, exps[i], (op, "guard false positive, low limb of P", lows[i]))
    pts = cases["add_lz"][0]
    zero = np.zeros(len(pts), dtype=np.uint32)
    out = dev.g1("canon_pt", pts, np.zeros_like(pts), zero)
    same(out, host.g1("canon_pt", pts, np.zeros_like(pts), zero), "canon_pt")
    for o, a in zip(out.tolist(), pts.tolist()):
        for c in range(4):
            assert o[13 * c : 13 * c + 13] == M.nform_limbs(M.value(a[13 * c : 13 * c + 13]) % fm.P, 13)


def test_strict_g1_doublings_device_equals_host_and_contract(dev, host):
    """G1::dbl (through canon_pt, on every stored representation; 2-torsion with Y = 0 and Y = p -> ZZ limb-zero) and
    G1::dbl_affine, the strict formulas the batch kernels call."""
    fm = M.FieldModel("Fp")
    rows, exps, labels = M.g1_dbl_cases(fm)
    zero = np.zeros(len(rows), dtype=np.uint32)
    out = dev.g1("dbl", rows, np.zeros_like(rows), zero)
    same(out, host.g1("dbl", rows, np.zeros_like(rows), zero), "dbl")
    M.check_g1_doubles(fm, out, exps, labels, "dbl")
    rows, exps, labels = M.g1_dbl_affine_cases(fm)
    zero = np.zeros(len(rows), dtype=np.uint32)
    out = dev.g1("dbl_affine", np.zeros_like(rows), rows, zero)
    same(out, host.g1("dbl_affine", np.zeros_like(rows), rows, zero), "dbl_affine")
    M.check_g1_doubles(fm, out, exps, labels, "dbl_affine")


def test_strict_edwards_formulas_device_equals_host_and_contract(dev, host):
    """EdT<Fq, EdK29> madd, add, dbl, dbl_nt, make_base, cneg: the formulas of k_edbm_row_bases, k_edbm_entries and
    k_edbm_down<table>."""
    cm = M.CurveModel(M.FieldModel("Fq"))
    cases = M.ed_strict_cases(cm)
    assert set(cases) == set(M.ED_OPS)
    for op, case in cases.items():
        out = dev.ed(op, case[0], case[1], case[2])
        same(out, host.ed(op, case[0], case[1], case[2]), ("Ed", op))
        M.check_ed_strict_case(cm, op, case, out)


def test_inversion_walks_take_both_arms_on_the_device(dev, host, fm):
    """FpInverse / FqInverse::inverse_mont, one case per lane, each lane its own branch sequence: device == host bit for
    bit and == pow(a, -1, p) in Montgomery form, with the arm counts of the case list stated (the floors themselves are
    asserted from the k-model in tests/test_primitives_host.py)."""
    cases = M.inverse_cases(fm)
    short = sum(1 for _, k, _ in cases if k < M.INVERSE_WALK[fm.name]["short_below"])
    assert short >= 8 and len(cases) - short >= 8
    a = M.arr([M.nform_limbs(v, fm.N) for v, _, _ in cases])
    ins = [a] + [np.zeros_like(a)] * 3
    got = dev.field(fm, "inverse_mont", ins)
    same(got, host.field(fm, "inverse_mont", ins), (fm.name, "inverse_mont"))
    M.check_field_case(fm, "inverse_mont", "both arms", ins, got)
    for n in (1, 67):  # a ragged launch: idle lanes beside walking ones
        same(dev.field(fm, "inverse_mont", [x[:n] for x in ins]), got[:n], (fm.name, "inverse_mont ragged", n))


def test_te_add_quad_is_the_thread_level_addition(dev, fm):
    """te_add_quad<Fp> / te_add_quad<Fq>: the same products as TeLazy::add, spread over four lanes -- bit-identical to it,
    every lane holding the whole sum, adjacent quads carrying different operands; and the contract on top."""
    cm = M.CurveModel(fm)
    kind = fm.index  # 0: TeDev, 1: EdDev
    case = M.te_point_cases(cm)["add"]
    out4, flags4 = dev.add_quad(kind, case[0], case[1])
    out = all_lanes_agree(out4, (fm.name, "te_add_quad"))
    thread, _ = dev.te(fm, "add", case[0], case[1], case[2])
    same(out, thread, (fm.name, "te_add_quad vs add"))
    M.check_te_point_case(cm, "add", case, out, flags4[:, 0])
    assert not flags4.any()
    poly = M.te_poly_cases(cm)["add"]
    out4, _ = dev.add_quad(kind, poly[0], poly[1])
    out = all_lanes_agree(out4, (fm.name, "te_add_quad poly"))
    same(out, dev.te(fm, "add", poly[0], poly[1], poly[2])[0], (fm.name, "te_add_quad vs add, corners"))
    M.check_te_poly_case(cm, "add", poly, out)
    ta, tb, tout = np.concatenate([poly[0]] * 2), np.concatenate([poly[1]] * 2), np.concatenate([out4] * 2)
    for n in RAGGED:  # whole quads stay together at a ragged end
        assert n < len(ta)
        o4, _ = dev.add_quad(kind, ta[:n], tb[:n])
        same(o4, tout[:n], (fm.name, "ragged", n))


def test_te_madd_quad_is_the_thread_level_mixed_addition(dev, fm):
    """te_madd_quad fed the way k_accumulate_quad feeds it (lane q one coordinate of the record, 0 and 1 swapped and 2
    negated limb-wise for a negated point): bit-identical to TeLazy::madd."""
    cm = M.CurveModel(fm)
    for name in ("points", "corners"):
        case = M.te_point_cases(cm)["madd"] if name == "points" else M.te_poly_cases(cm)["madd"]
        out = all_lanes_agree(dev.madd_quad(fm, case[0], case[1], case[2]), (fm.name, "te_madd_quad", name))
        thread, flags = dev.te(fm, "madd", case[0], case[1], case[2])
        same(out, thread, (fm.name, "te_madd_quad vs madd", name))
        if name == "points":
            M.check_te_point_case(cm, "madd", case, out, flags)
        else:
            M.check_te_poly_case(cm, "madd", case, out)
            ta, tb, tn, tout = (np.concatenate([x] * 2) for x in (case[0], case[1], case[2], out))
            for n in RAGGED:
                assert n < len(ta)
                same(all_lanes_agree(dev.madd_quad(fm, ta[:n], tb[:n], tn[:n]), n), tout[:n], (fm.name, "ragged", n))


def test_g1_add_quad_and_its_branches(dev):
    """g1_add_quad: pyref's sum and the storage invariant on real points in edge representations, P = Q, P = -Q,
    identity operands (the generic fallback on a whole quad), and a P whose low limb is 1, 2, 3 without P being 0 mod p."""
    fm = M.FieldModel("Fp")
    case = M.g1_point_cases(fm)["add_lz"]
    labels = case[4]
    assert any("P = Q" in l for l in labels) and any("P = -Q" in l for l in labels) and any("identity" in l for l in labels)
    out4, _ = dev.add_quad(2, case[0], case[1])
    out = all_lanes_agree(out4, "g1_add_quad")
    for i, o in enumerate(out.tolist()):
        M.check_g1_words(fm, o, case[3][i], ("g1_add_quad", labels[i]))
    a, b, exps, lows = M.guard_false_positive_cases(fm)["add_lz"]
    assert lows == [1, 2, 3]
    M.check_guard_cases(dev, fm, "add_lz", a, b, lows)  # with the device's own mul_lz the low limb of P is 1, 2, 3
    out = all_lanes_agree(dev.add_quad(2, a, b)[0], "g1_add_quad guard")
    for i, o in enumerate(out.tolist()):
        M.check_g1_words(fm, o, exps[i], ("g1_add_quad, guard false positive, low limb of P", lows[i]))
    for n in (1, 3, 67):
        same(dev.add_quad(2, case[0][:n], case[1][:n])[0], out4[:n], ("ragged", n))


def test_aff_wire_source_load(dev):
    """AffWireSource::load, the lazy wire -> Edwards map of the batched affine conversion: n1 / z and n2 / z are the
    affine Edwards coordinates, the bounds its comments state hold, and the points the model cannot represent return true."""
    fm = M.FieldModel("Fp")
    raw, pts = M.aff_wire_cases()
    assert len(pts) % 4 and len(pts) % 64
    out, flags = dev.aff_wire(raw)
    M.check_aff_wire(fm, pts, out, flags.tolist())
    assert sum(b for _, b in pts) >= 5


@pytest.mark.parametrize("kind", sorted(M.RECORD_KINDS))
def test_bucket_record_round_trip(dev, kind):
    """store_record -> load_record / load_record_quad -> store_coord: every word of every coordinate survives (all-ones
    words in every position), the slots' pad words are WRITTEN as zero (the memory held all-ones), the quad load equals
    the thread load on every lane."""
    name, nl, slot = M.RECORD_KINDS[kind]
    pts = M.record_cases(nl)
    assert len(pts) % 4 and len(pts) % 64
    rec, out_t, out_q, rec2 = dev.records(kind, pts)
    same(out_t, pts, (name, "load_record(store_record(x))"))
    same(all_lanes_agree(out_q, (name, "load_record_quad")), pts, (name, "load_record_quad(store_record(x))"))
    exp = np.zeros((len(pts), 4, slot), dtype=np.uint32)
    exp[:, :, :nl] = pts.reshape(len(pts), 4, nl)
    same(rec, exp.reshape(len(pts), 4 * slot), (name, "record layout, pads zero"))
    same(rec2, rec, (name, "store_coord per lane"))
