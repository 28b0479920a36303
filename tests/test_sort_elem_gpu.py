"""The two-level sort of the 2^15-bucket path with packed 4-byte sort_temp elements (csrc/common.hpp SortElem4,
kernels/sort.hpp k_partition_staged / k_local_sort_lds; MSM377_SORT_ELEM=4) and with the 8-byte form (=8).  Every case
runs on both, each result is compared with the CPU oracle and the two with each other; last_sort_elem_bytes() must read
4 and 8, so that a case cannot pass on the same kernels twice.  The sizes are the smallest the path runs at: it starts above
the narrow path's 2^16 points, so n = 65537 and a ragged 70001.  Host side of the element: tests/test_sort_elem_host.py."""
import random

import numpy as np
import pytest

import pyref as R
import stage_model as M
import util
import webgpu_msm_bls12_377_amd as msm

pytestmark = pytest.mark.gpu

N_MIN, N_RAGGED = 65537, 70001
NB, KRANGE = 1 << 15, 128
LS_CACHE_LARGEST = 8192  # the largest region length any build of k_local_sort_lds keeps in registers (kernels/sort.hpp)
FORMS = (4, 8)
A0, D = 0x50E7E1E4, 0xB17E5


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def pool(oracle):
    """70001 subgroup points P_i = [A0 + i D]G; every case takes a prefix."""
    return util.oracle_gen_points(oracle, N_RAGGED, A0, D)


def make_engine(form, extra_env=()):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_SORT_ELEM", str(form))
        for k, v in extra_env:
            mp.setenv(k, v)
        return msm.MsmEngine(1 << 17)


@pytest.fixture(scope="module")
def engines():
    """One context per form, shared by the cases that need no other setting."""
    engs = {form: make_engine(form) for form in FORMS}
    yield engs
    for e in engs.values():
        e.close()


def run_both(engs, call, expected, label, sort_ran=True):
    """call(engine) on the packed and on the 8-byte context: both equal the oracle's result, hence each other."""
    got = {}
    for form in FORMS:
        got[form] = call(engs[form])
        if sort_ran:
            assert engs[form].last_sort_elem_bytes() == form, (label, form, "the call did not run the form it is meant to test")
        assert got[form] == expected, (label, "%d-byte elements differ from the oracle" % form)
    assert got[4] == got[8], label


def check_rows(engine, slot, col, bias, key_unsigned, label):
    """row_ptr and val_idx of a slot against the model: every row holds exactly the entries of its key, with their signs
    (order inside a row is free: the comparison is per row, as sets)."""
    info, st = engine.read_stage_ex(slot, want=("row_ptr", "val_idx"))
    tag = (label, slot)
    assert info.columns == len(col) and info.row_ptr_len == NB + 2, tag
    key, sign = M.keys_and_signs(col, bias, key_unsigned)
    counts = np.bincount(key, minlength=NB + 1)
    rp, vi = st["row_ptr"].astype(np.int64), st["val_idx"]
    assert rp[0] == 0 and rp[-1] == len(col), tag
    assert np.array_equal(np.diff(rp), counts), tag  # every row_ptr word
    entry = (vi & 0x7FFFFFFF).astype(np.int64)
    assert np.array_equal(np.sort(entry), np.arange(len(col))), tag  # every entry once
    assert np.array_equal(key[entry], np.repeat(np.arange(NB + 1), counts)), tag  # ... in the row of its key
    assert np.array_equal(sign[entry], (vi >> 31).astype(bool)), tag  # ... with its sign
    return st


def digit_columns(ks, g):
    """M.digit_matrix, recoding every distinct scalar once (the skewed cases repeat one or three scalars 70001 times)."""
    distinct = sorted(set(ks))
    if len(distinct) * 2 > len(ks) or g.name == "glv8":
        cols, flags = M.digit_matrix(ks, g)
    else:
        small, flags = M.digit_matrix(distinct, g)
        where = np.searchsorted(np.array(distinct, dtype=object), np.array(ks, dtype=object))
        cols = [c[where.astype(np.int64)] for c in small]
    assert flags == 0, "the case's scalars fit the geometry it is meant to run"
    return cols


def staged_call(engs, g, ks, pts, expected, slots, label, call=None, cols=None):
    """The case under stage capture on both forms: result, then the rows of `slots`; the two forms' rows agree as sets
    because both agree with the model."""
    if cols is None:
        cols = digit_columns(ks, g)
    wire = R.encode_scalars(ks)
    for form in FORMS:
        e = engs[form]
        e.set_stage_capture(2)
        try:
            got = call(e) if call else e.msm(pts, wire)
            assert e.last_sort_elem_bytes() == form, (label, form)
            assert e.last_geometry() == (len(g.slots), 15), (label, form)
            for slot in slots:
                s = g.slots[slot]
                check_rows(e, slot, cols[slot], s.bias, s.key_unsigned, "%s, %d-byte elements" % (label, form))
            assert got == expected, (label, form)
        finally:
            e.set_stage_capture(0)
    return cols


# ---- uniform scalars ----
@pytest.mark.parametrize("n", [N_MIN, N_RAGGED])
def test_uniform_scalars(engines, oracle, pool, n):
    pts, ks = pool[: 96 * n], R.encode_scalars(R.rand_scalars(0x50E70000 + n, n))
    exp = util.oracle_msm(oracle, pts, ks)
    d_p, d_s = dev(pts), dev(ks)

    def call(e):
        with util.edwards_only(e):
            return e.msm_device(d_p.data_ptr(), d_s.data_ptr(), n)

    run_both(engines, call, exp, "uniform n=%d" % n)


# ---- digit edges ----
SIGNED_LIMBS = (0x8000, 0x7FFF, 127, 128, 129, 0xFF80, 0xFF7F, 0xFF81, 0, 1, 0xFFFF, 0x8001, 255, 256, 257, 0x7F80, 0x7F7F, 0x8080, 0x8081)
UNSIGNED_FIELDS = (0x7FFF, 127, 128, 129, 0, 1, 0x7F80, 0x7F7F, 255, 256, 257, 0x7FFE)


def edge_scalars(n):
    """Scalars for the even geometry (thirteen signed 16-bit windows, three unsigned 15-bit ones from bit 208) whose
    first 8192 lay the corner limbs out over all windows: 0x8000 (digit -2^15: key NB, sub 128 in the last range),
    0x7fff (key 2^15 - 1, and key NB when a carry comes in), 127 / 128 / 129 and their negatives at the border of ranges
    0 and 1, 0x7f80 / 0x7f7f at the border of the last range.  The limb of window w of scalar i steps through the list
    with i and w, at a step that changes from one run of the list to the next, so every window meets every corner behind
    every neighbour below it: with and without a carry coming in."""
    ks = R.rand_scalars(0xED6E5, n)
    for i in range(8192):
        k = 0
        for w in range(13):
            k |= SIGNED_LIMBS[(i + (5 + i // len(SIGNED_LIMBS)) * w) % len(SIGNED_LIMBS)] << (16 * w)
        for j in range(3):
            f = UNSIGNED_FIELDS[(i + (7 + i // len(UNSIGNED_FIELDS)) * j) % len(UNSIGNED_FIELDS)]
            if j == 2:
                f &= 0x3FFF  # below 2^252: nothing carries out of the top window
            k |= f << (208 + 15 * j)
        ks[i] = k
    return ks


def test_digit_edges(engines, oracle, pool):
    n = N_MIN
    g = M.even16()
    pts, ks = pool[: 96 * n], edge_scalars(n)
    cols = digit_columns(ks, g)
    for slot in range(16):  # the corners are there before anything runs
        key, sign = M.keys_and_signs(cols[slot], g.slots[slot].bias, g.slots[slot].key_unsigned)
        want = {127, 128, 129, 0x7FFF} | ({NB} if slot < 13 else set())
        if slot == 15:
            want.discard(0x7FFF)  # the top window is kept below 2^14
        assert want <= set(np.unique(key).tolist()), (slot, sorted(want - set(np.unique(key).tolist())))
        if slot < 13:
            assert sign[key == NB].all() and sign[key == 128].any() and not sign[key == 128].all(), slot
    exp = util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    staged_call(engines, g, ks, pts, exp, range(16), "digit edges", cols=cols)


# ---- skew ----
@pytest.mark.parametrize("distinct", [1, 3])
def test_skewed_scalars(engines, oracle, pool, distinct):
    """One scalar repeated: every window has ONE region of 70001 elements, far beyond what k_local_sort_lds keeps in
    registers -- the streamed arm -- and one row of 70001 entries.  Three distinct scalars: three such rows."""
    n = N_RAGGED
    assert n // distinct > LS_CACHE_LARGEST
    base = R.rand_scalars(0x5CE30 + distinct, distinct)
    rnd = random.Random(0x5CE3)
    ks = [base[rnd.randrange(distinct)] for _ in range(n)]
    pts = pool[: 96 * n]
    # (the oracle's own MSM takes seconds on rows this long: the closed form over P_i = [A0 + i D]G, one oracle scalar multiplication)
    exp = util.closed_form(oracle, sum(k * (A0 + i * D) for i, k in enumerate(ks)))
    g = M.even16()
    staged_call(engines, g, ks, pts, exp, (0, 12, 15), "skew, %d distinct" % distinct)


# ---- sixteen equal windows: the top window's ranges are narrowed ----
def test_sixteen_equal_windows(oracle, pool):
    """MSM377_EVEN_WINDOWS=0: scalars below r leave window 15 thirteen bits, so its ranges are narrowed (win_shift 2 or 3:
    32 or 16 keys per range) and sub = key - range * (KRANGE >> shift)."""
    n = N_MIN
    g = M.equal16()
    pts, ks = pool[: 96 * n], R.rand_scalars(0x16E0, n)
    cols = digit_columns(ks, g)
    top = M.key_max_word(cols[15], 1 << 15, False) & 0xFFFF
    assert (1 << 12) <= top < (1 << 14), "win_shift of the top window is 2 or 3"
    exp = util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    engs = {form: make_engine(form, [("MSM377_EVEN_WINDOWS", "0")]) for form in FORMS}
    try:
        staged_call(engs, g, ks, pts, exp, (0, 14, 15), "equal windows", cols=cols)
    finally:
        for e in engs.values():
            e.close()


# ---- short scalars: the UNS instantiations, the unsigned top slot ----
def test_short_scalars(engines, oracle, pool):
    n, sb, bits = N_MIN + 1, 8, 64
    g = M.short(bits, 15)
    rnd = random.Random(0x5407)
    ks = [rnd.getrandbits(bits) for _ in range(n)]
    ks[:4] = [(1 << bits) - 1, 0, 0x8000_8000_8000_8000, 0x7FFF_7FFF_7FFF_7FFF]
    pts = pool[: 96 * n]
    exp = util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    compact = b"".join(k.to_bytes(sb, "little") for k in ks)
    top = len(g.slots) - 1
    staged_call(engines, g, ks, pts, exp, (0, top - 1, top), "short 64-bit", call=lambda e: e.msm_short(pts, compact, sb, bits))


# ---- the GLV front end: 2 n columns ----
def test_glv_front_end(engines, oracle, pool):
    n = N_MIN
    g = M.glv8()
    pts, ks = pool[: 96 * n], R.rand_scalars(0x61F2, n)
    ks[:3] = [0, 1, R.R_ORDER - 1]
    exp = util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    for e in engines.values():
        e.set_g1_form("weierstrass")
        e.set_glv(True)
    try:
        cols = staged_call(engines, g, ks, pts, exp, (0, 7), "glv")
        assert len(cols[0]) == 2 * n
    finally:
        for e in engines.values():
            e.set_glv("auto")
            e.set_g1_form("edwards")


# ---- Edwards-BLS12: the same sort kernels ----
def test_edwards_bls12(engines, oracle):
    n = N_MIN
    pts = util.oracle_ed_gen_points(oracle, n, 0xED5047, 0x2468ACE)
    ks = R.encode_scalars(R.rand_scalars(0xED50, n, R.ED_SUBGROUP))
    exp = util.oracle_ed_msm(oracle, pts, ks)
    d_p, d_s = dev(pts), dev(ks)
    run_both(engines, lambda e: e.ed_msm_device(d_p.data_ptr(), d_s.data_ptr(), n), exp, "edwards-bls12")
