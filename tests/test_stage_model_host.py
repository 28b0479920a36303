"""Pins tests/stage_model.py before the GPU is compared with it (tests/test_stage_geometries_gpu.py): for every window
geometry the digits rebuild the scalar under the geometry's weights, every digit lies in its documented range, the flags
fire exactly on the documented sets, the equal-16 recode is the oracle's and the short recode is the model that
tests/test_short_scalars_host.py already keeps.  No GPU."""
import random

import numpy as np
import pytest

import pyref as R
import stage_model as M
import util
from test_short_scalars_host import recode as short_recode

r = R.R_ORDER
FULL = {"equal16": M.equal16(), "even16": M.even16(), "narrow22": M.narrow22(), "wide13": M.wide13()}
# The scalar error is the final carry of the sixteen-window signed recode: digits in [-2^15, 2^15 - 1] reach at most
# sum (2^15 - 1) 2^(16 w) = 0x7FFF7FFF...7FFF, so exactly the scalars above that carry out.  The documented bound
# 2^255 - 2^239 = 0x7FFF8000 << 224 lies just above this threshold: everything from it on is an error, nothing below r is.
SCALAR_ERROR_FROM = sum(0x7FFF << (16 * w) for w in range(16)) + 1
assert r < (1 << 253) < SCALAR_ERROR_FROM <= (1 << 255) - (1 << 239)
ALL_FLAGS = M.ERR_SCALAR | M.ERR_GLV_RANGE | M.ERR_RERUN | M.ERR_SHORT_WIDTH


def planted(g, top_bits):
    """0, 1, r - 1; the boundary values 0, 1, 2^(c-1) - 1, 2^(c-1), 2^(c-1) + 1, 2^c - 1 in every window of the geometry,
    alone and over all-ones lower bits (which hand every window a carry, signed or unsigned); carries through all windows."""
    ks = [0, 1, r - 1]
    for s in g.slots:
        c = s.width
        if c == 0:
            continue
        for v in sorted({0, 1, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1}):
            if v >> c:
                continue
            ks.append(v << s.offset)
            ks.append((v << s.offset) | ((1 << s.offset) - 1))
    ks.append((1 << top_bits) - 1)
    for s in g.slots:  # a carry born in this window that runs through every window above it
        if s.width:
            up = ((1 << top_bits) - 1) >> (s.offset + s.width) << (s.offset + s.width)
            ks.append(up | (1 << (s.offset + s.width - 1)))
    return [k for k in ks if k >> 256 == 0]


def check_ranges(g, rec):
    L = g.bucket_log
    for d, s in zip(rec.digits, g.slots):
        if s.signed:
            assert -(1 << L) <= d <= (1 << L), (g.name, s, d)
        elif g.name == "short":
            assert 0 <= d <= (1 << L), (g.name, s, d)  # the short top digit: the rest plus a carry
        elif g.name == "wide13":
            assert 0 <= d <= (1 << L), (g.name, s, d)  # its top window reaches 2^19 with the carry
        else:
            assert 0 <= d < (1 << L), (g.name, s, d)
    for v, s in zip(rec.stored, g.slots):
        assert 0 <= v < (1 << (8 * g.digit_bytes)), (g.name, s, v)


def carry_out_of_signed(k, g):
    """Whether the signed windows hand a carry to the first unsigned one, from the range of a signed-digit sum: digits
    of c bits in [-2^(c-1), 2^(c-1) - 1] reach at most sum (2^(c-1) - 1) 2^offset, anything above carries."""
    signed = [s for s in g.slots if s.signed]
    low_bits = signed[-1].offset + signed[-1].width
    most = sum(((1 << (s.width - 1)) - 1) << s.offset for s in signed)
    return (k & ((1 << low_bits) - 1)) > most, low_bits


def must_rerun(k, g):
    """even16 / narrow22 / wide13: the scalar does not fit the unsigned top of the geometry."""
    carry, low_bits = carry_out_of_signed(k, g)
    if g.name == "wide13":
        return (k >> 234) + carry > (1 << 19)
    return k >> 253 != 0 or ((k >> low_bits) + carry) >> (253 - low_bits) != 0


@pytest.mark.parametrize("name", sorted(FULL))
def test_full_width_geometries(name):
    g = FULL[name]
    assert sum(s.width for s in g.slots) == (256 if name == "equal16" else 253)
    rnd = random.Random("stage-model/" + name)
    ks = planted(g, 253) + planted(g, 256) + R.rand_scalars(0x57A6E, 3000) + [rnd.getrandbits(256) for _ in range(2000)]
    ks += [SCALAR_ERROR_FROM - 1, SCALAR_ERROR_FROM, (1 << 255) - (1 << 239) - 1, (1 << 255) - (1 << 239), (1 << 253) - (1 << 238) - 1, (1 << 253) - (1 << 238), (1 << 253) - 1, 1 << 253]
    fired = 0
    for k in ks:
        rec = M.recode(k, g)
        assert len(rec.digits) == len(g.slots) == len(rec.stored)
        assert bool(rec.flags & M.ERR_SCALAR) == (k >= SCALAR_ERROR_FROM), hex(k)
        rerun = name != "equal16" and must_rerun(k, g)
        assert bool(rec.flags & M.ERR_RERUN) == rerun, (name, hex(k))
        assert rec.flags & ~(M.ERR_SCALAR | M.ERR_RERUN) == 0
        fired += bool(rec.flags)
        if k < r and name != "wide13":
            assert not rerun or k >= (1 << 253) - (1 << 238), hex(k)  # below that no scalar reruns
        if k < (1 << 253) - (1 << 238):
            assert rec.flags == 0, (name, hex(k))
        if not rec.flags:
            assert M.rebuild(rec.digits, g) == k, (name, hex(k))
            check_ranges(g, rec)
            for d, v, s in zip(rec.digits, rec.stored, g.slots):
                assert v == d + s.bias
    assert fired > 100


def test_rerun_thresholds_of_the_even_and_the_narrow_geometry():
    """The smallest scalar that reruns: every unsigned field all ones and a carry coming in -- 2^253 - 2^208 + the
    smallest 208-bit value whose signed digits carry (even), 2^253 - 2^132 + ... (narrow); none below 2^253 - 2^238."""
    for g, low in ((M.even16(), 208), (M.narrow22(), 132)):
        signed = [s for s in g.slots if s.signed]
        first = (1 << 253) - (1 << low) + sum(((1 << (s.width - 1)) - 1) << s.offset for s in signed) + 1
        assert M.recode(first, g).flags == M.ERR_RERUN
        assert M.recode(first - 1, g).flags == 0
        assert first >= (1 << 253) - (1 << 238)
        assert M.recode((1 << 253) - (1 << 238) - 1, g).flags == 0
    assert M.recode(r - 1, M.even16()).flags == 0 and M.recode(r - 1, M.narrow22()).flags == 0 and M.recode(r - 1, M.wide13()).flags == 0


def test_equal16_is_the_oracles_recode():
    oracle = util.load_oracle()
    g = M.equal16()
    ks = [k for k in planted(g, 253) + R.rand_scalars(0xE16, 3000) if k < SCALAR_ERROR_FROM]
    n = len(ks)
    chunks = np.zeros(16 * n, dtype=np.uint32)
    assert oracle.oracle_decompose_scalars_signed(R.encode_scalars(ks), n, 16, chunks.ctypes.data) == 0
    cols, flags = M.digit_matrix(ks, g)
    assert flags == 0
    for w in range(16):
        assert np.array_equal(cols[w].astype(np.uint32), chunks.reshape(16, n)[w]), w


@pytest.mark.parametrize("L", (11, 15))
def test_short_is_the_short_recode(L):
    rnd = random.Random(0x5407 + L)
    for bits in list(range(1, 40)) + [63, 64, 65, 127, 128, 129, 199, 200, 252, 253]:
        g = M.short(bits, L)
        assert len(g.slots) == bits // (L + 1) + 1
        ks = [k & ((1 << bits) - 1) for k in planted(g, bits)] + [rnd.getrandbits(bits) for _ in range(200)]
        for k in ks:
            rec = M.recode(k, g)
            digits, out = short_recode(k, bits, L)
            assert rec.digits == digits and out == 0 and rec.flags == 0, (bits, L, hex(k))
            assert M.rebuild(rec.digits, g) == k
            check_ranges(g, rec)
            assert rec.stored[-1] == digits[-1] + (0 if L == 15 else 1 << L)
            assert g.slots[-1].key_unsigned == (L == 15)
        for k in (1 << bits, (1 << bits) | 5, (1 << 256) - 1):  # the width excess: flagged, dropped before the recode
            if k >> 256 == 0:
                rec = M.recode(k, g)
                assert rec.flags == M.ERR_SHORT_WIDTH
                assert rec.digits == M.recode(k & ((1 << bits) - 1), g).digits


def test_glv_split_and_digits():
    lam, beta = M.glv_consts()
    assert (lam * lam + lam + 1) % r == 0 and lam.bit_length() == 127
    assert pow(beta, 3, R.P) == 1 and beta != 1
    assert M.phi(R.G) == R.mul(R.G, lam)
    g = M.glv8()
    rnd = random.Random(0x61F)
    halves = [k & ((1 << 127) - 1) for k in planted(g, 127)]
    ks = [0, 1, r - 1, lam - 1, lam, lam + 1] + R.rand_scalars(0x61E, 2000)
    ks += [(k1 % lam) + lam * k2 for k1 in halves[:60] for k2 in rnd.sample(halves, 4)]
    ks += [(k1 % lam) + lam * k2 for k2 in halves[:60] for k1 in rnd.sample(halves, 4)]
    for k in ks:
        if k >> 256:
            continue
        rec = M.recode(k, g)
        k1 = sum(d << (16 * w) for w, d in enumerate(rec.digits[:8]))
        k2 = sum(d << (16 * w) for w, d in enumerate(rec.digits[8:]))
        if rec.flags:
            assert rec.flags == M.ERR_GLV_RANGE and k >= r, hex(k)
            continue
        assert 0 <= k1 < lam and 0 <= k2 < (1 << 127) and k1 + lam * k2 == k == M.rebuild(rec.digits, g)
        assert (k1 + lam * k2) % r == k % r
        for half in (rec.digits[:8], rec.digits[8:]):
            assert all(-(1 << 15) <= d <= (1 << 15) for d in half[:7]) and 0 <= half[7] < (1 << 15)
        assert all(v == (d + (1 << 15)) & 0xFFFF for d, v in zip(rec.digits, rec.stored))
    for k in R.rand_scalars(0x61D, 500) + [r - 1]:
        assert M.recode(k, g).flags == 0  # none below r
    assert M.recode((1 << 256) - 1, g).flags == M.ERR_GLV_RANGE


def test_digit_matrix_layouts_and_csr():
    ks = R.rand_scalars(0xC52, 300)
    n = len(ks)
    for g in (M.equal16(), M.even16(), M.narrow22(), M.short(64, 15), M.short(64, 11), M.wide13(), M.glv8()):
        kk = [k & ((1 << 64) - 1) for k in ks] if g.name == "short" else ks
        cols, flags = M.digit_matrix(kk, g)
        assert flags == 0
        per_slot = {"wide13": 13 * n, "glv8": 2 * n}.get(g.name, n)
        assert len(cols) == (1 if g.name == "wide13" else len(g.slots)) and all(len(c) == per_slot for c in cols)
        assert cols[0].dtype == (np.uint32 if g.digit_bytes == 4 else np.uint16)
        for w, col in enumerate(cols):
            s = g.slots[w]
            c = M.csr(col, g.bucket_log, s.bias, s.key_unsigned)
            assert c.counts.sum() == per_slot and len(c.counts) == (1 << g.bucket_log) + 1
            key, sign = M.keys_and_signs(col, s.bias, s.key_unsigned)
            for k_ in (0, 1, int(key[0]), int(key.max())):
                assert c.row(k_) == sorted((e, int(sign[e])) for e in range(per_slot) if key[e] == k_)
    # entry -> base point: GLV's second half is phi(P_i), the wide table's window w is [2^offset(w)] P_i
    pts = [R.mul(R.G, 3 + i) for i in range(4)]
    assert M.entry_base(pts, 5, M.glv8(), 4) == M.phi(pts[1])
    assert M.entry_base(pts, 4 * 7 + 2, M.wide13(), 4) == R.mul(pts[2], 1 << M.wide_offset(7)) and M.wide_offset(7) == 139
    assert M.bucket_sum(pts, [(0, 0), (1, 1), (3, 0)], M.equal16(), 4) == R.add(R.add(pts[0], R.neg(pts[1])), pts[3])
    assert M.key_max_word(np.array([5, 9], dtype=np.uint16), 0, True) == 9 | M.KEY_TRACKED | M.KEY_UNSIGNED


# ---- Edwards-BLS12: the model of tests/test_ed_stages_gpu.py and the vectors of tests/ed_curve_points.py ----
import ed_curve_points as V  # noqa: E402
from check_vectors import ed_low_order_points  # noqa: E402


def ed_weighted_sum(points, ks, g):
    """sum over slots of 2^offset sum over keys of key * bucket_sum: what the reduction and the host tail make of the buckets."""
    n = len(ks)
    cols, flags = M.digit_matrix(ks, g)
    assert flags == 0
    total = R.ED_ID
    for slot, s in enumerate(g.slots):
        c = M.csr(cols[slot], g.bucket_log, s.bias, s.key_unsigned)
        acc = R.ED_ID
        for key in np.nonzero(c.counts)[0]:
            if key:
                acc = R.ed_add(acc, R.ed_mul(M.bucket_sum(points, c.row(int(key)), g, n, ed=True), int(key)))
        total = R.ed_add(total, R.ed_mul(acc, 1 << s.offset))
    return total


@pytest.mark.parametrize("name", ["even16", "equal16"])
def test_ed_model_buckets_add_up_to_the_naive_msm(name):
    """48 points with every low-order class among them: the weighted sum of the model's bucket sums is pyref.ed_msm_naive."""
    points, ks, planted, expected = V.every_curve_point(48, 7)
    low = [R.ED_ID] + ed_low_order_points()
    assert all(t in points for t in low) and any(R.ed_mul(pt, R.ED_SUBGROUP) not in low[:1] + [pt] and pt not in low for pt in points)  # P + T too
    assert R.ed_msm_naive(points, ks) == expected
    assert ed_weighted_sum(points, ks, FULL[name]) == expected
    assert M.bucket_sum(points, [], FULL[name], 48, ed=True) == R.ED_ID
    assert M.bucket_sum(points, [(3, 0), (3, 1)], FULL[name], 48, ed=True) == R.ED_ID and M.entry_base(points, 5, FULL[name], 48, ed=True) == points[5]


def test_ed_oracle_and_closed_form_agree_with_pyref_on_low_order_inputs():
    """The C oracle (its windowed MSM and its naive one) and the closed form over the progression equal pyref.ed_msm_naive
    on the vectors the GPU tests feed: every curve point, low-order points alone, a total that is the identity; and the
    oracle's point generator is the progression the closed form assumes."""
    oracle = util.load_oracle()
    cases = []
    for n in (1, 2, 63, 65):
        points, ks, _, expected = V.every_curve_point(n, 1)
        cases.append((points, ks, expected))
    points, ks = V.only_low_order(64, 1)
    cases.append((points, ks, None))
    points, ks = V.total_is_identity(64, 1)
    cases.append((points, ks, R.ED_ID))
    for points, ks, expected in cases:
        exp = R.ed_msm_naive(points, ks)
        assert expected is None or exp == expected
        pts_b, ks_b = R.ed_encode_points(points), R.encode_scalars(ks)
        assert util.oracle_ed_msm(oracle, pts_b, ks_b) == R.ed_encode_result(exp)
        assert util.oracle_ed_msm(oracle, pts_b, ks_b, fn="oracle_ed_msm_naive") == R.ed_encode_result(exp)
    # the larger vectors of the GPU tests: the closed form against the oracle (pinned to pyref just above)
    for n in (257, 600, 1000):
        points, ks, _, expected = V.every_curve_point(n, 1)
        assert util.oracle_ed_msm(oracle, R.ed_encode_points(points), R.encode_scalars(ks)) == R.ed_encode_result(expected), n
    a0, d = 0xED57A6E5, 0xD15717C7
    assert util.oracle_ed_gen_points(oracle, 40, a0, d) == R.ed_encode_points(V.subgroup_points(40, a0, d))
    ks = V.uniform_scalars(40, 0)
    assert V.progression_msm(a0, d, ks) == R.ed_msm_naive(V.subgroup_points(40, a0, d), ks)


def test_ed_record_decode():
    """ed_record_affine: 9-limb coordinates in Montgomery form with radix 2^261, lazy residues (zero as 0 or as q, values up
    to q + e), any projective factor."""
    fq = M.fq_model()
    assert (fq.N, fq.P, fq.R) == (9, R.Q, 1 << 261)
    rnd = random.Random(0xEDDEC)
    t2, t4a, _ = ed_low_order_points()

    def record(pt, z, lift):
        x, y = pt
        vals = [x * z % R.Q, y * z % R.Q, x * y * z % R.Q, z % R.Q]
        words = []
        for v, up in zip(vals, lift):
            m = v * fq.R % R.Q
            if up and m + R.Q < fq.shapes["stored"].hi:  # the same residue one modulus higher where q + e admits it: zero as q
                m += R.Q
            words += [(m >> (29 * j)) & ((1 << 29) - 1) for j in range(8)] + [m >> 232]
        return np.array(words, dtype=np.uint32)

    assert R.Q < fq.shapes["stored"].hi
    for pt in [R.ED_ID, t2, t4a, R.ED_G, R.ed_add(R.ED_G, t4a), R.ed_mul(R.ED_G, 12345)]:
        for lift in ((0, 0, 0, 0), (1, 0, 1, 0), (1, 1, 1, 1)):
            assert M.ed_record_affine(record(pt, rnd.randrange(1, R.Q), lift)) == pt
    bad = record(R.ED_G, 5, (0, 0, 0, 0))
    bad[9] ^= 1
    with pytest.raises(AssertionError):
        M.ed_record_affine(bad)


def test_ed_stage_cases_meet_the_decode_floors():
    """What tests/test_ed_stages_gpu.py asserts again before it touches the GPU, here without one: every slot of its
    5000-point cases that is not listed as small offers 300 non-empty buckets and 50 rows of two and more entries (about
    340 such rows are expected among 5000 uniform entries over 2^15 keys), and its case scalars fit their geometry."""
    cases = [(M.even16(), V.uniform_scalars(5000, 1)), (M.even16(), V.uniform_scalars(5000, 2)), (M.equal16(), R.rand_scalars(0xED3E12, 5000))]
    for g, ks in cases:
        cols, flags = M.digit_matrix(ks, g)
        assert flags == 0
        for slot in (0, 8, 12, 15):
            lens = M.csr(cols[slot], 15, g.slots[slot].bias).counts[1:]
            assert int((lens > 0).sum()) >= 300 and int((lens >= 2).sum()) >= 50, (g.name, slot)
    for ks in (V.few_distinct_scalars(3000, 5, 8), V.one_long_row_scalars(1100, 600, 10), V.every_curve_point(600, 1)[1]):
        assert M.digit_matrix(ks, M.even16())[1] == 0
    assert len([k for k in V.even_edge_scalars() if M.recode(k, M.even16()).flags == 0]) == 13  # the others rerun


# ---- the window records: stage_model.partial_points, the record decode, and the inputs of tests/test_partial_records_gpu.py ----
import ctypes

import partial_cases as C
from test_field29_host import shim  # noqa: F401  (the fixture: the product's host tail behind ctypes)

# (name, geometry, Edwards-BLS12, folded table): every way a call lays out its records
RECORD_GEOMETRIES = [
    ("even16", M.even16(), False, False), ("equal16", M.equal16(), False, False), ("narrow22", M.narrow22(), False, False),
    ("short 64/15", M.short(64, 15), False, False), ("short 64/11", M.short(64, 11), False, False), ("short 200/15", M.short(200, 15), False, False),
    ("wide13", M.wide13(), False, False), ("glv8", M.glv8(), False, False), ("table16", M.equal16(), False, True),
    ("ed even16", M.even16(), True, False), ("ed equal16", M.equal16(), True, False),
]
RECORD_IDS = [x[0] for x in RECORD_GEOMETRIES]


def naive(points, scalars, ed):
    return R.ed_msm_naive(points, scalars) if ed else R.msm_naive(points, scalars)


def small_inputs(g, ed, seed):
    """A dozen points -- random ones, one twice, one with its negative, low-order ones on Edwards-BLS12 -- under random
    scalars and the geometry's edge scalars that fit it."""
    rnd = random.Random("record model/%s/%s" % (g.name, seed))
    _, neg, mul, _, gen, order = M.group(ed)
    logs = [rnd.randrange(1, order) for _ in range(8)]
    logs += [logs[0], order - logs[1]]
    points = [mul(gen, a) for a in logs]
    if ed:
        from check_vectors import ed_low_order_points

        low = ed_low_order_points()
        points += low
        logs += [None] * len(low)
    top = g.bits if g.name == "short" else 253
    pool = [k for k in planted(g, top) if M.recode(k, g).flags == 0 and k < order]
    ks = [rnd.choice(pool) if i % 3 == 0 else rnd.randrange(min(order, 1 << top)) for i in range(len(points))]
    ks = [k if M.recode(k, g).flags == 0 else 1 for k in ks]
    return points, logs, ks


@pytest.mark.parametrize("name,g,ed,fold", RECORD_GEOMETRIES, ids=RECORD_IDS)
def test_partial_points_weigh_up_to_the_naive_msm(name, g, ed, fold):
    """(a) sum_records 2^offset (total + sum_b 2^b plane_b) = msm_naive, with the logarithms and with the group law alone;
    both give the same points."""
    for seed in range(1 if ed else 2):  # (pyref.ed_mul takes 20 ms)
        points, logs, ks = small_inputs(g, ed, seed)
        n = len(ks)
        cols, flags = M.digit_matrix(ks, g)
        assert flags == 0
        by_law = M.partial_points(points, cols, g, n, ed=ed, fold=fold)
        by_log = M.partial_points(points, cols, g, n, logs=logs, ed=ed, fold=fold)
        assert by_law == by_log, name
        assert len(by_law) == (1 if fold or g.name == "wide13" else len(g.slots)) and all(len(rec) == g.bucket_log + 1 for rec in by_law)
        assert M.weighted_sum(by_law, g, ed=ed, fold=fold) == naive(points, ks, ed), name


def tail_args(g, ed, fold, form):
    """(windows, cbits, planes, short_from, shim form) the product calls its host tail with at this geometry."""
    L = g.bucket_log
    records = 1 if fold or g.name == "wide13" else len(g.slots)
    short_from = {"even16": 13, "narrow22": 11}.get(g.name, 0)
    return records, L + 1, L, short_from, {M.FORM_TE: 0, M.FORM_XYZZ: 1, M.FORM_ED: 2}[form]


def through_the_host_tail(shim, model, g, ed, fold, form, rnd):
    words = M.encode_records(model, form, 20 if g.name == "wide13" else 16, z=lambda: rnd.randrange(1, R.Q if ed else R.P))
    arr = (ctypes.c_uint32 * len(words))(*[int(x) for x in words])
    out = ctypes.create_string_buffer(64 if ed else 96)
    assert shim.shim_tail_combine_geom(arr, *tail_args(g, ed, fold, form), out) == 0
    return out.raw


@pytest.mark.parametrize("name,g,ed,fold", RECORD_GEOMETRIES, ids=RECORD_IDS)
def test_partial_points_through_the_products_host_tail(shim, name, g, ed, fold):
    """(b) The model's points, encoded as records under random projective factors with 0xFFFFFFFF words beyond `planes`, give
    the call's 96 (64) bytes through teh_combine / g1h_combine / edh_combine at the geometry the product passes.  The
    Weierstrass tail takes 16-bit windows only: equal16 and glv8."""
    rnd = random.Random("tail/" + name)
    points, logs, ks = small_inputs(g, ed, 7)
    cols, _ = M.digit_matrix(ks, g)
    model = M.partial_points(points, cols, g, len(ks), logs=logs, ed=ed, fold=fold)
    exp = R.ed_encode_result(naive(points, ks, ed)) if ed else R.encode_result(naive(points, ks, ed))
    forms = [M.FORM_ED] if ed else [M.FORM_XYZZ] if g.name == "glv8" else [M.FORM_TE, M.FORM_XYZZ] if name == "equal16" else [M.FORM_TE]
    for form in forms:
        assert through_the_host_tail(shim, model, g, ed, fold, form, rnd) == exp, (name, form)


def test_record_point_decode_and_contract():
    """record_point_affine inverts the encoders in each form and refuses what the contract forbids: a coordinate at or
    above the modulus, a tag in the wrong place or missing, a broken invariant; is_stored_identity tells the identity as
    stored from a point that merely decodes to it."""
    rnd = random.Random("record decode")
    p = R.mul(R.G, 0xDEC0DE)
    e = R.ed_mul(R.ED_G, 0xDEC0DE)
    for form, pt, ident in ((M.FORM_TE, p, None), (M.FORM_XYZZ, p, None), (M.FORM_ED, e, R.ED_ID)):
        cw, mod = (8, R.Q) if form == M.FORM_ED else (12, R.P)
        for first in (True, False):
            for value in (pt, ident):
                words = list(M.encode_records([[value] if first else [ident, value]], form, 2, z=lambda: rnd.randrange(2, mod))[(0 if first else 4 * cw) : (4 * cw if first else 8 * cw)])
                assert M.record_point_affine(words, form, first_point=first) == value
                assert M.is_stored_identity(words, form) == (value == ident)
                bad = list(words)  # + modulus on coordinate 1: the same point, not canonical
                v = sum(int(x) << (32 * i) for i, x in enumerate(bad[cw : 2 * cw])) + mod
                bad[cw : 2 * cw] = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(cw)]
                with pytest.raises(AssertionError, match="not canonical"):
                    M.record_point_affine(bad, form, first_point=first)
                bad = list(words)  # the tag where it must not be / missing where it must be
                bad[cw - 1] ^= M.RECORD_TAG
                with pytest.raises(AssertionError, match="tag"):
                    M.record_point_affine(bad, form, first_point=first)
                bad = list(words)  # the tag bit on another coordinate: at or above the modulus
                bad[3 * cw - 1] |= M.RECORD_TAG
                with pytest.raises(AssertionError, match="not canonical"):
                    M.record_point_affine(bad, form, first_point=first)
                if value != ident:
                    bad = list(words)
                    bad[2 * cw] ^= 1  # T / ZZ off by one
                    with pytest.raises(AssertionError, match="invariant"):
                        M.record_point_affine(bad, form, first_point=first)


def test_meetings_of_the_reduction_tree_against_a_replay_of_all_buckets():
    """stage_model.meetings follows two occupied buckets; here the whole array of 2^L sets is folded level by level as
    reduce.hpp defines it, for L = 6, and every pair must meet where meetings says (and end in the same record points)."""
    L = 6
    NB = 1 << L
    for x in range(NB):
        for y in range(x + 1, NB):
            B = [set() for _ in range(NB)]
            B[x], B[y] = {"x"}, {"y"}
            met = []
            for r in range(L):
                half = NB >> (r + 1)
                for arr in range(r + 1):
                    lo = 0 if arr == 0 else NB >> arr
                    for k in range(half):
                        a, b = B[lo + k], B[lo + k + half]
                        if len(a) == 1 and len(b) == 1 and a != b:
                            met.append((r, arr))
                        B[lo + k] = a | b
            assert met == M.meetings(x, y, L), (x, y)
            assert B[0] == {"x", "y"}
            for b in range(L):
                assert B[1 << b] == ({"x"} if (x >> b) & 1 else set()) | ({"y"} if (y >> b) & 1 else set()), (x, y, b)


LADDER_GEOMETRIES = [x for x in RECORD_GEOMETRIES if x[0] in ("even16", "equal16", "narrow22", "glv8", "ed even16", "wide13", "table16")]


def occupied_by_the_model(case):
    """record -> bucket indices that hold entries, from the model's digit matrix alone."""
    cols, flags = M.digit_matrix(case.scalars, case.g)
    assert flags == 0
    out = {}
    for rec, slots in enumerate(M.record_slots(case.g, case.fold)):
        for slot in slots:
            s = case.g.slots[-1] if case.g.name == "wide13" else case.g.slots[slot]
            key, _ = M.keys_and_signs(cols[slot], s.bias, s.key_unsigned)
            for k in key[key > 0]:
                out.setdefault(rec, set()).add(int(k) - 1)
    return out


def check_preconditions(case):
    """(c) What a case promises, from the model alone: which buckets are occupied, where its pair meets, which planes are
    empty -- and that its records weigh up to its expected result."""
    L = case.g.bucket_log
    assert occupied_by_the_model(case) == {r: s for r, s in case.occupied.items() if s}, case.name
    for rec, where in case.meet.items():
        x, y = sorted(case.occupied[rec])
        assert M.meetings(x, y, L) == where, (case.name, rec)
    model = C.model_records(case)
    ident = R.ED_ID if case.ed else None
    for rec, points in enumerate(model):
        held = case.occupied.get(rec, set())
        for b in range(L):
            if not any((t >> b) & 1 for t in held):
                assert points[1 + b] == ident, (case.name, rec, b, "a plane no occupied bucket feeds")
        if not held:
            assert points[0] == ident
    got = M.weighted_sum(model, case.g, ed=case.ed, fold=case.fold)
    assert (R.ed_encode_result(got) if case.ed else R.encode_result(got)) == C.expected_result(case), case.name
    return model


@pytest.mark.parametrize("name,g,ed,fold", RECORD_GEOMETRIES, ids=RECORD_IDS)
def test_planted_planes_hold_what_they_promise(name, g, ed, fold):
    """One point alone in bucket 2^b: plane b and the total ARE that point, every other plane is the identity.  Coverage:
    every plane of the geometry in some window; every window of a full-width geometry used."""
    ident = R.ED_ID if ed else None
    seen_planes = set()
    uses = [range(8), range(8, 16)] if g.name == "glv8" else [None]
    for use in uses:
        for case in C.planted(g, ed=ed, fold=fold, use=use):
            model = check_preconditions(case)
            for rec, held in case.occupied.items():
                if len(held) != 1:
                    continue
                (t,) = held
                b = t.bit_length() - 1
                assert t == 1 << b
                pts = [pt for pt, k in zip(case.points, case.scalars) if k]  # (single-record cases: one scalar)
                assert model[rec][0] == model[rec][1 + b] != ident
                assert all(model[rec][1 + c] == ident for c in range(g.bucket_log) if c != b)
                assert model[rec][0] in pts or fold or g.name in ("wide13", "glv8")  # (a table window / phi(P) carries a factor)
                seen_planes.add(b)
    if g.name != "short":
        assert seen_planes == set(range(g.bucket_log)), (name, seen_planes)
    for case in C.extras(g, ed=ed, fold=fold):
        model = check_preconditions(case)
        if case.name in ("extras", "P and -P"):
            rec = 0 if (fold or g.name == "wide13") else 3
            assert model[rec][0] == ident and model[rec][1 + g.bucket_log - 1] != ident and model[rec][1] != ident, name
        if case.name == "extras":
            assert all(pt == ident for pt in model[2]) and all(pt != ident for pt in model[0]), name  # an empty window; index 2^L - 1: every plane set


@pytest.mark.parametrize("name,g,ed,fold", LADDER_GEOMETRIES, ids=[x[0] for x in LADDER_GEOMETRIES])
def test_the_ladder_meets_where_it_promises(name, g, ed, fold):
    """Indices 0 and 2^L >> (r + 1) first meet at level r in the running block; lo + k and lo + k + half meet at level r in
    the block and in the list of level r - age.  A doubling doubles, a cancellation leaves total O and plane -P."""
    ident = R.ED_ID if ed else None
    single = fold or g.name == "wide13"
    kinds = C.SECOND + (("order2", "order4") if ed else ())
    for kind in kinds:
        for age in (0, 1, 2, 3) if kind in C.SECOND else (0,):  # the ages the GPU cases run
            levels = [lv for lv in range(g.bucket_log) if lv >= age]
            todo, done_all = ([levels[0]], [levels[-1]]) if single else (levels,), []
            for lv_list in todo:
                use = range(8, 16) if g.name == "glv8" and age % 2 else None
                left = list(lv_list)
                while left:
                    case = C.ladder(g, kind, ed=ed, age=age, use=use, levels=left, fold=fold)
                    model = check_preconditions(case)
                    done = C.levels_in(case)
                    done_all += done
                    left = [lv for lv in left if lv not in done]
                    for rec, where in case.meet.items():
                        assert where[0][1] == 0 and (len(where) == 1) == (age == 0)
                        if kind == "negative":
                            assert model[rec][0] == ident and sum(pt != ident for pt in model[rec][1:]) >= 1
                        if kind == "same" and age == 0 and not single and g.name != "glv8":
                            assert model[rec][0] == M.group(ed)[0](case.points[0], case.points[0])
            if not single:
                assert sorted(done_all) == levels, (name, kind, age)


# ---- the accumulation work list: row_split of the product against the model, the model on hand-worked rows ----
import os  # noqa: E402
import subprocess  # noqa: E402

import work_list_cases as W  # noqa: E402

ROW_SPLIT_SRC = os.path.join(util.ROOT, "tests", "native", "row_split_shim.cpp")
ROW_SPLIT_SO = os.path.join(util.ROOT, "tests", "native", "_build", "librow_split_shim.so")


@pytest.fixture(scope="module")
def row_split_shim():
    csrc = os.path.join(util.ROOT, "webgpu-msm-bls12-377_amd", "csrc")
    deps = [ROW_SPLIT_SRC, os.path.join(csrc, "row_split.hpp")]
    if not os.path.exists(ROW_SPLIT_SO) or any(os.path.getmtime(d) > os.path.getmtime(ROW_SPLIT_SO) for d in deps):
        os.makedirs(os.path.dirname(ROW_SPLIT_SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", csrc, "-o", ROW_SPLIT_SO, ROW_SPLIT_SRC])
    return ctypes.CDLL(ROW_SPLIT_SO)


def test_row_split_of_the_product_is_the_models_and_keeps_its_contract(row_split_shim):
    """csrc/row_split.hpp (the function every accumulation kernel cuts its rows with, compiled for the host) against
    stage_model.row_split for every SEG in 8..128 and every length in 0..34 SEG + 8, and the contract of a split."""
    for seg in range(8, 129):
        count = 34 * seg + 9
        out = (ctypes.c_uint32 * (3 * count))()
        row_split_shim.row_split_table(ctypes.c_uint32(seg), ctypes.c_uint32(0), ctypes.c_uint32(count), out)
        got = np.frombuffer(out, dtype=np.uint32).reshape(count, 3)
        for length in range(count):
            nseg, seglen, lastlen = (int(x) for x in got[length])
            assert (nseg, seglen, lastlen) == tuple(M.row_split(length, seg)), (seg, length)
            if length == 0:
                assert (nseg, seglen, lastlen) == (1, 0, 0)
                continue
            assert seglen <= seg and 1 <= lastlen <= seglen, (seg, length)
            assert (nseg - 1) * seglen + lastlen == length, (seg, length)
            assert nseg <= -(-length // seg), (seg, length)
            assert (nseg == 1) == (length <= seg), (seg, length)


def test_work_list_model_on_hand_worked_rows():
    """Rows of 0, 1, SEG, SEG + 1, 2 SEG + 1, 32 SEG and 32 SEG + 1 entries at SEG = 24, worked by hand."""
    seg = 24
    assert M.row_split(0, seg) == (1, 0, 0) and M.row_split(1, seg) == (1, 1, 1) and M.row_split(24, seg) == (1, 24, 24)
    assert M.row_split(25, seg) == (2, 13, 12)      # two parts: 13 + 12
    assert M.row_split(49, seg) == (3, 17, 15)      # three parts: 17 + 17 + 15
    assert M.row_split(768, seg) == (32, 24, 24)    # 32 full parts
    assert M.row_split(769, seg) == (33, 24, 1)     # 33 parts of ceil(769 / 33) = 24: 32 x 24 + 1
    assert M.item_range(49, seg, 2) == (34, 49) and M.item_range(769, seg, 32) == (768, 769)
    lens = [0, 1, 24, 25, 49, 768, 769]
    # two slots of 2^3 rows; the same lengths in both, the second slot is the fold slot
    L = 3
    rows = lens + [0] + lens + [0]
    wl = M.work_list(rows, seg, fold_slot=1, bucket_log=L)
    hist = [0] * M.SEG_BINS
    for b, c in ((0, 2), (1, 1 + 1), (24, 1 + 32 + 32), (13, 1), (12, 1), (17, 2), (15, 1)):
        hist[b] += 2 * c
    assert wl.hist == hist
    assert wl.items == 2 * (2 + 1 + 1 + 2 + 3 + 32 + 33) == sum(hist)
    assert wl.split_rows == [3, 4, 5, 6, 11, 12, 13, 14]
    assert wl.overflow_slots == 2 * (1 + 2 + 31 + 32)
    assert wl.folded == [14]  # 33 items: more than 32, in the fold slot; the 32-item row 13 is not, nor is row 6 of slot 0
    assert M.work_list(rows, seg, bucket_log=L).folded == []
    assert wl.item_set.shape == (wl.items, 3)
    as_set = {tuple(int(x) for x in it) for it in wl.item_set}
    assert len(as_set) == wl.items
    assert {(0, 0, 0), (1, 0, 1), (3, 0, 13), (3, 1, 12), (4, 2, 15), (6, 32, 1), (14, 31, 24), (15, 0, 0)} <= as_set
    assert (6, 33, 1) not in as_set and (5, 32, 0) not in as_set


@pytest.mark.parametrize("S", [16, 24, 64, 120, 128])
def test_work_list_cases_hold_what_they_promise(S):
    """The skewed inputs of tests/test_work_list_gpu.py in every geometry they are run in: every slot holds rows of exactly
    the case's lengths, among them rows of 32 and of 33 work items; three histogram bins above 16 are occupied."""
    geoms = [M.even16()] if S not in (24, 64) else [M.even16(), M.equal16(), M.short(72, 15)] + ([M.glv8(), M.wide13(), M.narrow22()] if S == 64 else [])
    for g in geoms + ([M.equal16()] if S == 128 else []):
        case = W.skewed(g, S, bound=(1 << 72) if g.name == "short" else R.R_ORDER)
        assert len(case.scalars) == len(case.other) == 138 * S + 8 and sorted(case.scalars) != sorted(case.other)
        cols, flags = M.digit_matrix(case.scalars, g)
        assert flags == 0 and M.digit_matrix(case.other, g)[1] == 0
        lens = W.row_lengths(g, cols)
        slots = 1 if g.name == "wide13" else len(g.slots)
        assert len(lens) == slots << g.bucket_log
        wl = M.work_list(lens, S, fold_slot=slots - 1 if g.name == "short" else -1, bucket_log=g.bucket_log)
        W.check_promises(case, lens, wl, range(slots))
        per = {"glv8": 2, "wide13": 13}.get(g.name, 1)
        assert len(wl.split_rows) == 8 * per * slots  # the rows longer than S: eight of the eleven lengths
        if g.name == "short":
            assert len(wl.folded) == 2  # 32 S + 1 and 33 S + 5 in the top slot: 33 and 34 items; 31 S + 1 and 32 S (32 items) stay


# ---- the GLV front end: csrc/glv_split.hpp (the arithmetic of k_decompose_glv, compiled for the host) against the model ----
import glv_cases as GC  # noqa: E402

GLV_SPLIT_SRC = os.path.join(util.ROOT, "tests", "native", "glv_split_shim.cpp")
GLV_SPLIT_SO = os.path.join(util.ROOT, "tests", "native", "_build", "libglv_split_shim.so")


@pytest.fixture(scope="module")
def glv_split_shim():
    csrc = os.path.join(util.ROOT, "webgpu-msm-bls12-377_amd", "csrc")
    deps = [GLV_SPLIT_SRC, os.path.join(csrc, "glv_split.hpp"), os.path.join(csrc, "consts_gen.hpp")]
    if not os.path.exists(GLV_SPLIT_SO) or any(os.path.getmtime(d) > os.path.getmtime(GLV_SPLIT_SO) for d in deps):
        os.makedirs(os.path.dirname(GLV_SPLIT_SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", csrc, "-o", GLV_SPLIT_SO, GLV_SPLIT_SRC])
    return ctypes.CDLL(GLV_SPLIT_SO)


def glv_split_table(lib, ks):
    """(rem0, k1, k2, digits, bad, corrected) per scalar, as the product's arithmetic computes them."""
    n = len(ks)
    words = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint32)
    rem0, k1, k2 = (np.zeros(5 * n, dtype=np.uint32) for _ in range(3))
    digits, bad, corrected = np.zeros(16 * n, dtype=np.uint16), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    lib.glv_split_table(ptr(words), ctypes.c_uint64(n), ptr(rem0), ptr(k1), ptr(k2), ptr(digits), ptr(bad), ptr(corrected))
    def ints(a):
        raw = a.tobytes()
        return [int.from_bytes(raw[20 * i : 20 * i + 20], "little") for i in range(n)]

    return ints(rem0), ints(k1), ints(k2), digits.reshape(n, 16).tolist(), bad.tolist(), corrected.tolist()


def test_glv_split_of_the_product_is_divmod_and_the_models_digits(glv_split_shim):
    """csrc/glv_split.hpp -- Barrett quotient, its one correction, the digit chains of both halves -- against Python's
    divmod and stage_model.recode(k, glv8()): k1, k2, the sixteen stored digits, the range flag, and WHETHER THE CORRECTION
    WAS TAKEN: for every k = m lambda with m >= 1 and for no other input (so the test cannot pass without reaching the
    arm); the remainder before it is below 2 lambda, as the kernel's comment says.  Inputs: m lambda + t, t in -2 .. 2,
    for the factors of glv_cases.lambda_factors (10^5 random ones); 10^6 random k below 2^256 and 10^5 below r; every
    boundary word in every window of k2 and of k1; the edge of the range."""
    lam, g = GC.LAM, M.glv8()
    rnd = GC.rng("host")
    groups = {
        "multiples": GC.around_multiples(GC.lambda_factors(rnd, 100000)),
        "random256": [rnd.getrandbits(256) for _ in range(1000000)],
        "random_r": [rnd.randrange(r) for _ in range(100000)],
        "boundaries": GC.boundary_halves(rnd, 25),
        "edge": [GC.EDGE - 1, GC.EDGE, GC.BEYOND, GC.BEYOND + 1, GC.EDGE_CARRIED, GC.EDGE_CARRIED + 1, (1 << 256) - 1],
    }
    taken = {}
    for name, ks in groups.items():
        rem0, k1, k2, digits, bad, corrected = glv_split_table(glv_split_shim, ks)
        flagged = 0
        for i, k in enumerate(ks):
            q, t = divmod(k, lam)
            rec = M.recode(k, g)
            assert (k1[i], k2[i]) == (t, q), (name, hex(k))
            assert digits[i] == rec.stored, (name, hex(k))
            assert bool(bad[i]) == bool(rec.flags & M.ERR_GLV_RANGE) and rec.flags & ~M.ERR_GLV_RANGE == 0, (name, hex(k))
            assert bool(corrected[i]) == (t == 0 and q >= 1), (name, hex(k), "the correction arm")
            assert rem0[i] < 2 * lam and rem0[i] == t + lam * corrected[i], (name, hex(k))
            flagged += bad[i]
        taken[name] = (sum(corrected), len(ks), flagged)
    print("correction arm taken / inputs / out of range:", taken)
    assert taken["multiples"][0] == sum(k % lam == 0 and k > 0 for k in groups["multiples"]) > 100000
    assert taken["random256"][0] == taken["random_r"][0] == 0  # no random scalar reaches it
    assert taken["edge"][0] == 2  # BEYOND = lambda (HALF_MAX + 1) and EDGE_CARRIED + 1 = lambda (HALF_MAX_CARRIED + 1)
    assert taken["boundaries"][2] > 0 and taken["random_r"][2] == 0 and taken["random256"][2] > 0
    # the edge of the range, from the model: EDGE is the largest scalar without the flag
    assert M.recode(GC.EDGE, g).flags == 0 and M.recode(GC.EDGE_CARRIED, g).flags == 0 and M.recode(GC.BEYOND, g).flags == M.ERR_GLV_RANGE
    assert M.recode(GC.EDGE, g).digits == M.recode(lam - 1, g).digits[:8] + [0x7FFF] * 8
    assert M.recode(GC.EDGE_CARRIED, g).digits[8:] == [-1] + [0] * 6 + [0x7FFF]  # top limb 0x7FFE + the carry
    assert all(M.recode(GC.EDGE + 1 + lam * j, g).flags for j in range(0, 70000, 7))  # (no gap right above it)
