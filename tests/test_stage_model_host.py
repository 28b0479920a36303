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
