"""Stage read-backs on the window geometries production runs (capture mode 2, msm377_g1_read_stage_ex): digits, CSR rows
and bucket records of the route a call takes by itself -- even 13 + 3, narrow 11 + 11, short scalars, the wide table, the
GLV front end, reruns -- against tests/stage_model.py (pinned by tests/test_stage_model_host.py).  tests/STAGES.md maps
kernels to these tests and lists the seeded faults they were shown to catch.

Every case runs one MSM of the same size with OTHER scalars first, on the same context: a row_ptr word the kernels fail
to write then holds that call's value, not a plausible one.  Each slot read is checked whole (every digit, every row_ptr
word, every val_idx entry, the empty / non-empty state and the coordinate box of every bucket); the big-integer decode
covers the rows with two and more entries first, up to DECODE_CAP buckets per slot."""
import random

import numpy as np
import pytest

import lazy_model
import pyref as R
import stage_model as M
import util
import webgpu_msm_bls12_377_amd as msm
from test_g1_parity_gpu import dev
from webgpu_msm_bls12_377_amd.host.engine import ESTATE

pytestmark = pytest.mark.gpu

DECODE_CAP = 300  # buckets per slot decoded with Python integers
MIN_NONEMPTY, MIN_MULTI = 300, 50  # what a slot must offer for that cap to be a cap and not the whole check
FORM_XYZZ, FORM_TE, FORM_ED = 0, 1, 2  # MSM377_STAGE_FORM_*: G1 in XYZZ, G1 in twisted Edwards form, the Edwards-BLS12 curve
FP = lazy_model.FieldModel("Fp")
STORED, STORED_X = FP.shapes["stored"], FP.shapes["stored_x"]  # the boxes tools/check_lazy_bounds.py starts from
STORED_FQ = M.fq_model().shapes["stored"]  # ... under use_field("Fq"): every coordinate of an Edwards-BLS12 record, below q + e
LIMBS = {FORM_XYZZ: 13, FORM_TE: 13, FORM_ED: 9}  # per coordinate of a record as read back


def coordinate_shapes(form):
    """Stored-record contract per coordinate: every Edwards coordinate and Y, ZZ, ZZZ of XYZZ below p + e, X of XYZZ below
    5p + e; every coordinate of an Edwards-BLS12 record below q + e in the 9-limb box."""
    if form == FORM_ED:
        return (STORED_FQ,) * 4
    return (STORED_X if form == FORM_XYZZ else STORED, STORED, STORED, STORED)


def identity_mask(bk, form):
    """Records that ARE the stored identity: XYZZ with ZZ = 0; Edwards (0 : c : 0 : c), on either curve."""
    nl = LIMBS[form]
    if form == FORM_XYZZ:
        return ~bk[:, 2 * nl : 3 * nl].any(axis=1)
    return ~bk[:, 0:nl].any(axis=1) & ~bk[:, 2 * nl : 3 * nl].any(axis=1) & (bk[:, nl : 2 * nl] == bk[:, 3 * nl : 4 * nl]).all(axis=1)


def decode(words, form):
    if form == FORM_ED:
        return M.ed_record_affine(words)
    return util.affine_from_xyzz_words(words) if form == FORM_XYZZ else util.affine_from_te_ext_words(words)


def model_identity(form):
    """What stage_model.bucket_sum returns for a row that adds up to nothing: None on G1, the point (0, 1) on Edwards-BLS12
    (a record that decodes to it counts as the identity whichever representative of zero it stores)."""
    return R.ED_ID if form == FORM_ED else None


def wire_points(points_wire, form):
    return [(int.from_bytes(points_wire[64 * i : 64 * i + 32], "little"), int.from_bytes(points_wire[64 * i + 32 : 64 * i + 64], "little"))
            for i in range(len(points_wire) // 64)] if form == FORM_ED else R.decode_points(points_wire)


def slot_of(g, slot):
    """The model's description of a slot read (the wide table's one slot: every window shares bias and sign handling)."""
    return g.slots[-1] if g.name == "wide13" else g.slots[slot]


def values_below(limbs, hi):
    """value(limbs) < hi for every row of an (m, 13) or (m, 9) limb array: carries propagated in 64-bit words, then compared with
    the limbs of hi from the top down -- lazy_model.value without a Python integer per record."""
    lb, mask, nl = lazy_model.LB, lazy_model.MASK, limbs.shape[1]
    l = limbs.astype(np.uint64)
    for j in range(nl - 1):
        l[:, j + 1] += l[:, j] >> np.uint64(lb)
        l[:, j] &= np.uint64(mask)
    h = lazy_model.nform_limbs(hi, nl)
    lt, eq = np.zeros(len(l), dtype=bool), np.ones(len(l), dtype=bool)
    for j in reversed(range(nl)):
        lt |= eq & (l[:, j] < np.uint64(h[j]))
        eq &= l[:, j] == np.uint64(h[j])
    return lt


def model_csr(g, cols, slots, small, label):
    """The model's CSR of every slot to be read, and -- on the CPU, before anything runs on the GPU -- the floors that make
    DECODE_CAP a cap: 300 non-empty buckets and 50 rows of two and more entries in every slot not listed as small."""
    out = {}
    for slot in slots:
        s = slot_of(g, slot)
        c = M.csr(cols[slot], g.bucket_log, s.bias, s.key_unsigned)
        if slot not in small:
            lens = c.counts[1:]
            assert int((lens > 0).sum()) >= MIN_NONEMPTY and int((lens >= 2).sum()) >= MIN_MULTI, (label, g.name, slot, int((lens > 0).sum()), int((lens >= 2).sum()))
        out[slot] = c
    return out


def check_slot(engine, slot, g, cols, c, points, n, form, small=False, key_max=None, label=""):
    """One window slot of the last call against the model (c: its CSR): layout, digits, the whole CSR, every bucket."""
    tag = (label, g.name, slot)
    info, st = engine.read_stage_ex(slot)
    L = g.bucket_log
    wide = g.name == "wide13"
    s = slot_of(g, slot)
    col = cols[slot]
    assert (info.slots, info.bucket_log) == (1 if wide else len(g.slots), L) == engine.last_geometry(), tag
    assert info.columns == len(col) == {"wide13": 13 * n, "glv8": 2 * n}.get(g.name, n), tag
    assert (info.digit_bytes, info.row_ptr_len, info.bucket_records, info.form) == (g.digit_bytes, (1 << L) + 2, 1 << L, form), tag
    assert info.bias[slot] == s.bias and bool(info.key_unsigned[slot]) == s.key_unsigned, tag
    assert info.table_stride == (n if wide else 0), tag
    # digits: whole columns
    assert st["digits"].dtype == col.dtype and np.array_equal(st["digits"], col), tag
    if key_max is not None:
        assert info.key_max[slot] == key_max, (tag, hex(info.key_max[slot]), hex(key_max))
    elif info.key_max[slot]:  # an untracked slot never narrows its ranges
        assert not info.key_max[slot] & M.KEY_TRACKED, tag
    # CSR: every row_ptr word, every val_idx entry
    rp, vi = st["row_ptr"].astype(np.int64), st["val_idx"]
    assert rp[0] == 0 and rp[-1] == len(col) and np.all(np.diff(rp) >= 0), tag
    assert np.array_equal(np.diff(rp), c.counts), tag
    rec = (vi & 0x7FFFFFFF).astype(np.int64)
    entry = (rec // info.table_stride) * n + rec % info.table_stride if wide else rec  # table record w * stride + i -> column w n + i
    assert np.array_equal(np.sort(entry), np.arange(len(col))), tag  # every entry once
    key, sign = M.keys_and_signs(col, s.bias, s.key_unsigned)
    row_of_position = np.repeat(np.arange((1 << L) + 1), c.counts)
    assert np.array_equal(key[entry], row_of_position), tag  # ... in the row of its key
    assert np.array_equal(sign[entry], (vi >> 31).astype(bool)), tag  # ... with its sign
    # buckets: bucket t (key t + 1) of every row
    bk = st["buckets"]
    nl, ed = LIMBS[form], form == FORM_ED
    assert bk.shape == (1 << L, 4 * nl), tag
    lens = c.counts[1:]
    ident = identity_mask(bk, form)
    assert ident[lens == 0].all(), (tag, "a bucket without entries is not the stored identity")
    for t in np.nonzero(ident & (lens > 0))[0]:  # entries that cancel (repeated points): the model must agree
        assert M.bucket_sum(points, c.row(int(t) + 1), g, n, ed=ed) == model_identity(form), (tag, int(t))
    live = ~ident
    for ci, shape in enumerate(coordinate_shapes(form)):  # the representation contract, every coordinate of every record
        limbs = bk[live][:, nl * ci : nl * ci + nl]
        assert (limbs <= np.array(shape.box, dtype=np.uint64)).all(), (tag, "coordinate %d outside its stored box" % ci)
        assert values_below(limbs, shape.hi).all(), (tag, "coordinate %d at or above its stored bound" % ci)
    multi, single = np.nonzero(live & (lens >= 2))[0], np.nonzero(live & (lens == 1))[0]
    if small:  # a slot that cannot offer 300 buckets: every non-empty bucket is decoded
        chosen = list(multi) + list(single)
    else:
        assert live.sum() >= MIN_NONEMPTY and len(multi) >= MIN_MULTI, (tag, int(live.sum()), len(multi))
        chosen = list(multi[:DECODE_CAP]) + list(single[: max(0, DECODE_CAP - len(multi))])
    cache = {}
    for t in chosen:
        words = bk[t]
        assert decode(words, form) == M.bucket_sum(points, c.row(int(t) + 1), g, n, cache, ed=ed), (tag, int(t), int(lens[t]))
    return info


def short_point(pt):
    """A point in a failure message: the identity, or the head of its x."""
    return "the identity" if pt in (None, R.ED_ID) else "x = %s..." % hex(pt[0])[:20]


TAIL_SHORT_FROM = {"even16": 13, "narrow22": 11}  # the first window that is one bit narrower (WindowPlan::short_from)


def check_records(engine, g, model, form, fold=False, label="", schedule=None):
    """The window records of the last call (msm377_g1_read_partials) against stage_model.partial_points: `info` against the
    geometry, then EVERY point of EVERY record up to `planes` -- its words against the record contract of include/msm377.h
    (canonical coordinates, the tag on coordinate 0 of point 0 of a twisted Edwards record and nowhere else), its invariant
    and its value; where the model says identity, the identity as stored.  Points beyond `planes` are not read.
    schedule: what `info` must report of the reduction schedule (a dict over coop_from, tail_from, columns, tail_lds)."""
    info, words = engine.read_partials()
    L, one = g.bucket_log, g.name == "wide13" or fold
    tag = (label, g.name)
    assert info.records == len(model) == (1 if one else len(g.slots)), (tag, info)
    assert (info.points, info.planes, info.coord_words, info.form) == (20 if g.name == "wide13" else 16, L, 8 if form == FORM_ED else 12, form), (tag, info)
    assert info.folded_slots == (len(g.slots) if fold else 1), (tag, info)
    assert info.tail_kind == {FORM_TE: 0, FORM_XYZZ: 1, FORM_ED: 2}[form], (tag, info)
    assert (info.tail_windows, info.tail_cbits, info.tail_planes, info.tail_short_from) == (info.records, L + 1, L, TAIL_SHORT_FROM.get(g.name, 0)), (tag, info)
    assert info.coop_from <= L and info.tail_from <= L and info.columns in (0, 1) and info.tail_lds in (0, 1), (tag, info)
    if info.tail_from == L:
        assert info.tail_lds == 0, (tag, "no single-launch tail ran")
    for key, want in (schedule or {}).items():
        assert getattr(info, key) == want, (tag, "schedule", key, getattr(info, key), want)
    assert words.shape == (info.records, info.points, 4, info.coord_words) and info.planes + 1 <= info.points, tag
    ident = model_identity(form)
    for w in range(info.records):
        for p in range(L + 1):
            where = (label, g.name, "record %d" % w, "the total" if p == 0 else "plane %d" % (p - 1))
            flat = words[w, p].ravel()
            try:
                got = M.record_point_affine(flat, form, first_point=p == 0)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (where, e)) from e
            assert got == model[w][p], "%s: value: the record holds %s, the model %s" % (where, short_point(got), short_point(model[w][p]))
            if model[w][p] == ident:
                assert M.is_stored_identity(flat, form), (where, "the identity is not stored as the form writes it")
    return info


def tracked_key_max(g, cols):
    """The slots whose largest key the decomposition measures, and the word it must publish: window 15 of sixteen equal
    windows; the unsigned top slot of a short call on 2^15 buckets.  Every other slot's word stays untracked."""
    top = len(g.slots) - 1
    if g.name == "equal16":
        return {15: M.key_max_word(cols[15], 1 << 15, False)}
    if g.name == "short" and g.bucket_log == 15:
        return {top: M.key_max_word(cols[top], 0, True)}
    return {}


def run_case(engine, call, g, scalars, points_wire, form, slots, other_scalars, expected, small=(), label="", reruns=0, records=None, schedule=None):
    """call(scalars) runs the MSM under test; first once with other_scalars (same size, same context).
    records: the model's window records (stage_model.partial_points) -- compared as the LAST stage, after the buckets and
    before the result (check_records; schedule: what the read-back must report of the reduction schedule)."""
    n = len(scalars)
    points = wire_points(points_wire, form)
    cols, flags = M.digit_matrix(scalars, g)
    assert flags == 0, "the case's scalars must fit the geometry it promises"
    assert len(other_scalars) == n and list(other_scalars) != list(scalars) and sorted(other_scalars) != sorted(scalars), "the call before runs other scalars"
    key_max = tracked_key_max(g, cols)
    slots, small = list(slots), set(small)
    csrs = model_csr(g, cols, slots, small, label)  # (with its floors: checked before the GPU is touched)
    engine.set_stage_capture(2)
    try:
        call(other_scalars)
        before, _ = engine.fallback_info()
        reruns_before = engine.read_stage_ex(0, want=())[0].geometry_reruns
        got = call(scalars)
        # The stages are checked BEFORE the result is: a fault that changes the result too is then reported at the stage
        # where it first shows, and one that leaves the result right has nowhere else to show.
        try:
            assert engine.fallback_info()[0] == before, (label, "a silent rerun on the Weierstrass path")
            for slot in range(len(cols)):  # every digit of EVERY slot, also of those whose rows and buckets are not read
                digits = engine.read_stage_ex(slot, want=("digits",))[1]["digits"]
                assert digits.dtype == cols[slot].dtype and np.array_equal(digits, cols[slot]), (label, g.name, slot, "digits")
            info = None
            for slot in slots:
                info = check_slot(engine, slot, g, cols, csrs[slot], points, n, form, small=slot in small, key_max=key_max.get(slot), label=label)
            assert info.geometry_reruns == reruns_before + reruns, (label, "reruns on another window geometry", info.geometry_reruns - reruns_before)
            if records is not None:
                check_records(engine, g, records, form, label=label, schedule=schedule)
        except AssertionError as e:
            raise AssertionError("%s [the call's result is %s]" % (e, "right" if got == expected else "WRONG")) from e
        assert got == expected, (label, "every stage read agrees with the model, the result does not")
    finally:
        engine.set_stage_capture(0)


def host_call(engine, pts):
    return lambda ks: engine.msm(pts, R.encode_scalars(ks))


def three(g):
    """First slot, last signed slot, last slot."""
    signed = [i for i, s in enumerate(g.slots) if s.signed]
    picked = {0, signed[-1], len(g.slots) - 1}
    return sorted(picked if len(picked) == 3 else picked | {len(g.slots) // 2})  # (all slots signed: one from the middle)


@pytest.fixture(scope="module")
def pool(oracle):
    """65536 subgroup points, shared by every case (prefixes of it)."""
    return util.oracle_gen_points(oracle, 1 << 16, 0x57A6E5, 0xD15717C7)


@pytest.fixture
def main_path(engine):
    engine.set_narrow_max(0)
    yield engine
    engine.set_narrow_max()


def fits(g, ks):
    return [k for k in ks if M.recode(k, g).flags == 0]


def edge_case(golden, g):
    """g1_n20_edge_scalars, as far as its scalars fit g without a rerun: (scalars, OTHER scalars for the call before,
    points, expected result)."""
    edge = golden["g1_n20_edge_scalars"]
    ek = fits(g, R.decode_scalars(edge["scalars"]))
    epts = edge["points"][: 96 * len(ek)]
    other = fits(g, R.rand_scalars(0xED6E, 2 * len(ek)))[: len(ek)]
    return ek, other, epts, R.encode_result(R.msm_naive(R.decode_points(epts), ek))


# ---- even geometry: 13 signed 16-bit + 3 unsigned 15-bit windows ----
@pytest.mark.parametrize("records", ["projective", "affine"])
def test_even_geometry(main_path, oracle, golden, pool, records):
    """k_decompose even mode, the two-level sort at full width, k_accumulate over projective (8 products) and affine
    (7 products, MSM377_AFFINE_MIN=1) Edwards records, k_merge_split_rows_quad."""
    g = M.even16()
    n = 5000
    pts = pool[: 96 * n]
    ks, other = R.rand_scalars(0xE7E0, n), R.rand_scalars(0xE7E1, n)
    exp = util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    ek, eother, epts, eexp = edge_case(golden, g)
    if records == "projective":
        run_case(main_path, host_call(main_path, pts), g, ks, pts, FORM_TE, three(g), other, exp, label="even")
        assert main_path.accumulate_products() == 8
        run_case(main_path, host_call(main_path, epts), g, ek, epts, FORM_TE, range(16), eother, eexp, small=range(16), label="even edge scalars")
        return
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_AFFINE_MIN", "1")
        eng = msm.MsmEngine(1 << 13)
    try:
        eng.set_narrow_max(0)
        def device_call(wire):
            d_p = dev(wire)

            def call(kk):
                d_s = dev(R.encode_scalars(kk))
                return eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(kk))

            return call

        run_case(eng, device_call(pts), g, ks, pts, FORM_TE, three(g), other, exp, label="even, affine records")
        assert eng.accumulate_products() == 7
        run_case(eng, device_call(epts), g, ek, epts, FORM_TE, range(16), eother, eexp, small=range(16), label="even edge scalars, affine records")
        assert eng.accumulate_products() == 7
    finally:
        eng.close()


def test_weierstrass_runs_sixteen_equal_windows_as_run(main_path, oracle, golden, pool):
    """The Weierstrass form keeps sixteen equal windows with a tracked top window: k_decompose plain mode with
    top_key_max, k_local_sort_lds with narrowed ranges, k_accumulate<G1Dev>; XYZZ records (X below 5p + e)."""
    g = M.equal16()
    n = 5000
    pts = pool[: 96 * n]
    ks, other = R.rand_scalars(0x3E10, n), R.rand_scalars(0x3E11, n)
    main_path.set_g1_form("weierstrass")
    try:
        run_case(main_path, host_call(main_path, pts), g, ks, pts, FORM_XYZZ, three(g), other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), label="weierstrass")
        ek, eother, epts, eexp = edge_case(golden, g)
        run_case(main_path, host_call(main_path, epts), g, ek, epts, FORM_XYZZ, range(16), eother, eexp, small=range(16), label="weierstrass edge scalars")
    finally:
        main_path.set_g1_form("edwards")


def test_equal_windows_with_a_tracked_top_window(oracle, pool):
    """MSM377_EVEN_WINDOWS=0: the Edwards form on sixteen equal windows.  Scalars below r leave window 15 thirteen bits, so
    its ranges are narrowed (win_shift 2 or 3) and the rows above the covered keys are filled by the rp_w[idx] = total
    loop of k_local_sort_lds: all 2^15 + 2 row_ptr words of that slot are compared."""
    g = M.equal16()
    n = 5000
    pts = pool[: 96 * n]
    # The call before covers MORE keys of window 15 (scalars up to 2^253 + r: win_shift 1, 16384 keys covered), so the
    # words between this call's 8192 covered keys and that call's hold real offsets of the other call unless the fill
    # writes them.
    ks, other = R.rand_scalars(0x3E12, n), [k + ((i & 1) << 253) for i, k in enumerate(R.rand_scalars(0x3E13, n))]
    cols, _ = M.digit_matrix(ks, g)
    word = M.key_max_word(cols[15], 1 << 15, False)
    top = word & 0xFFFF
    assert (1 << 12) <= top < (1 << 14), "win_shift of the top window is 2 or 3"
    assert (1 << 13) <= max(k >> 240 for k in other) < (1 << 14), "win_shift 1 in the call before"
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_EVEN_WINDOWS", "0")
        eng = msm.MsmEngine(1 << 13)
    try:
        eng.set_narrow_max(0)
        run_case(eng, host_call(eng, pts), g, ks, pts, FORM_TE, three(g), other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), label="equal windows")
    finally:
        eng.close()


def test_streamed_local_sort(main_path, oracle, pool):
    """n = 8192 scalars whose slot-0 digits all lie in one 128-key range: one sort region of 8192 elements, longer than
    LS_CACHE = 6144 -- the streamed arm of k_local_sort_lds -- and rows of ~64 entries (split rows, merge).  Slot 0 has
    at most 128 non-empty buckets by construction: all of them are decoded."""
    g = M.even16()
    n = 8192
    pts = pool[: 96 * n]
    rnd = random.Random(0x57E4)

    def scalars(seed, lo):
        return [(k & ~0xFFFF) | (lo + rnd.randrange(128)) for k in R.rand_scalars(seed, n)]

    ks, other = scalars(0x57E5, 0x2A00), scalars(0x57E6, 0x1300)
    run_case(main_path, host_call(main_path, pts), g, ks, pts, FORM_TE, three(g), other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), small=(0,),
             label="streamed sort")


# ---- narrow geometry: 11 signed 12-bit + 11 unsigned 11-bit windows ----
@pytest.mark.parametrize("n", [1, 257, 5000, 65536])
def test_narrow_geometry(engine, oracle, pool, n):
    """k_decompose_geom, k_small_sort, k_accumulate_quad (up to ~100 k work items) / k_accumulate (n = 65536), merge.
    n <= 257 cannot fill 300 buckets: every slot is read and every non-empty bucket decoded instead."""
    g = M.narrow22()
    pts = pool[: 96 * n]
    ks, other = R.rand_scalars(0x4A00 + n, n), R.rand_scalars(0x4B00 + n, n)
    tiny = n <= 257
    slots = range(22) if tiny else three(g)
    run_case(engine, host_call(engine, pts), g, ks, pts, FORM_TE, slots, other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), small=slots if tiny else (),
             label="narrow n=%d" % n)


def test_narrow_geometry_edge_scalars(engine, golden):
    g = M.narrow22()
    ek, eother, epts, eexp = edge_case(golden, g)
    run_case(engine, host_call(engine, epts), g, ek, epts, FORM_TE, range(22), eother, eexp, small=range(22), label="narrow edge scalars")


def test_narrow_geometry_long_rows(engine, oracle, pool):
    """n = 4096 over 5 distinct scalars: rows of ~800 entries -- quad work items, split rows, overflow records, merge.
    At most 5 buckets per slot are non-empty: all are decoded."""
    g = M.narrow22()
    n = 4096
    pts = pool[: 96 * n]
    rnd = random.Random(0x10F6)
    five, five2 = R.rand_scalars(0x10F7, 5), R.rand_scalars(0x10F8, 5)
    ks, other = [five[rnd.randrange(5)] for _ in range(n)], [five2[rnd.randrange(5)] for _ in range(n)]
    run_case(engine, host_call(engine, pts), g, ks, pts, FORM_TE, three(g), other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), small=range(22),
             label="narrow long rows")


# ---- short scalars ----
def short_case(engine, oracle, pool, n, sbytes, bits, L, label):
    g = M.short(bits, L)
    pts = pool[: 96 * n]
    rnd = random.Random("short/%d/%d" % (sbytes, bits))
    ks, other = ([rnd.getrandbits(bits) for _ in range(n)] for _ in range(2))
    ks[0], ks[1] = (1 << bits) - 1, 0

    def call(kk):
        return engine.msm_short(pts, b"".join(k.to_bytes(sbytes, "little") for k in kk), sbytes, bits)

    cols, _ = M.digit_matrix(ks, g)
    top = len(g.slots) - 1
    slots = sorted({0, max(top - 1, 0), top})
    # the unsigned top slot holds bits mod (L + 1) bits and the carry: at most 257 keys at every width used here
    small = [s for s in slots if not g.slots[s].signed]
    run_case(engine, call, g, ks, pts, FORM_TE, slots, other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), small=small, label=label)
    return g, cols


@pytest.mark.parametrize("sbytes,bits", [(4, 16), (8, 64), (16, 128), (32, 200)])
def test_short_scalars_main_path(main_path, oracle, pool, sbytes, bits):
    """k_decompose_short<4|8|16|32> on 2^15 buckets: the unsigned top slot (KEY_UNSIGNED, top_key_max), the UNS
    instantiations of k_range_count / k_partition_staged, k_fold_long_rows.  bits = 16, 64, 128: the top slot holds carries
    only -- rows 0 and 1 of ~n / 2 entries each, folded through the overflow slots; bucket 1 (decoded like every non-empty
    bucket of a small slot) must equal the sum of every point that carried."""
    g, cols = short_case(main_path, oracle, pool, 4096, sbytes, bits, 15, "short %d/%d" % (sbytes, bits))
    if bits % 16 == 0:
        top = cols[-1]
        assert set(np.unique(top)) == {0, 1} and 1500 < int(top.sum()) < 2600, "about half of the scalars carry into the top slot"


@pytest.mark.parametrize("sbytes,bits", [(8, 64), (4, 1)])
def test_short_scalars_narrow_path(engine, oracle, pool, sbytes, bits):
    short_case(engine, oracle, pool, 1000, sbytes, bits, 11, "short narrow %d/%d" % (sbytes, bits))


# ---- the wide table ----
def test_wide_table(engine, oracle, pool):
    """One fixed-base MSM on the 20-bit-window table: k_decompose_wide (4-byte digits), the two-pass wide sort, the
    single slot of 2^19 buckets with 13 n entries, accumulation over [2^offset(w)] P_i."""
    g = M.wide13()
    n = 3000
    pts = pool[: 96 * n]
    wide = lambda d: sum((d & 0xFFFFF) << (20 * w) for w in range(12))  # noqa: E731  (20-bit digits at their boundaries)
    ks, other = R.rand_scalars(0x71DE, n), R.rand_scalars(0x71DF, n)
    ks[:8] = [0, 1, R.R_ORDER - 1, wide(0x80000), wide(0x7FFFF), wide(0xFFFFF) % R.R_ORDER, 2, (1 << 252) + 5]
    engine.set_precompute_window(20)
    try:
        engine.set_bases_precomputed(pts)
        run_case(engine, lambda kk: engine.msm_fixed_base(R.encode_scalars(kk)), g, ks, pts, FORM_TE, [0], other,
                 util.oracle_msm(oracle, pts, R.encode_scalars(ks)), label="wide table")
        assert engine.accumulate_products() == 7
    finally:
        engine.set_precompute_window(16)
        engine.msm(pts[:96], R.encode_scalars([1]))  # drops the resident table


# ---- the GLV front end ----
def test_glv_front_end(engine, oracle, pool):
    """k_decompose_glv: 8 slots of 2 n columns, buckets over P_i and phi(P_i) = (beta x, y)."""
    g = M.glv8()
    n = 3000
    pts = pool[: 96 * n]
    ks, other = R.rand_scalars(0x61F0, n), R.rand_scalars(0x61F1, n)
    ks[:3] = [0, 1, R.R_ORDER - 1]
    engine.set_g1_form("weierstrass")
    engine.set_glv(True)
    try:
        run_case(engine, host_call(engine, pts), g, ks, pts, FORM_XYZZ, [0, 6, 7], other, util.oracle_msm(oracle, pts, R.encode_scalars(ks)), label="glv")
    finally:
        engine.set_glv("auto")
        engine.set_g1_form("edwards")


# ---- scalars that must rerun ----
@pytest.mark.parametrize("route", ["even", "narrow"])
def test_scalars_that_do_not_fit_rerun_on_equal_windows(engine, oracle, pool, route):
    """One scalar of 2^253 - 2^238 and more among 500: the pass on the even / narrow geometry is discarded, the call
    reruns on sixteen equal windows, and the read-back describes THAT pass -- the one case where a rerun is expected,
    exactly one."""
    n = 500
    pts = pool[: 96 * n]
    ks, other = R.rand_scalars(0x2E2A, n), R.rand_scalars(0x2E2B, n)
    big = (1 << 253) - (1 << 238) + (1 << 237) + 12345
    first = M.even16() if route == "even" else M.narrow22()
    assert all(M.recode(k, first).flags == 0 for k in ks)
    ks[77] = (1 << 253) + 99  # from 2^253 on nothing fits either geometry
    other[5] = big
    assert M.recode(ks[77], first).flags == M.ERR_RERUN and M.recode(ks[77], M.equal16()).flags == 0
    pl = R.decode_points(pts)
    rest = list(ks)
    rest[77] = 0
    exp = R.encode_result(R.add(R.decode_result(util.oracle_msm(oracle, pts, R.encode_scalars(rest))), R.mul(pl[77], ks[77])))
    engine.set_narrow_max(0 if route == "even" else 1 << 16)
    try:
        run_case(engine, host_call(engine, pts), M.equal16(), ks, pts, FORM_TE, [0, 15], other, exp, small=(0, 15), reruns=1, label="rerun from " + route)
    finally:
        engine.set_narrow_max()


# ---- state ----
def test_capture_off_leaves_the_context_as_it_was(engine, oracle, golden, pool):
    """After set_stage_capture(0) the same context answers a golden vector and a narrow call exactly, and the as-run
    read-back refuses (MSM377_ESTATE) instead of returning what an earlier call left; so it does right after capture is
    switched on, before any call, after a call the mode does not describe (window partials that do not start at window
    0), and for the fixed-size read-back of mode 1 while mode 2 is set."""
    engine.set_stage_capture(2)
    with pytest.raises(msm.MsmError) as e:
        engine.read_stage_ex(0)
    assert e.value.code == ESTATE
    case = golden["g1_n1024_random"]
    assert engine.msm(case["points"], case["scalars"]) == case["expected"]
    info, _ = engine.read_stage_ex(21, want=())
    assert (info.slots, info.bucket_log) == (22, 11)
    with pytest.raises(msm.MsmError) as e:
        engine.read_stage_ex(22)
    assert e.value.code == ESTATE
    with pytest.raises(msm.MsmError) as e:  # sixteen windows of 2^15 buckets are not what this call ran
        engine.read_stage(0, 1024)
    assert e.value.code == ESTATE
    d_p, d_s = dev(case["points"]), dev(case["scalars"])
    engine.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), 1024, 8, 8)
    with pytest.raises(msm.MsmError) as e:
        engine.read_stage_ex(0)
    assert e.value.code == ESTATE
    with pytest.raises(msm.MsmError):
        engine.set_stage_capture(3)
    engine.set_stage_capture(0)
    with pytest.raises(msm.MsmError) as e:
        engine.read_stage_ex(0)
    assert e.value.code == ESTATE
    with util.edwards_only(engine):
        assert engine.msm(case["points"], case["scalars"]) == case["expected"]
        assert engine.last_geometry() == (22, 11)
        n = 700
        ks = R.encode_scalars(R.rand_scalars(0x0FF, n))
        assert engine.msm(pool[: 96 * n], ks) == util.oracle_msm(oracle, pool[: 96 * n], ks)
    with pytest.raises(msm.MsmError) as e:
        engine.read_stage_ex(0)
    assert e.value.code == ESTATE
    engine.set_stage_capture(1)  # mode 1 keeps its route: sixteen equal windows for the same small input
    try:
        assert engine.msm(case["points"], case["scalars"]) == case["expected"]
        assert engine.last_geometry() == (16, 15)
    finally:
        engine.set_stage_capture(0)


# ---- what the driver of a pass owns: the bookkeeping behind the last stage ----
def test_shard_call_leaves_nothing_describable(oracle, pool):
    """Capture mode 2 on a context of 2^12 points: a window-partials call for windows [3, 5) records its geometry (two
    slots of 2^15 buckets) and no stage layout -- the as-run read-back refuses -- and the whole call right after is
    describable again, with the slots its own pass ran."""
    n = 2049
    pts, ks = pool[: 96 * n], R.encode_scalars(R.rand_scalars(0x5A4D, n))
    d_p, d_s = dev(pts), dev(ks)
    eng = msm.MsmEngine(1 << 12)
    try:
        eng.set_stage_capture(2)
        eng.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 3, 2)
        with pytest.raises(msm.MsmError) as e:
            eng.read_stage_ex(0)
        assert e.value.code == ESTATE
        assert eng.last_geometry() == (2, 15)
        assert eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == util.oracle_msm(oracle, pts, ks)
        info, _ = eng.read_stage_ex(0, want=())
        assert info.slots == eng.last_geometry()[0]
    finally:
        eng.close()


def test_chunked_host_call_reports_the_geometry_of_its_back_phase(oracle, pool):
    """MSM377_UPLOAD_CHUNK_MIN=100, capture off: the chunks' front phases accumulate into one set of buckets and ONE back
    phase reduces them; last_geometry() is that phase's -- sixteen slots of 2^15 buckets on the chunked route at this n."""
    n = 2049
    pts, ks = pool[: 96 * n], R.encode_scalars(R.rand_scalars(0xC4A2, n))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_UPLOAD_CHUNK_MIN", "100")
        eng = msm.MsmEngine(1 << 12)
    try:
        assert eng.msm(pts, ks) == util.oracle_msm(oracle, pts, ks)
        assert eng.last_geometry() == (16, 15)
    finally:
        eng.close()
