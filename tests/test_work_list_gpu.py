"""The accumulation work list and the overflow partials of split rows (msm377_g1_read_work_list) at every work-item length
production runs, against tests/stage_model.py work_list / row_split (pinned by tests/test_stage_model_host.py, which also
compares the product's row_split with the model on the CPU).  tests/STAGES.md maps kernels to these tests and lists the
seeded faults they were shown to catch.

Every case runs the skewed input of tests/work_list_cases.py -- rows of 1, S - 1, S, S + 1, 2S, 2S + 1, 3S - 1, 31S + 1, 32S,
32S + 1 and 33S + 5 entries in EVERY window slot -- under a forced work-item length S (MSM377_SEG_PLAIN / MSM377_SEG_GLV) on
a fresh context, after one call with other scalars of the same size.  The work list is checked first (counters, histogram,
the list as a set and its order, the split-row list, the overflow ranges, the fold marks, every limb of every overflow
record, up to DECODE_CAP decoded partials), then three slots through check_slot of tests/test_stage_geometries_gpu.py,
then the result against the oracle.

The model's partial sum of work item s of a row is the sum of the signed base points of entries [s seglen, min((s + 1)
seglen, len)) of the row in the order val_idx holds them; the pool points are P_i = [a0 + i d]G, so the sum is worked out
on the logarithms and costs one scalar multiplication (as stage_model.partial_points does); the first records of every
case are also summed point by point with stage_model.bucket_sum, and the logarithms are tied to the wire points."""
import numpy as np
import pytest

import pyref as R
import stage_model as M
import util
import webgpu_msm_bls12_377_amd as msm
import work_list_cases as W
from test_g1_parity_gpu import dev
from test_stage_geometries_gpu import FORM_ED, FORM_TE, FORM_XYZZ, LIMBS, coordinate_shapes, decode, run_case, values_below, wire_points
from webgpu_msm_bls12_377_amd.host.engine import ESTATE, WORK_ROW_FOLDED

pytestmark = pytest.mark.gpu

DECODE_CAP = 300    # overflow records per case decoded with Python integers
CROSS_CHECK = 12    # of them also summed point by point with stage_model.bucket_sum
POOL_A0, POOL_D = 0x57A6E5, 0xD15717C7      # P_i = [POOL_A0 + i POOL_D] G
ED_A0, ED_D = 0xED57A6E5, 0xD15717C7
POOL_N = 138 * 128 + 8


@pytest.fixture(scope="module")
def pool(oracle):
    return util.oracle_gen_points(oracle, POOL_N, POOL_A0, POOL_D)


@pytest.fixture(scope="module")
def ed_pool(oracle):
    return util.oracle_ed_gen_points(oracle, POOL_N, ED_A0, ED_D)


def fresh_engine(env, cap=1 << 17):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        return msm.MsmEngine(cap)


def entries_of(vi, g, n):
    """(entry, sign) of val_idx words: a column of the slot (the wide table names record w * stride + i: column w n + i)."""
    rec = (vi & 0x7FFFFFFF).astype(np.int64)
    entry = (rec // n) * n + rec % n if g.name == "wide13" else rec
    return [(int(e), int(s)) for e, s in zip(entry, vi >> 31)]


def log_sum_point(pairs, slot, g, n, logs, ed, fold):
    """The sum of the signed bases of (entry, sign) pairs, on the logarithms of the pool points."""
    _, _, mul, ident, gen, order = M.group(ed)
    v = 0
    for entry, sign in pairs:
        i, factor = M.entry_weight(entry, slot, g, n, fold)
        v += -factor * logs[i] if sign else factor * logs[i]
    return mul(gen, v % order) if v % order else ident


def check_work_list(eng, case, form, cols, lens, wl, points, logs, slots, quad=0, fold_slot=-1, fold=False, verdict=""):
    """The read-back of the last call against the model `wl` of its row lengths `lens`; slots: where partials are decoded."""
    g, S, L = case.g, case.S, case.g.bucket_log
    ed = form == FORM_ED
    n = len(case.scalars)
    tag = "%s S=%d%s" % (g.name, S, verdict)
    info, got = eng.read_work_list()
    assert (info.seg, info.rows, info.quad, info.fold_slot) == (S, len(lens), quad, fold_slot), (tag, info[:8])
    assert (info.form, info.bucket_log, info.record_words) == (form, L, 4 * LIMBS[form]), (tag, info[:8])
    assert info.max_items == len(lens) + sum(len(c) for c in cols) // S, (tag, info.max_items)
    assert list(info.hist) == wl.hist, (tag, "histogram", [(b, x, y) for b, (x, y) in enumerate(zip(info.hist, wl.hist)) if x != y][:6])
    assert (info.items, info.split_rows, info.overflow_slots) == (wl.items, len(wl.split_rows), wl.overflow_slots), (tag, info.items, info.split_rows, info.overflow_slots)
    # the list as a set, and its order
    items = got["items"].astype(np.int64)
    assert items.shape == (wl.items, 2) and items[:, 1].max() < 256, tag
    key = items[:, 0] * 256 + items[:, 1]
    model_key = wl.item_set[:, 0] * 256 + wl.item_set[:, 1]  # sorted: item_set is sorted by (row, seg)
    assert np.array_equal(np.sort(key), model_key), (tag, "the work list is not the model's set of (row, seg)")
    length = wl.item_set[np.searchsorted(model_key, key), 2]
    down = np.nonzero(np.diff(length) > 0)[0]
    assert len(down) == 0, (tag, "item lengths increase along the list", int(down[0]), int(length[down[0]]), int(length[down[0] + 1]))
    # split rows and their overflow ranges
    split = got["split_rows"].astype(np.int64)
    assert np.array_equal(np.sort(split), np.array(wl.split_rows, dtype=np.int64)), (tag, "split-row list")
    word = got["row_ovf_base"][split].astype(np.int64)
    base, marked = word & ~WORK_ROW_FOLDED, (word & WORK_ROW_FOLDED) != 0
    count = np.array([M.row_split(int(lens[r]), S).nseg - 1 for r in split], dtype=np.int64)
    order = np.argsort(base, kind="stable")
    ends = base[order] + count[order]
    assert base[order][0] == 0 and np.array_equal(ends[:-1], base[order][1:]) and ends[-1] == wl.overflow_slots, (tag, "overflow ranges overlap or leave a gap")
    assert sorted(int(r) for r in split[marked]) == wl.folded, (tag, "fold marks", sorted(int(r) for r in split[marked]), wl.folded)
    if fold_slot < 0:
        assert not marked.any(), tag
    # every limb of every overflow record
    ovf = eng.read_work_list(want=(), ovf_first=0, ovf_count=wl.overflow_slots)[1]["ovf"]
    nl = LIMBS[form]
    assert ovf.shape == (wl.overflow_slots, 4 * nl), tag
    for ci, shape in enumerate(coordinate_shapes(form)):
        limbs = ovf[:, nl * ci : nl * ci + nl]
        assert (limbs <= np.array(shape.box, dtype=np.uint64)).all(), (tag, "overflow records: coordinate %d outside its stored box" % ci)
        assert values_below(limbs, shape.hi).all(), (tag, "overflow records: coordinate %d at or above its stored bound" % ci)
    # decoded partials: every item of the split rows of `slots`, shortest rows first
    base_of = {int(r): (int(b), bool(m)) for r, b, m in zip(split, base, marked)}
    decoded, folded_decoded = 0, 0
    for slot in dict.fromkeys([slots[0], slots[-1]] + list(slots)):  # slot 0, the top slot (the fold's), then the middle one
        st = eng.read_stage_ex(slot, want=("row_ptr", "val_idx"))[1]
        rp, vi = st["row_ptr"].astype(np.int64), st["val_idx"]
        rows = sorted((r for r in wl.split_rows if r >> L == slot), key=lambda r: int(lens[r]))
        for row in rows:
            t, ln = row & ((1 << L) - 1), int(lens[row])
            assert rp[t + 2] - rp[t + 1] == ln, (tag, slot, t)
            pairs = entries_of(vi[rp[t + 1] : rp[t + 2]], g, n)
            sp = M.row_split(ln, S)
            at, folded = base_of[row]
            todo = [(at, sp.seglen, ln)] if folded else [(at + s - 1,) + M.item_range(ln, S, s) for s in range(1, sp.nseg)]
            for rec, lo, hi in todo:
                if decoded >= DECODE_CAP:
                    break
                want = log_sum_point(pairs[lo:hi], slot, g, n, logs, ed, fold)
                if decoded < CROSS_CHECK and not fold and g.name != "wide13":
                    assert M.bucket_sum(points, pairs[lo:hi], g, n, ed=ed) == want, (tag, "the two models of a partial sum differ")
                where = (tag, "slot %d bucket %d (%d entries)" % (slot, t, ln), "the sum of its partials" if folded else "entries [%d, %d)" % (lo, hi), "overflow record %d" % rec)
                assert decode(ovf[rec], form) == want, where
                decoded += 1
                folded_decoded += folded
    assert decoded >= min(DECODE_CAP, 100), (tag, decoded)
    assert folded_decoded == len(wl.folded), (tag, "every folded row's sum is decoded", folded_decoded, len(wl.folded))
    return info


def prepare(case, points_wire, form, logs_a0_d):
    g = case.g
    n = len(case.scalars)
    cols, flags = M.digit_matrix(case.scalars, g)
    assert flags == 0
    lens = W.row_lengths(g, cols)
    points = wire_points(points_wire, form)
    a0, d = logs_a0_d
    logs = [a0 + i * d for i in range(n)]
    _, _, mul, _, gen, _ = M.group(form == FORM_ED)
    for i in (0, 1, n - 1):
        assert mul(gen, logs[i]) == points[i], "the pool is not the progression its logarithms promise"
    return cols, lens, points, logs


def three_slots(g):
    count = 1 if g.name == "wide13" else len(g.slots)
    return sorted({0, count // 2, count - 1})


def run_work_case(eng, call, case, points_wire, form, expected, pool_logs, quad=0, fold_slot=-1, label=""):
    """Work list, then check_slot on three slots, then the result: through run_case, whose call under test is wrapped so
    that the work list is read before run_case reads the stages."""
    g = case.g
    cols, lens, points, logs = prepare(case, points_wire, form, pool_logs)
    wl = M.work_list(lens, case.S, fold_slot=fold_slot, bucket_log=g.bucket_log)
    slots = three_slots(g)
    W.check_promises(case, lens, wl, slots)  # before anything runs on the GPU

    def wrapped(kk):
        got = call(kk)
        if kk is case.scalars:
            verdict = " [the call's result is %s]" % ("right" if got == expected else "WRONG")
            check_work_list(eng, case, form, cols, lens, wl, points, logs, slots, quad=quad, fold_slot=fold_slot, verdict=verdict)
        return got

    run_case(eng, wrapped, g, case.scalars, points_wire, form, slots, case.other, expected, small=slots, label=label)


def g1_case(oracle, pool, g, S, bound=R.R_ORDER):
    case = W.skewed(g, S, bound=bound)
    pts = pool[: 96 * len(case.scalars)]
    return case, pts, util.oracle_msm(oracle, pts, R.encode_scalars(case.scalars))


G1_LOGS = (POOL_A0, POOL_D)


# ---- the Edwards form of G1 on the even geometry ----
@pytest.mark.parametrize("S", [16, 24, 64, 120, 128])
def test_edwards_form_projective_records(oracle, pool, S):
    """k_work_hist / k_work_scatter bins up to S, k_accumulate<TeDev> chains of up to S additions, k_merge_split_rows_quad."""
    case, pts, exp = g1_case(oracle, pool, M.even16(), S)
    eng = fresh_engine({"MSM377_SEG_PLAIN": S})
    try:
        eng.set_narrow_max(0)
        run_work_case(eng, lambda kk: eng.msm(pts, R.encode_scalars(kk)), case, pts, FORM_TE, exp, G1_LOGS, label="te S=%d" % S)
        assert eng.accumulate_products() == 8
    finally:
        eng.close()


def test_edwards_form_affine_records(oracle, pool):
    """k_accumulate<TeDev, 2, TeAffBase> (MSM377_AFFINE_MIN lowered: 7 products)."""
    case, pts, exp = g1_case(oracle, pool, M.even16(), 64)
    eng = fresh_engine({"MSM377_SEG_PLAIN": 64, "MSM377_AFFINE_MIN": 1})
    try:
        eng.set_narrow_max(0)
        d_p = dev(pts)

        def call(kk):
            d_s = dev(R.encode_scalars(kk))
            return eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(kk))

        run_work_case(eng, call, case, pts, FORM_TE, exp, G1_LOGS, label="te affine S=64")
        assert eng.accumulate_products() == 7
    finally:
        eng.close()


@pytest.mark.parametrize("S", [24, 128])
def test_weierstrass_form(oracle, pool, S):
    """k_accumulate<G1Dev> on sixteen equal windows with a tracked top window; XYZZ overflow records."""
    case, pts, exp = g1_case(oracle, pool, M.equal16(), S)
    eng = fresh_engine({"MSM377_SEG_PLAIN": S})
    try:
        eng.set_narrow_max(0)
        eng.set_g1_form("weierstrass")
        run_work_case(eng, lambda kk: eng.msm(pts, R.encode_scalars(kk)), case, pts, FORM_XYZZ, exp, G1_LOGS, label="weierstrass S=%d" % S)
    finally:
        eng.close()


def test_glv_front_end(oracle, pool):
    """MSM377_SEG_GLV: eight slots of 2 n columns, every length twice per slot (P_i and phi(P_i) = [lambda] P_i)."""
    case, pts, exp = g1_case(oracle, pool, M.glv8(), 64)
    eng = fresh_engine({"MSM377_SEG_GLV": 64})
    try:
        eng.set_g1_form("weierstrass")
        eng.set_glv(True)
        run_work_case(eng, lambda kk: eng.msm(pts, R.encode_scalars(kk)), case, pts, FORM_XYZZ, exp, G1_LOGS, label="glv S=64")
    finally:
        eng.close()


@pytest.mark.parametrize("S", [24, 64])
def test_short_scalars_fold_long_rows(oracle, pool, S):
    """72-bit scalars in 16 bytes: five slots, the top one unsigned with 8 bits and the carry.  k_fold_long_rows is launched
    on it: its rows of 33 and 34 work items carry the fold mark and their first overflow record holds the sum of all
    their partials; its rows of 32 items, and the rows of 33 items of every other slot, do not."""
    g = M.short(72, 15)
    case, pts, exp = g1_case(oracle, pool, g, S, bound=1 << 72)
    eng = fresh_engine({"MSM377_SEG_PLAIN": S})
    try:
        eng.set_narrow_max(0)
        call = lambda kk: eng.msm_short(pts, b"".join(k.to_bytes(16, "little") for k in kk), 16, 72)  # noqa: E731
        run_work_case(eng, call, case, pts, FORM_TE, exp, G1_LOGS, fold_slot=len(g.slots) - 1, label="short S=%d" % S)
    finally:
        eng.close()


@pytest.mark.parametrize("S", [24, 64])
def test_edwards_bls12(oracle, ed_pool, S):
    """k_accumulate<EdDev>, k_merge_split_rows_quad<EdDev>: 36-word records from 12-word slots, no fold."""
    case = W.skewed(M.even16(), S, bound=R.ED_SUBGROUP)
    pts = ed_pool[: 64 * len(case.scalars)]
    exp = util.oracle_ed_msm(oracle, pts, R.encode_scalars(case.scalars))
    eng = fresh_engine({"MSM377_SEG_PLAIN": S})
    try:
        run_work_case(eng, lambda kk: eng.ed_msm(pts, R.encode_scalars(kk)), case, pts, FORM_ED, exp, (ED_A0, ED_D), label="ed S=%d" % S)
    finally:
        eng.close()


@pytest.mark.parametrize("lanes", ["quad", "thread"])
def test_narrow_path_with_a_forced_length(oracle, pool, lanes):
    """MSM377_SEG_PLAIN on the narrow path (22 slots of 2^11 buckets): k_accumulate_quad, and with
    MSM377_NARROW_QUAD_ITEMS=0 k_accumulate, over the same rows."""
    case, pts, exp = g1_case(oracle, pool, M.narrow22(), 64)
    env = {"MSM377_SEG_PLAIN": 64}
    if lanes == "thread":
        env["MSM377_NARROW_QUAD_ITEMS"] = 0
    eng = fresh_engine(env)
    try:
        run_work_case(eng, lambda kk: eng.msm(pts, R.encode_scalars(kk)), case, pts, FORM_TE, exp, G1_LOGS, quad=1 if lanes == "quad" else 0, label="narrow S=64 " + lanes)
    finally:
        eng.close()


# ---- behind a precomputed table: the rows and buckets of run_case's model do not describe these (check_slot is not run) ----
@pytest.mark.parametrize("table", ["table16", "wide"])
def test_precomputed_tables(oracle, pool, table):
    """The 16-bit table (window slot ws gathers [2^(16 ws)] P_i through its own table_stride) and the wide table (one slot of
    2^19 rows, 13 n columns, every length thirteen times): work list, overflow partials, result."""
    wide = table == "wide"
    g = M.wide13() if wide else M.equal16()
    case, pts, exp = g1_case(oracle, pool, g, 64)
    cols, lens, points, logs = prepare(case, pts, FORM_TE, G1_LOGS)
    wl = M.work_list(lens, 64, bucket_log=g.bucket_log)
    slots = three_slots(g)
    W.check_promises(case, lens, wl, slots)
    eng = fresh_engine({"MSM377_SEG_PLAIN": 64})
    try:
        eng.set_precompute_window(20 if wide else 16)
        eng.set_bases_precomputed(pts)
        eng.set_stage_capture(2)
        before, _ = eng.fallback_info()
        eng.msm_fixed_base(R.encode_scalars(case.other))
        got = eng.msm_fixed_base(R.encode_scalars(case.scalars))
        verdict = " [the call's result is %s]" % ("right" if got == exp else "WRONG")
        assert eng.fallback_info()[0] == before
        stage = eng.read_stage_ex(0, want=())[0]
        assert (stage.slots, stage.bucket_log, stage.table_stride) == (1 if wide else 16, g.bucket_log, len(case.scalars)), stage
        check_work_list(eng, case, FORM_TE, cols, lens, wl, points, logs, slots, fold=not wide, verdict=verdict)
        assert got == exp
    finally:
        eng.close()


# ---- routes capture does not describe: the result on the same skewed input ----
def test_chunked_upload_continues_split_rows(oracle, pool):
    """MSM377_UPLOAD_CHUNK_MIN=100: later chunks accumulate `into` the buckets of the earlier ones, so the first item of a
    split row continues from a bucket while its other items start fresh."""
    case, pts, exp = g1_case(oracle, pool, M.even16(), 64)
    eng = fresh_engine({"MSM377_SEG_PLAIN": 64, "MSM377_UPLOAD_CHUNK_MIN": 100})
    try:
        eng.set_narrow_max(0)
        with util.edwards_only(eng):
            assert eng.msm(pts, R.encode_scalars(case.scalars)) == exp
    finally:
        eng.close()


def test_twin_batch(oracle, pool):
    """A fixed-base batch large enough to run as two halves on the twin context (four MSMs: two each)."""
    case, pts, exp = g1_case(oracle, pool, M.even16(), 64)
    exp_other = util.oracle_msm(oracle, pts, R.encode_scalars(case.other))
    eng = fresh_engine({"MSM377_SEG_PLAIN": 64})
    try:
        eng.set_narrow_max(0)
        eng.set_bases(pts)
        a, b = R.encode_scalars(case.scalars), R.encode_scalars(case.other)
        d_s = dev(a + b + b + a)
        with util.edwards_only(eng):
            assert eng.msm_fixed_base_batch_device(d_s.data_ptr(), len(case.scalars), 4) == [exp, exp_other, exp_other, exp]
    finally:
        eng.close()


# ---- the rule without a forced length ----
@pytest.mark.parametrize("n,seg", [(278528, 24), (278527, 16)])
def test_unforced_rule(engine, oracle, n, seg):
    """auto_seg: ((entries >> 18) + 7) & ~7 with entries = 16 n: 24 from n = 17 x 2^14 on, 16 one point below."""
    pts = util.oracle_gen_points(oracle, n, 0xA070, 0x5E6)
    ks = R.encode_scalars(R.rand_scalars(0xA071, n))
    d_p, d_s = dev(pts), dev(ks)
    engine.set_stage_capture(2)
    try:
        with util.edwards_only(engine):
            got = engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n)
        info, _ = engine.read_work_list(want=())
        assert (info.seg, info.rows, info.fold_slot, info.quad) == (seg, 16 << 15, -1, 0)
        assert info.items == sum(info.hist) <= info.max_items == info.rows + 16 * n // seg
    finally:
        engine.set_stage_capture(0)
    assert got == util.oracle_msm(oracle, pts, ks)


# ---- when the read-back answers ----
def test_read_back_stops_answering_after_a_check_call(engine, oracle, pool):
    """MSM377_ESTATE with capture off, before a call, after a window-partials call from window 8 and -- the header's rule --
    after a check call or a width measurement, which use the front of the work-list block as scratch; the stage read-back
    still answers there, and the next MSM is described again.  A refusal writes nothing."""
    n = 3000
    pts, ks = pool[: 96 * n], R.encode_scalars(R.rand_scalars(0xE57A, n))
    d_p, d_s = dev(pts), dev(ks)

    def refuses():
        with pytest.raises(msm.MsmError) as e:
            engine.read_work_list()
        assert e.value.code == ESTATE

    refuses()  # capture off
    engine.set_stage_capture(2)
    try:
        refuses()  # nothing captured yet
        exp = util.oracle_msm(oracle, pts, ks)
        assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp
        info, got = engine.read_work_list()
        assert info.items == len(got["items"]) == sum(info.hist) and info.rows == len(got["row_ovf_base"]) == 22 << 11 and info.quad == 1
        with pytest.raises(msm.MsmError) as e:  # a record range outside the overflow records: EINVAL
            engine.read_work_list(want=(), ovf_first=info.overflow_slots, ovf_count=1)
        assert e.value.code == -1
        engine.check_points_device(d_p.data_ptr(), n)
        refuses()
        engine.read_stage_ex(0, want=())  # the stage read-back does not depend on those words
        assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp
        assert engine.read_work_list(want=())[0] == info
        assert engine.scalars_width_device(d_s.data_ptr(), n, 32) > 240
        refuses()
        assert engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), n) == exp
        assert engine.read_work_list(want=())[0] == info
        engine.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, 8, 8)
        refuses()
    finally:
        engine.set_stage_capture(0)
    refuses()
