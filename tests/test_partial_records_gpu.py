"""The window records -- what the bucket reduction (csrc/kernels/reduce.hpp) hands to the host tail -- read back with
msm377_g1_read_partials and compared point by point with tests/stage_model.py partial_points (pinned by
tests/test_stage_model_host.py): every point of every record up to `planes`, its words against the record contract of
include/msm377.h, its invariant, its value, and `info` against the geometry and the reduction schedule.  tests/STAGES.md
maps the kernels of reduce.hpp to these tests and lists the seeded faults they were shown to catch.

Baselines go through run_case of tests/test_stage_geometries_gpu.py, with the records as the last stage behind digits,
rows and buckets.  The crafted inputs of tests/partial_cases.py (planted planes, the level ladder) hold a handful of
entries; they go through run_records, which keeps run_case's order -- records before the result, the failure says whether
the result was right -- and its comparisons of geometry_reruns and fallback_info around the call."""
import contextlib
import functools

import pytest

import partial_cases as C
import pyref as R
import stage_model as M
import util
import webgpu_msm_bls12_377_amd as msm
from ed_curve_points import subgroup_points
from test_g1_parity_gpu import dev
from test_stage_geometries_gpu import FORM_ED, FORM_TE, FORM_XYZZ, check_records, run_case
from webgpu_msm_bls12_377_amd.host.engine import ESTATE, FB_TREE

pytestmark = pytest.mark.gpu

POOL_A0, POOL_D = 0x57A6E5, 0xD15717C7  # P_i = [POOL_A0 + i POOL_D] G: the logarithms the model sums
ED_A0, ED_D = 0x1234567, 0x89ABCDF


@pytest.fixture(scope="module")
def pool(oracle):
    return util.oracle_gen_points(oracle, 5000, POOL_A0, POOL_D)


def pool_logs(n):
    return [POOL_A0 + i * POOL_D for i in range(n)]


# ---- routes: how a geometry is reached, on the session's engine or on one made under other settings ----
class Route:
    """g: the geometry the route promises; form; call(points_wire, scalars) -> result bytes; enter/leave set the engine up."""

    def __init__(self, name, g, form, fold=False):
        self.name, self.g, self.form, self.fold, self.ed = name, g, form, fold, form == FORM_ED


ROUTES = {
    "even": Route("even", M.even16(), FORM_TE),
    "weierstrass": Route("weierstrass", M.equal16(), FORM_XYZZ),
    "narrow": Route("narrow", M.narrow22(), FORM_TE),
    "short": Route("short", M.short(64, 15), FORM_TE),
    "short-narrow": Route("short-narrow", M.short(64, 11), FORM_TE),
    "wide": Route("wide", M.wide13(), FORM_TE),
    "table16": Route("table16", M.equal16(), FORM_TE, fold=True),
    "glv": Route("glv", M.glv8(), FORM_XYZZ),
    "ed": Route("ed", M.even16(), FORM_ED),
}


@contextlib.contextmanager
def on_route(engine, route):
    """The engine set up so that a small call takes `route`; yields call(points_wire, scalars_ints) -> result."""
    name = route.name
    table = {}
    try:
        if name in ("even", "short", "weierstrass", "glv", "ed"):
            engine.set_narrow_max(0)
        if name in ("weierstrass", "glv"):
            engine.set_g1_form("weierstrass")
        if name == "glv":
            engine.set_glv(True)
        if name == "wide":
            engine.set_precompute_window(20)

        def call(points_wire, ks):
            if name in ("short", "short-narrow"):
                return engine.msm_short(points_wire, b"".join(k.to_bytes(8, "little") for k in ks), 8, 64)
            if name in ("wide", "table16"):
                if table.get("points") != points_wire:
                    engine.set_bases_precomputed(points_wire)
                    table["points"] = points_wire
                return engine.msm_fixed_base(R.encode_scalars(ks))
            if name == "ed":
                return engine.ed_msm(points_wire, R.encode_scalars(ks))
            return engine.msm(points_wire, R.encode_scalars(ks))

        yield call
    finally:
        if name in ("wide", "table16"):
            engine.set_precompute_window(16)
            engine.msm(R.encode_points([R.G]), R.encode_scalars([1]))  # drops the resident table
        engine.set_glv("auto")
        engine.set_g1_form("edwards")
        engine.set_narrow_max()


_PREPARED = {}


def prepared(case):
    """(points as the engine takes them, the model's records, the expected result) of a case: worked out once and shared by
    every test and parameter that runs the case."""
    key = (case.name, case.g.name, case.ed, case.fold, tuple(case.scalars))
    if key not in _PREPARED:
        _PREPARED[key] = (C.wire(case)[0], C.model_records(case), C.expected_result(case))
    return _PREPARED[key]


def run_records(engine, call, route, case, schedule=None, reruns=0, fallbacks=0, label=""):
    """One crafted call under capture mode 2: the records against the model, THEN the result; geometry_reruns and
    fallback_info compared before and after, as run_case does.  Returns the read-back's info."""
    label = "%s / %s %s" % (route.name, case.name, label)
    points_wire, model, expected = prepared(case)
    other = [3 + 2 * i for i in range(len(case.scalars))]  # the call before: other scalars, same size, same context
    assert sorted(other) != sorted(case.scalars)
    engine.set_stage_capture(2)
    try:
        call(points_wire, other)
        before, _ = engine.fallback_info()
        reruns_before = engine.read_stage_ex(0, want=())[0].geometry_reruns
        got = call(points_wire, case.scalars)
        try:
            assert engine.fallback_info()[0] == before + fallbacks, (label, "reruns on the Weierstrass path", engine.fallback_info())
            stage = engine.read_stage_ex(0, want=())[0]
            assert stage.geometry_reruns == reruns_before + reruns, (label, "reruns on another window geometry", stage.geometry_reruns - reruns_before)
            assert (stage.slots, stage.bucket_log, stage.form) == (1 if route.g.name == "wide13" else len(route.g.slots), route.g.bucket_log, route.form), (label, stage)
            info = check_records(engine, route.g, model, route.form, fold=route.fold, label=label, schedule=schedule)
        except AssertionError as e:
            raise AssertionError("%s [the call's result is %s]" % (str(e).split("\n")[0], "right" if got == expected else "WRONG")) from e
        assert got == expected, (label, "every record agrees with the model, the result does not")
        return info
    finally:
        engine.set_stage_capture(0)


# ---- baselines: every geometry through the whole chain digits -> rows -> buckets -> records -> result ----
def baseline(engine, oracle, pool, route, n, seed, slots, small=(), schedule=None, device=False):
    g = route.g
    pts = pool[: 96 * n]
    ks, other = R.rand_scalars(seed, n), R.rand_scalars(seed + 1, n)
    if g.name == "short":
        ks, other = [k & ((1 << 64) - 1) for k in ks], [k & ((1 << 64) - 1) for k in other]
    cols, flags = M.digit_matrix(ks, g)
    assert flags == 0
    model = M.partial_points(R.decode_points(pts), cols, g, n, logs=pool_logs(n), fold=route.fold)
    exp = util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    with on_route(engine, route) as call:
        if device:  # device buffers: the route that converts to affine records under MSM377_AFFINE_MIN
            d_p = dev(pts)

            def call(_, kk):
                d_s = dev(R.encode_scalars(kk))
                return engine.msm_device(d_p.data_ptr(), d_s.data_ptr(), len(kk))

        run_case(engine, lambda kk: call(pts, kk), g, ks, pts, route.form, slots, other, exp, small=small, label="records baseline " + route.name, records=model,
                 schedule=schedule)


def test_even_geometry_projective_records(engine, oracle, pool):
    baseline(engine, oracle, pool, ROUTES["even"], 5000, 0xB000, [0, 12, 15])
    assert engine.accumulate_products() == 8


def test_even_geometry_affine_records(oracle, pool):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_AFFINE_MIN", "1")
        eng = msm.MsmEngine(1 << 13)
    try:
        baseline(eng, oracle, pool, ROUTES["even"], 5000, 0xB010, [0, 12, 15], device=True)
        assert eng.accumulate_products() == 7
    finally:
        eng.close()


def test_sixteen_equal_windows_in_weierstrass_form(engine, oracle, pool):
    baseline(engine, oracle, pool, ROUTES["weierstrass"], 5000, 0xB020, [0, 8, 15])


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_narrow_geometry(engine, oracle, pool, n):
    """22 records of 11 planes: k_tree_columns over levels 0-3, k_reduce_tail_lds at L = 11."""
    tiny = n <= 257
    slots = range(22) if tiny else [0, 10, 21]
    baseline(engine, oracle, pool, ROUTES["narrow"], n, 0xB030 + n, slots, small=slots if tiny else ())


@pytest.mark.parametrize("route", ["short", "short-narrow"])
def test_short_call(engine, oracle, pool, route):
    """8 bytes / 64 bits: five records of 15 planes on the main path, six of 11 on the narrow one; the top slot holds carries."""
    r = ROUTES[route]
    top = len(r.g.slots) - 1
    baseline(engine, oracle, pool, r, 4096 if route == "short" else 1000, 0xB040, [0, top - 1, top], small=[top])


@pytest.mark.parametrize("n", [257, 2049])
def test_wide_table(engine, oracle, pool, n):
    """One record of 20 points over 2^19 buckets: three column launches and the tail.  13 x 257 entries cannot offer
    run_case's 50 rows of two and more entries among 2^19 buckets, and decoding all 3341 takes a minute: that size
    compares records and result, 2049 the whole chain."""
    if n == 2049:
        return baseline(engine, oracle, pool, ROUTES["wide"], n, 0xB050 + n, [0])
    pts = pool[: 96 * n]
    case = C.Case("n=%d" % n, M.wide13(), R.rand_scalars(0xB050 + n, n), R.decode_points(pts), pool_logs(n), {}, {})
    assert C.expected_result(case) == util.oracle_msm(oracle, pts, R.encode_scalars(case.scalars))
    with on_route(engine, ROUTES["wide"]) as call:
        info = run_records(engine, call, ROUTES["wide"], case)
    assert (info.records, info.points, info.planes) == (1, 20, 19)


def test_glv_front_end(engine, oracle, pool):
    baseline(engine, oracle, pool, ROUTES["glv"], 5000, 0xB060, [0, 7])


def table16_call(engine, oracle, pool, n, seed, schedule=None):
    pts = pool[: 96 * n]
    ks = R.rand_scalars(seed, n)
    ks[:3] = [0, 1, R.R_ORDER - 1]
    case = C.Case("n=%d" % n, M.equal16(), ks, R.decode_points(pts), pool_logs(n), {}, {}, fold=True)
    assert C.expected_result(case) == util.oracle_msm(oracle, pts, R.encode_scalars(ks))
    with on_route(engine, ROUTES["table16"]) as call:
        return run_records(engine, call, ROUTES["table16"], case, schedule=schedule)


def test_precomputed_16_bit_table_folds_sixteen_slots_into_one_record(engine, oracle, pool):
    """k_fold_windows 16 -> 8 -> 4 -> 2 -> 1: the one record is the sum over all sixteen slots, slot w weighted 2^(16 w) by
    its table.  (run_case's row and bucket model does not describe table records of sixteen slots: records and result.)"""
    info = table16_call(engine, oracle, pool, 2049, 0xB070)
    assert (info.records, info.folded_slots) == (1, 16)


def ed_pool(n):
    return subgroup_points(n, ED_A0, ED_D), [ED_A0 + i * ED_D for i in range(n)]


@pytest.mark.parametrize("windows", ["even", "equal"])
def test_edwards_bls12_call(engine, oracle, monkeypatch, windows):
    """Records of 8 words per coordinate, no tag; the even geometry, and sixteen equal windows under MSM377_EVEN_WINDOWS=0."""
    n = 5000
    points, logs = ed_pool(n)
    pts = R.ed_encode_points(points)
    g = M.even16() if windows == "even" else M.equal16()
    rnd_ks = R.rand_scalars(0xB080, n + 50, modulus=1 << 253)
    ks = [k for k in rnd_ks if M.recode(k, g).flags == 0][:n]
    other = [k ^ 0x5555 for k in ks]
    cols, _ = M.digit_matrix(ks, g)
    model = M.partial_points(points, cols, g, n, logs=logs, ed=True)
    exp = util.oracle_ed_msm(oracle, pts, R.encode_scalars(ks))
    assert R.ed_encode_result(M.weighted_sum(model, g, ed=True)) == exp
    if windows == "equal":
        monkeypatch.setenv("MSM377_EVEN_WINDOWS", "0")
        monkeypatch.setenv("MSM377_TWIN_BATCH", "0")
        eng = msm.MsmEngine(1 << 13)
    else:
        eng = engine
    try:
        run_case(eng, lambda kk: eng.ed_msm(pts, R.encode_scalars(kk)), g, ks, pts, FORM_ED, [0, 15], other, exp, label="records baseline ed " + windows, records=model)
    finally:
        if eng is not engine:
            eng.close()


# ---- planted planes ----
PLANTED = ["even", "weierstrass", "narrow", "short", "short-narrow", "glv", "ed"]


@pytest.mark.parametrize("route", PLANTED)
def test_planted_planes(engine, route):
    """Window w holds ONE point, in bucket index 2^b: plane b and the total are that point, every other plane the identity
    as stored.  Then index 0, index 2^L - 1, an empty window and a window whose total cancels while its planes do not."""
    r = ROUTES[route]
    halves = [range(8), range(8, 16)] if route == "glv" else [None]
    with on_route(engine, r) as call:
        for use in halves:
            for case in C.planted(r.g, ed=r.ed, use=use):
                run_records(engine, call, r, case)
        for case in C.extras(r.g, ed=r.ed):
            run_records(engine, call, r, case)


@pytest.mark.parametrize("route", ["wide", "table16"])
def test_planted_planes_of_a_single_record(engine, route):
    """One record: one call per plane (19 on the wide table, 15 behind the folded one), the digit moving through the
    digit columns / slots, whose table windows carry the weights; then the extras, one call each."""
    r = ROUTES[route]
    with on_route(engine, r) as call:
        for case in C.planted(r.g, fold=r.fold) + C.extras(r.g, fold=r.fold):
            run_records(engine, call, r, case)


# ---- the level ladder ----
def ladder_cases(r, kind, age):
    return _ladder_cases(r.name, kind, age)


@functools.lru_cache(maxsize=None)
def _ladder_cases(route, kind, age):
    """Every level of the route's tree: one call where the geometry has a window per level, else as many as it takes."""
    r = ROUTES[route]
    L, free = r.g.bucket_log, C.positions(r.g)
    if r.g.name == "glv8":
        uses = [range(0, 8), range(8, 16)]  # k1's windows (P), then k2's (phi(P))
    else:
        uses = [None]
    levels, cases = [lv for lv in range(L) if lv - age >= 0], []
    for use in uses:
        todo = list(levels)
        while todo:
            case = C.ladder(r.g, kind, ed=r.ed, age=age, use=use, levels=todo)
            done = C.levels_in(case)
            assert done, (r.name, kind, age, todo)
            cases.append(case)
            todo = [lv for lv in todo if lv not in done]
    assert sorted({lv for c in cases for lv in C.levels_in(c)}) == levels
    return cases


def which_kernel(info, level):
    """The kernel that ran a level, from the schedule the read-back reports."""
    if level >= info.tail_from:
        return "k_reduce_tail_lds" if info.tail_lds else "k_reduce_tail"
    if info.columns:
        return "k_tree_columns"
    return "k_tree_step_quad" if level >= info.coop_from else "k_tree_step"


LADDER = ["even", "narrow", "weierstrass", "glv", "ed"]


@pytest.mark.parametrize("kind", C.SECOND)
@pytest.mark.parametrize("route", LADDER)
def test_level_ladder(engine, route, kind):
    """A window's only two entries at bucket indices 0 and 2^L >> (r + 1) first meet at level r of its tree, in the running
    block: a doubling, a cancellation (total O, plane -P) or an ordinary addition at EVERY level, a different level in each
    window.  At the defaults the levels belong to k_tree_columns and k_reduce_tail_lds; `info` says which."""
    r = ROUTES[route]
    kernels = set()
    with on_route(engine, r) as call:
        for case in ladder_cases(r, kind, 0):
            info = run_records(engine, call, r, case)
            kernels |= {which_kernel(info, lv) for lv in C.levels_in(case)}
    assert kernels == {"k_tree_columns", "k_reduce_tail_lds"}, kernels


@pytest.mark.parametrize("kind", ["order2", "order4"])
def test_level_ladder_with_low_order_points_of_edwards_bls12(engine, kind):
    r = ROUTES["ed"]
    with on_route(engine, r) as call:
        for case in ladder_cases(r, kind, 0):
            run_records(engine, call, r, case)


@pytest.mark.parametrize("age", [1, 3])
@pytest.mark.parametrize("kind", C.SECOND)
@pytest.mark.parametrize("route", LADDER)
def test_level_ladder_inside_a_list(engine, route, kind, age):
    """The pair at lo + k and lo + k + half inside the list that level r - age left behind: the high lanes' re-pairing in
    k_tree_columns and the nlists > 1 arm of the tail (the pair also meets in the running block, whose upper half it sat in)."""
    r = ROUTES[route]
    with on_route(engine, r) as call:
        for case in ladder_cases(r, kind, age):
            run_records(engine, call, r, case)


@pytest.mark.parametrize("kind", C.SECOND)
def test_level_ladder_on_the_wide_table(engine, kind):
    """One window of 2^19 buckets: one call per level, at the first and last level of each launch -- read from `info`."""
    r = ROUTES["wide"]
    with on_route(engine, r) as call:
        info = run_records(engine, call, r, C.ladder(r.g, kind, levels=[0]))
        assert (info.columns, info.tail_from, info.planes) == (1, 11, 19), info
        edges, lv = [], 0
        while lv < info.tail_from:  # column launches of up to four levels
            last = min(lv + 4, info.tail_from) - 1
            edges += [lv, last]
            lv = last + 1
        edges += [info.tail_from, info.planes - 1]
        assert edges == [0, 3, 4, 7, 8, 10, 11, 18]
        for lv in edges[1:]:
            run_records(engine, call, r, C.ladder(r.g, kind, levels=[lv]))
        run_records(engine, call, r, C.ladder(r.g, kind, age=2, levels=[9]))  # a list inside the third column launch
        run_records(engine, call, r, C.ladder(r.g, kind, age=3, levels=[15]))  # a list the tail's block spawned


# ---- schedules ----
TS, TSQ, TC, RT, RTL = "k_tree_step", "k_tree_step_quad", "k_tree_columns", "k_reduce_tail", "k_reduce_tail_lds"
BIG, SMALL, TINY = "100000000", "65536", "16"  # MSM377_COOP_THREADS: lane quads from level 0 on; from level 7 (16 windows of 2^15); at no level
# (settings, what `info` must report, kernels that take levels of a sixteen-window call, kernels of a narrow call: 22 windows
# of 2^11 buckets are down to the default 131072 threads at level 0 already, so their per-level launches are lane quads)
SCHEDULES = [
    ({"MSM377_REDUCE_COLUMNS": "0"}, {"columns": 0, "coop_from": 6, "tail_from": 7, "tail_lds": 1}, {TS, TSQ, RTL}, {TSQ, RTL}),
    ({"MSM377_TAIL_LDS": "0"}, {"columns": 1, "tail_lds": 0, "tail_from": 7}, {TC, RT}, {TC, RT}),
    ({"MSM377_TAIL_FROM": "15"}, {"columns": 1, "tail_from": 15, "tail_lds": 0}, {TC}, {TC, RTL}),
    ({"MSM377_REDUCE_COLUMNS": "0", "MSM377_TAIL_FROM": "15"}, {"columns": 0, "coop_from": 6, "tail_from": 15}, {TS, TSQ}, {TSQ, RTL}),
    ({"MSM377_REDUCE_COLUMNS": "0", "MSM377_TAIL_FROM": "15", "MSM377_COOP_THREADS": TINY}, {"columns": 0, "coop_from": 15, "tail_from": 15}, {TS}, {TS, RTL}),
    ({"MSM377_REDUCE_COLUMNS": "0", "MSM377_TAIL_FROM": "15", "MSM377_COOP_THREADS": BIG}, {"columns": 0, "coop_from": 0, "tail_from": 15}, {TSQ}, {TSQ, RTL}),
    ({"MSM377_NARROW_TAIL_FROM": "1", "MSM377_COOP_THREADS": BIG}, {"columns": 1, "coop_from": 0}, {TC, RTL}, {TC, RT}),
    ({"MSM377_NARROW_TAIL_FROM": "1", "MSM377_COOP_THREADS": SMALL}, {"columns": 1}, {TC, RTL}, {TC, RT}),
    ({"MSM377_REDUCE_COLUMNS": "0", "MSM377_NARROW_TAIL_FROM": "1", "MSM377_COOP_THREADS": BIG}, {"columns": 0, "coop_from": 0}, {TSQ, RTL}, {TSQ, RT}),
    ({"MSM377_REDUCE_COLUMNS": "0", "MSM377_NARROW_TAIL_FROM": "1", "MSM377_COOP_THREADS": SMALL}, {"columns": 0}, {TS, RTL}, {TS, RT}),
]


@functools.lru_cache(maxsize=None)
def _schedule_baseline(name, pts):
    n = len(pts) // 96
    return C.Case("baseline n=%d" % n, ROUTES[name].g, R.rand_scalars(0xB0A0, n), R.decode_points(pts), pool_logs(n), {}, {})


def schedule_baseline(oracle, pool, name):
    """5000 random scalars over the pool; records and result (the whole chain runs at the defaults, in the baselines above)."""
    case = _schedule_baseline(name, pool)
    assert prepared(case)[2] == util.oracle_msm(oracle, pool, R.encode_scalars(case.scalars))
    return case


@pytest.mark.parametrize("knobs,schedule,main_kernels,narrow_kernels", SCHEDULES,
                         ids=[",".join("%s=%s" % (a.replace("MSM377_", ""), b) for a, b in s[0].items()) for s in SCHEDULES])
def test_schedules(oracle, pool, monkeypatch, knobs, schedule, main_kernels, narrow_kernels):
    """The ladder (doubling and cancellation, in the block and in a list) and one baseline under the settings that move
    levels to k_tree_step, k_tree_step_quad and k_reduce_tail: Edwards form on the main and the narrow path, Weierstrass
    form, Edwards-BLS12.  Which kernel ran which level is read from `info`, not assumed.  Over the parameters k_tree_step
    and k_tree_step_quad each take all fifteen levels of a sixteen-window tree (TAIL_FROM=15 with COOP_THREADS tiny /
    huge) and k_reduce_tail takes levels 7-14 there and 1-10 of the narrow tree (NARROW_TAIL_FROM=1: 213 KB of buckets
    per workgroup do not fit the LDS)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    eng = msm.MsmEngine(1 << 13)
    try:
        for name in ("even", "narrow", "weierstrass", "ed"):
            r = ROUTES[name]
            narrow = name == "narrow"
            want = {k: v for k, v in schedule.items() if not narrow or k == "columns"}  # tail_from / coop_from below are those of sixteen windows of 2^15 buckets
            if narrow:
                want["tail_from"] = int(knobs.get("MSM377_NARROW_TAIL_FROM", 4))
            seen = {}
            with on_route(eng, r) as call:
                for kind in ("same", "negative"):
                    for age in (0, 2):
                        for case in ladder_cases(r, kind, age):
                            info = run_records(eng, call, r, case, schedule=want, label=str(knobs))
                            for lv in C.levels_in(case):
                                seen.setdefault(which_kernel(info, lv), set()).add(lv)
            assert set(seen) == (narrow_kernels if narrow else main_kernels), (name, seen)
            assert sorted(lv for lvs in seen.values() for lv in lvs) == list(range(r.g.bucket_log)), (name, seen)
        for name in ("even", "narrow") if "MSM377_NARROW_TAIL_FROM" in knobs else ("even",):
            want = schedule if name == "even" else {"columns": schedule["columns"], "tail_from": 1, "tail_lds": 0}
            with on_route(eng, ROUTES[name]) as call:
                run_records(eng, call, ROUTES[name], schedule_baseline(oracle, pool, name), schedule=want, label=str(knobs))
    finally:
        eng.close()


# ---- mode switches ----
def test_read_back_refuses_wherever_the_stage_read_back_does(engine, golden):
    """MSM377_ESTATE before any call under the mode, after a shard call that does not start at window 0, and with capture
    off; nothing is written then.  After a described call it answers, and again refuses once capture is off."""
    def refused():
        with pytest.raises(msm.MsmError) as e:
            engine.read_partials()
        assert e.value.code == ESTATE

    refused()  # capture off
    case = golden["g1_n1024_random"]
    engine.set_stage_capture(2)
    try:
        refused()  # before any call
        assert engine.msm(case["points"], case["scalars"]) == case["expected"]
        info, words = engine.read_partials()
        assert (info.records, info.planes, info.points) == (22, 11, 16) and words.shape == (22, 16, 4, 12)
        d_p, d_s = dev(case["points"]), dev(case["scalars"])
        engine.window_partials_device(d_p.data_ptr(), d_s.data_ptr(), 1024, 8, 8)
        refused()  # a shard call that does not start at window 0
    finally:
        engine.set_stage_capture(0)
    refused()
    assert engine.msm(case["points"], case["scalars"]) == case["expected"]
    refused()


@pytest.mark.parametrize("route", ["even", "narrow"])
def test_after_a_geometry_rerun_the_records_are_those_of_sixteen_equal_windows(engine, oracle, pool, route):
    """A scalar of 2^253 and more fits neither the even nor the narrow geometry: the pass is discarded and the read-back
    describes the pass on sixteen equal windows that produced the result -- exactly one rerun."""
    n = 500
    pts = pool[: 96 * n]
    ks = R.rand_scalars(0xB0B0, n)
    ks[77] = (1 << 253) + 99
    first = ROUTES[route].g
    assert M.recode(ks[77], first).flags == M.ERR_RERUN and M.recode(ks[77], M.equal16()).flags == 0
    case = C.Case("rerun from " + route, M.equal16(), ks, R.decode_points(pts), pool_logs(n), {}, {})
    after = Route(route, M.equal16(), FORM_TE)
    with on_route(engine, ROUTES[route]) as call:
        info = run_records(engine, call, after, case, reruns=1)
    assert (info.records, info.planes, info.tail_short_from) == (16, 15, 0)


def test_after_a_tree_exception_the_records_are_weierstrass_records(engine):
    """P and P + T' (util.t_prime: an exceptional pair of the a = -1 law) in two buckets the tree adds at level 2: the
    Edwards pass raises the tree's flag, the call reruns in Weierstrass form, and the read-back describes THAT pass --
    untagged XYZZ records of sixteen equal windows whose window 0 holds the exact sum."""
    p = R.mul(R.G, 31337)
    q = R.add(p, util.t_prime())
    g = M.equal16()
    half = (1 << 15) >> 3
    ks = [C.scalar_from_digits(g, {0: 1}), C.scalar_from_digits(g, {0: half + 1})]
    assert M.meetings(0, half, 15) == [(2, 0)]
    case = C.Case("tree exception", g, ks, [p, q], [None, None], {0: {0, half}}, {0: [(2, 0)]})
    after = Route("even", g, FORM_XYZZ)
    with on_route(engine, ROUTES["even"]) as call:
        info = run_records(engine, call, after, case, fallbacks=1)
    assert engine.fallback_info()[1] & FB_TREE
    assert info.tail_kind == 1
