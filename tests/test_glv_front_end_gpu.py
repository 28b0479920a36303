"""k_decompose_glv as run, on the inputs that reach its arms (tests/STAGES.md, "The GLV front end at its arms"): exact
multiples of lambda -- the ONLY scalars that take the correction of the Barrett quotient (pinned on the host by
tests/test_stage_model_host.py over csrc/glv_split.hpp) --, every boundary digit in every window of both halves, both
sides of the edge of the GLV range; inputs where P_j = +-phi(P_i), so that the two halves of the digit matrix add the SAME
point -- in one bucket, at the split-row merge, in the tree --; and the routes of a GLV table and a GLV upload that no
other test takes (short call, prefix call, chunked upload, native input forms).  Stage read-backs through run_case /
check_slot of tests/test_stage_geometries_gpu.py, window records through run_records of tests/test_partial_records_gpu.py,
against tests/stage_model.py; the crafted scalars come from tests/glv_cases.py.

Every stage case: n = 3000, crafted scalars on lanes 0, 1, 63, 64, 255, 256, 2999 and inside, random ones elsewhere; the
floors of run_case hold from the model before anything runs; all 8 slots are read whole; no rerun on another geometry and
no fallback unless the case says so."""
import pytest

import glv_cases as GC
import partial_cases as C
import pyref as R
import stage_model as M
import util
import webgpu_msm_bls12_377_amd as msm
import work_list_cases as W
from test_g1_parity_gpu import dev
from test_partial_records_gpu import ROUTES, on_route, run_records, which_kernel
from test_stage_geometries_gpu import FORM_XYZZ, host_call, pool, run_case  # noqa: F401  (pool: the shared fixture)
from webgpu_msm_bls12_377_amd.host.engine import EGLVRANGE

pytestmark = pytest.mark.gpu

N = 3000
LANES = [0, 1, 63, 64, 255, 256, 2999] + list(range(300, 2900, 7))  # where crafted scalars go, in this order
LAM, r = GC.LAM, R.R_ORDER
G = M.glv8()


@pytest.fixture
def glv(engine):
    engine.set_g1_form("weierstrass")
    engine.set_glv(True)
    yield engine
    engine.set_glv("auto")
    engine.set_g1_form("edwards")


def plant(seed, crafted):
    """(scalars, other scalars): random below r, the crafted ones on LANES."""
    assert len(crafted) <= len(LANES)
    ks, other = R.rand_scalars(seed, N), R.rand_scalars(seed + 1, N)
    for lane, k in zip(LANES, crafted):
        ks[lane] = k
    return ks, other


def expected(oracle, pts, ks):
    """The oracle's sum over the scalars below r, plus pyref's [k] P of every lane whose scalar is not (legal: below the
    edge of the GLV range k may exceed r)."""
    big = [i for i, k in enumerate(ks) if k >= r]
    rest = [0 if k >= r else k for k in ks]
    acc = R.decode_result(util.oracle_msm(oracle, pts, R.encode_scalars(rest)))
    pl = R.decode_points(pts[: 96 * (max(big) + 1)]) if big else []
    for i in big:
        acc = R.add(acc, R.mul(pl[i], ks[i]))
    return R.encode_result(acc)


def lambda_multiples():
    rnd = GC.rng("gpu-multiples")
    ms = [1, 2, LAM - 1, LAM, 1 << 32, 1 << 64, (1 << 96) + (1 << 64), 0xFFFFFFFF, (5 << 32) | 0xFFFFFFFF] + [rnd.randrange(1, LAM) for _ in range(12)]
    ks = [m * LAM for m in ms]
    assert LAM * LAM == r - LAM - 1 and all(0 < k < r for k in ks)
    return ks + [k + 1 for k in ks] + [k - 1 for k in ks]


def test_multiples_of_lambda_take_the_correction_arm(glv, oracle, pool):
    """k = lambda, 2 lambda, (lambda - 1) lambda, lambda^2 = r - lambda - 1, m lambda for m = 2^32, 2^64 and 2^96 + 2^64
    (the increment of q = m - 1 carries across one, two and two words), for m with a low word of all ones and for random
    m, each with k + 1 and k - 1 beside it: the k1 half of a multiple is all zeros (key 0: in no bucket), its k2 half is m."""
    crafted = lambda_multiples()
    ks, other = plant(0x1A3B, crafted)
    for k in crafted[: len(crafted) // 3]:
        rec = M.recode(k, G)
        assert rec.digits[:8] == [0] * 8 and M.rebuild(rec.digits, G) == k and rec.flags == 0
        up, down = M.recode(k + 1, G), M.recode(k - 1, G)  # the neighbours: k1 = 1 with the same k2, k1 = lambda - 1 with k2 - 1
        assert up.digits == [1] + [0] * 7 + rec.digits[8:] and k + 1 in crafted
        assert down.digits[:8] == M.recode(LAM - 1, G).digits[:8] and M.rebuild(down.digits, G) == k - 1 and k - 1 in crafted
    pts = pool[: 96 * N]
    run_case(glv, host_call(glv, pts), G, ks, pts, FORM_XYZZ, range(8), other, expected(oracle, pts, ks), label="glv multiples of lambda")


def test_lambda_and_its_square_are_the_endomorphism(glv, pool):
    """The closed form, independent of oracle and model: [lambda] P = (beta x, y) and [lambda^2] P = phi(phi(P)), one
    point per call, on the GLV geometry."""
    pl = R.decode_points(pool[: 96 * 3])
    for i, p in enumerate(pl):
        wire = pool[96 * i : 96 * i + 96]
        assert glv.msm(wire, R.encode_scalars([LAM])) == R.encode_result(M.phi(p)), i
        assert glv.last_geometry() == (8, 15)
        assert glv.msm(wire, R.encode_scalars([LAM * LAM])) == R.encode_result(M.phi(M.phi(p))), i
        assert glv.msm(wire, R.encode_scalars([LAM + 1])) == R.encode_result(R.add(p, M.phi(p))), i
    assert R.add(R.add(pl[0], M.phi(pl[0])), M.phi(M.phi(pl[0]))) is None  # 1 + lambda + lambda^2 = 0 mod r


def test_every_scalar_a_multiple_of_lambda(glv, oracle, pool):
    """Every k1 is zero: in all 8 slots the first n columns hold key 0 and sit in no bucket; the call is the k2 half alone."""
    rnd = GC.rng("gpu-all-multiples")
    ks = [rnd.randrange(1, LAM) * LAM for _ in range(N)]
    other = R.rand_scalars(0x1A3D, N)
    cols, _ = M.digit_matrix(ks, G)
    assert all((c[:N] == 1 << 15).all() for c in cols)
    pts = pool[: 96 * N]
    run_case(glv, host_call(glv, pts), G, ks, pts, FORM_XYZZ, range(8), other, expected(oracle, pts, ks), label="glv all multiples")


def test_boundary_digits_in_every_window_of_both_halves(glv, oracle, pool):
    """0, +1, -1, 2^15 - 1 and -2^15 in each of the 16 digit positions, as far as a position can hold them (the top digit of
    a half stays non-negative, and k1 < lambda keeps its top digit below 2^15 - 1): k = k1 + lambda k2 built from the
    digits of its halves (glv_cases.boundary_digits), the model asked whether the digit is where it was put.  Such a k may
    exceed r: legal below the edge of the range; those lanes' share of the result comes from pyref."""
    cases = GC.boundary_digits(GC.rng("gpu-boundaries"))
    assert len(cases) == 16 * 5 - 2 * 2 - 1  # (-1 and -2^15 in neither top position, 2^15 - 1 not in k1's)
    for k, pos, d in cases:
        rec = M.recode(k, G)
        assert rec.flags == 0 and rec.digits[pos] == d, (hex(k), pos, d)
    ks, other = plant(0x1A3F, [k for k, _, _ in cases])
    assert any(k >= r for k in ks)
    pts = pool[: 96 * N]
    run_case(glv, host_call(glv, pts), G, ks, pts, FORM_XYZZ, range(8), other, expected(oracle, pts, ks), label="glv boundary digits")


def edge_scalars():
    """Both sides of the edge, from the model: EDGE (k1 = lambda - 1, k2 = 0x7FFF in every window) is the largest scalar
    that splits, EDGE_CARRIED its variant whose window 6 carries into window 7, BEYOND = EDGE + 1 the first that does not."""
    assert M.recode(GC.EDGE, G).flags == 0 and M.recode(GC.EDGE_CARRIED, G).flags == 0
    assert M.recode(GC.EDGE_CARRIED, G).digits[8:] == [-1] + [0] * 6 + [0x7FFF]  # top limb 0x7FFE + the carry
    assert M.recode(GC.BEYOND, G).flags == M.ERR_GLV_RANGE and M.recode(GC.BEYOND, M.equal16()).flags == 0
    return GC.EDGE, GC.EDGE_CARRIED, GC.BEYOND


def test_the_largest_scalars_that_split_do_not_rerun(glv, oracle, pool):
    edge, carried, _ = edge_scalars()
    ks, other = plant(0x1A41, [edge, carried, edge - 1, 0, carried, 1, edge])
    pts = pool[: 96 * N]
    run_case(glv, host_call(glv, pts), G, ks, pts, FORM_XYZZ, range(8), other, expected(oracle, pts, ks), label="glv range edge, inside")


def test_the_smallest_scalar_that_does_not_split_reruns_once(glv, oracle, pool):
    """EDGE + 1 on one lane: the GLV pass is discarded, the call reruns ONCE, the read-back describes sixteen plain windows."""
    edge, _, beyond = edge_scalars()
    g16 = M.equal16()
    ks, other = plant(0x1A43, [edge, 1, 2, 3, beyond])
    pts = pool[: 96 * N]
    run_case(glv, host_call(glv, pts), g16, ks, pts, FORM_XYZZ, range(16), other, expected(oracle, pts, ks), reruns=1, label="glv range edge, beyond")


def test_the_range_edge_through_window_partials(glv, oracle, pool):
    """The same pair through the window-partials call under GLV: EDGE passes, EDGE + 1 is MSM377_EGLVRANGE in every shard."""
    from webgpu_msm_bls12_377_amd.host.engine import combine_partials_bytes

    edge, carried, beyond = edge_scalars()
    n = 500
    pts = pool[: 96 * n]
    ks = R.rand_scalars(0x1A45, n)
    ks[0], ks[64], ks[499] = edge, carried, LAM
    d_p, d_s = dev(pts), dev(R.encode_scalars(ks))
    parts = [glv.glv_window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, b, c) for b, c in ((0, 3), (3, 5))]
    assert combine_partials_bytes(b"".join(parts), 8) == expected(oracle, pts, ks)
    ks[255] = beyond
    d_s = dev(R.encode_scalars(ks))
    for b, c in ((0, 8), (7, 1)):
        with pytest.raises(msm.MsmError) as e:
            glv.glv_window_partials_device(d_p.data_ptr(), d_s.data_ptr(), n, b, c)
        assert e.value.code == EGLVRANGE


def test_the_range_edge_inside_a_fixed_base_batch(glv, oracle, pool):
    """The same pair as one element of msm_fixed_base_batch_device over a GLV table, in either half of a batch of 5: the call
    gives elements 0 .. 2 to the caller's context and elements 3, 4 to its twin (batches of four and more), and each share
    reruns its own out-of-range elements plain, after its others.  Every element's result is right; last_geometry() is the
    caller's context's: it ends on the plain rerun (sixteen windows) when element 1 holds EDGE + 1, and on the GLV geometry
    when element 4 does -- the twin's share reran that element, the caller's share reran nothing -- or when no element does."""
    edge, carried, beyond = edge_scalars()
    pts = pool[: 96 * N]
    sets = [R.rand_scalars(0x1A50 + b, N) for b in range(5)]
    for b in range(5):
        sets[b][64 * b], sets[b][2999 - b] = edge, carried
    want = [expected(oracle, pts, ks) for ks in sets]
    glv.set_bases(pts)
    try:
        d_s = dev(b"".join(R.encode_scalars(ks) for ks in sets))
        assert glv.msm_fixed_base_batch_device(d_s.data_ptr(), N, 5) == want
        assert glv.last_geometry() == (8, 15)
        for b in (1, 4):
            with_beyond = [list(ks) for ks in sets]
            with_beyond[b][255] = beyond
            want_b = list(want)
            want_b[b] = expected(oracle, pts, with_beyond[b])
            d_s = dev(b"".join(R.encode_scalars(ks) for ks in with_beyond))
            assert glv.msm_fixed_base_batch_device(d_s.data_ptr(), N, 5) == want_b, b
            assert glv.last_geometry() == ((16, 15) if b == 1 else (8, 15)), b
        d_s = dev(b"".join(R.encode_scalars(ks) for ks in sets))
        assert glv.msm_fixed_base_batch_device(d_s.data_ptr(), N, 5) == want  # the table is still the GLV one
        assert glv.last_geometry() == (8, 15)
    finally:
        glv.msm(pts[:96], R.encode_scalars([1]))  # drops the resident table


# ---- relations across the two halves: entry i adds P_i under k1's digits, entry n + i adds phi(P_i) under k2's ----
RELATION_WINDOW = 3


def relation_case(pool):
    """(points, scalars, other, {case: (key, row)}): in window 3, from the model --
    (a) phi(P_10) from the k2 half of lane 10 and P_20 = phi(P_10) from the k1 half of lane 20, equal signs: a doubling;
    (b) phi(P_30) and P_40 = phi(P_30) with opposite signs: the identity from two entries;
    (c) P_50 and phi(P_50) from both halves of lane 50, phi(phi(P_50)) from the k2 half of lane 60 (P_60 = phi(P_50)): the
        identity from three distinct points.
    Each in a bucket of its own that no other entry shares, low enough to be among the buckets check_slot decodes."""
    rnd = GC.rng("gpu-relations")
    pl = R.decode_points(pool[: 96 * N])
    pl[20], pl[40], pl[60] = M.phi(pl[10]), M.phi(pl[30]), M.phi(pl[50])
    ks, other = R.rand_scalars(0x1A60, N), R.rand_scalars(0x1A61, N)
    w = RELATION_WINDOW
    base_cols, _ = M.digit_matrix(ks, G)
    used = set(int(x) for x in M.keys_and_signs(base_cols[w], 1 << 15, False)[0])
    da, db, dc = [d for d in range(40, 2000) if d not in used][:3]
    k1_with = lambda d: GC.half_with_digit(rnd, w, d, LAM)  # noqa: E731
    k2_with = lambda d: GC.half_with_digit(rnd, w, d, GC.HALF_MAX + 1)  # noqa: E731
    ks[10] = rnd.randrange(LAM) + LAM * k2_with(da)
    ks[20] = k1_with(da) + LAM * rnd.getrandbits(126)
    ks[30] = rnd.randrange(LAM) + LAM * k2_with(db)
    ks[40] = k1_with(-db) + LAM * rnd.getrandbits(126)
    ks[50] = k1_with(dc) + LAM * k2_with(dc)
    ks[60] = rnd.randrange(LAM) + LAM * k2_with(dc)
    rows = {"a": (da, [(20, 0), (N + 10, 0)]), "b": (db, [(40, 1), (N + 30, 0)]), "c": (dc, [(50, 0), (N + 50, 0), (N + 60, 0)])}
    return pl, ks, other, rows


def test_a_point_meets_its_own_endomorphism_in_one_bucket(glv, oracle, pool):
    """P_j = phi(P_i) is a legal input under the GLV promise (on the curve and in the subgroup whenever P_i is).  Then entry
    n + i and entry j add the SAME point: a bucket of window 3 doubles (a), cancels to the identity (b), or holds P, phi(P)
    and phi^2(P), which sum to the identity (c) -- the equal-operand and opposite-operand exits of the XYZZ additions of
    k_accumulate<G1Dev>.  The model says which bucket and what it must hold; no fallback is expected (run_case asserts
    it): the Weierstrass path handles these itself."""
    pl, ks, other, rows = relation_case(pool)
    cols, flags = M.digit_matrix(ks, G)
    assert flags == 0
    c = M.csr(cols[RELATION_WINDOW], 15, 1 << 15)
    multi = [k for k in range(1, (1 << 15) + 1) if c.counts[k] >= 2]
    for name, (key, row) in rows.items():
        assert c.row(key) == sorted(row), (name, key, c.row(key))  # exactly these entries, with these signs
        assert multi.index(key) < 300, (name, "not among the buckets that are decoded")
        total = M.bucket_sum(pl, c.row(key), G, N)
        assert total == (R.add(pl[20], pl[20]) if name == "a" else None), name
    pts = R.encode_points(pl)
    run_case(glv, host_call(glv, pts), G, ks, pts, FORM_XYZZ, range(8), other, expected(oracle, pts, ks), label="glv relations across the halves")


MERGE_SEG = 17  # odd: S entries of +X and S of -X in two work items of S leave partial sums (2 p - S) X and -(2 p - S) X, never O and O


def merge_case(pool):
    """(points, scalars, other, {case: (key, row)}): two rows of 2 S = 34 entries in window 3, each cut into two work items
    of S = 17 under MSM377_SEG_GLV=17 --
    (a) S lanes of P (their k2 halves add phi(P)) and S lanes of phi(P) itself (k1 halves), equal signs: whichever entries
        an item gets, its partial sum is [17] phi(P), and the merge adds two EQUAL partial sums;
    (b) the same with opposite signs: the items' partial sums are X and -X with X != O (S is odd), and the merge adds them."""
    rnd = GC.rng("gpu-merge")
    S, w = MERGE_SEG, RELATION_WINDOW
    pl = R.decode_points(pool[: 96 * N])
    ks, other = R.rand_scalars(0x1A90, N), R.rand_scalars(0x1A91, N)
    base_cols, _ = M.digit_matrix(ks, G)
    used = set(int(x) for x in M.keys_and_signs(base_cols[w], 1 << 15, False)[0])
    da, db = [d for d in range(40, 2000) if d not in used][:2]
    rows = {}
    for name, d, sign, at in (("a", da, 0, 100), ("b", db, 1, 500)):
        for j in range(S):
            pl[at + j] = pl[at]
            pl[at + 200 + j] = M.phi(pl[at])
            ks[at + j] = rnd.randrange(LAM) + LAM * GC.half_with_digit(rnd, w, d, GC.HALF_MAX + 1)
            ks[at + 200 + j] = GC.half_with_digit(rnd, w, -d if sign else d, LAM) + LAM * rnd.getrandbits(126)
        rows[name] = (d, [(at + 200 + j, sign) for j in range(S)] + [(N + at + j, 0) for j in range(S)])
    return pl, ks, other, rows


def test_a_point_meets_its_own_endomorphism_at_the_split_row_merge(oracle, pool):
    """The same pairs where a split row is merged (g1_add_quad in k_merge_split_rows_quad): a fresh context with
    MSM377_SEG_GLV=17, rows of 34 entries in two work items.  The work list read back after the call says that it ran with
    work items of 17 and that exactly these two rows were split, two items each.  No fallback (run_case asserts it)."""
    S = MERGE_SEG
    pl, ks, other, rows = merge_case(pool)
    cols, flags = M.digit_matrix(ks, G)
    assert flags == 0 and tuple(M.row_split(2 * S, S)) == (2, S, S)
    c = M.csr(cols[RELATION_WINDOW], 15, 1 << 15)
    multi = [k for k in range(1, (1 << 15) + 1) if c.counts[k] >= 2]
    for name, (key, row) in rows.items():
        assert c.row(key) == sorted(row) and multi.index(key) < 300, (name, key)
        assert M.bucket_sum(pl, c.row(key), G, N) == (R.mul(M.phi(pl[100]), 2 * S) if name == "a" else None), name
    wl = M.work_list(W.row_lengths(G, cols), S)
    want_split = sorted((RELATION_WINDOW << 15) + key - 1 for key, _ in rows.values())  # row = slot 2^15 + bucket index
    assert wl.split_rows == want_split and wl.overflow_slots == 2  # no other row of the call splits; one overflow partial each
    pts = R.encode_points(pl)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_SEG_GLV", str(S))
        eng = msm.MsmEngine(1 << 12)
    try:
        eng.set_g1_form("weierstrass")
        eng.set_glv(True)
        seen = []

        def call(kk):  # (the work list answers while the capture of run_case is on)
            out = eng.msm(pts, R.encode_scalars(kk))
            seen.append(eng.read_work_list())
            return out

        run_case(eng, call, G, ks, pts, FORM_XYZZ, range(8), other, expected(oracle, pts, ks), label="glv split-row merge")
        info, got = seen[-1]
        assert (info.seg, info.split_rows, info.overflow_slots) == (S, 2, 2), info[:8]
        assert sorted(int(x) for x in got["split_rows"]) == want_split
        items = {(int(row), int(seg)) for row, seg in got["items"]}
        assert {(row, seg) for row in want_split for seg in (0, 1)} <= items and not any((row, 2) in items for row in want_split)
    finally:
        eng.close()


def cross_ladders(kind):
    """Calls of two points, P and Q = phi(P) ("same") or -phi(P) ("negative"), and two scalars: lane 0 has digits in its k2
    half only (entry n + 0 adds phi(P)), lane 1 in its k1 half only (entry 1 adds Q).  In window w the two are the only
    entries, at bucket indices 0 and 2^15 >> (r + 1): they first meet at level r of the window's tree, a different level
    in every window, every level 0 .. 14 over the calls."""
    L, cases, todo = 15, [], list(range(15))
    pts = C.Points("glv cross ladder/" + kind)
    a = pts.new()
    b = pts.add_log(LAM * pts.logs[a] if kind == "same" else -LAM * pts.logs[a])
    assert pts.points[b] == (M.phi(pts.points[a]) if kind == "same" else R.neg(M.phi(pts.points[a])))
    while todo:
        free, first, second, occupied, meet = list(range(8)), {}, {}, {}, {}
        for r, (x, y, where) in C.ladder_pairs(L, todo).items():
            for w in free:
                if C.scalar_from_digits(G, {8 + w: x + 1}) is not None and C.scalar_from_digits(G, {w: y + 1}) is not None:
                    free.remove(w)
                    first[8 + w], second[w], occupied[w], meet[w] = x + 1, y + 1, {x, y}, where
                    break
        assert first, todo
        ks = [C.scalar_from_digits(G, first), C.scalar_from_digits(G, second)]
        assert None not in ks
        case = C.Case("cross ladder %s levels %s" % (kind, sorted(r for ms in meet.values() for r, _ in ms)), G, ks,
                      [pts.points[a], pts.points[b]], [pts.logs[a], pts.logs[b]], occupied, meet)
        cases.append(case)
        todo = [r for r in todo if r not in C.levels_in(case)]
    return cases


@pytest.mark.parametrize("kind", ["same", "negative"])
def test_a_point_meets_its_own_endomorphism_in_the_tree(engine, kind):
    """phi(P) from the k2 half and Q = +-phi(P) from the k1 half alone in two buckets of a window: the tree's first addition
    of the two is a doubling or a cancellation, at every level -- levels of the column launches and of the tail, as the
    read-back's schedule says.  Placement from the model (stage_model.csr, stage_model.meetings); every point of every
    window record against the model, then the result; no fallback (run_records asserts it)."""
    route, kernels, levels = ROUTES["glv"], set(), set()
    cases = cross_ladders(kind)
    for case in cases:
        cols, flags = M.digit_matrix(case.scalars, G)
        assert flags == 0
        for w in range(8):
            c = M.csr(cols[w], 15, 1 << 15)
            if w not in case.occupied:
                assert int(c.counts[1:].sum()) == 0, (case.name, w)
                continue
            x, y = sorted(case.occupied[w])
            assert c.row(x + 1) == [(2, 0)] and c.row(y + 1) == [(1, 0)] and int(c.counts[1:].sum()) == 2, (case.name, w)
            assert M.meetings(x, y, 15) == case.meet[w], (case.name, w)
    with on_route(engine, route) as call:
        for case in cases:
            info = run_records(engine, call, route, case)
            kernels |= {which_kernel(info, lv) for lv in C.levels_in(case)}
            levels |= set(C.levels_in(case))
    assert levels == set(range(15)) and kernels == {"k_tree_columns", "k_reduce_tail_lds"}, (levels, kernels)


# ---- routes of a GLV table and of a GLV upload ----
def test_a_glv_table_serves_short_prefix_and_full_calls(glv, oracle, pool):
    """set_bases under GLV, then: a short fixed-base call (64-bit and 128-bit scalars: the table serves through its plain
    half) against the full-width call on the zero-extended scalars and the oracle; msm_fixed_base on a prefix of 100 and
    of n - 1 bases (sixteen plain windows over records 0 .. n - 1); the full n again on the 8 GLV windows.  The table
    survives all of it."""
    pts = pool[: 96 * N]
    glv.set_bases(pts)
    try:
        full = R.rand_scalars(0x1A70, N)
        want_full = expected(oracle, pts, full)
        assert glv.msm_fixed_base(R.encode_scalars(full)) == want_full and glv.last_geometry() == (8, 15)
        rnd = GC.rng("gpu-short")
        for sbytes, bits in ((8, 64), (16, 128)):
            short = [rnd.getrandbits(bits) for _ in range(N)]
            short[0], short[1], short[N - 1] = (1 << bits) - 1, 0, 1 << (bits - 1)
            d_s = dev(b"".join(k.to_bytes(sbytes, "little") for k in short))
            got = glv.msm_fixed_base_short_device(d_s.data_ptr(), N, sbytes, bits)
            assert got == expected(oracle, pts, short), bits
            assert glv.msm_fixed_base(R.encode_scalars(short)) == got and glv.last_geometry() == (8, 15), bits
        for m in (100, N - 1):
            assert glv.msm_fixed_base(R.encode_scalars(full[:m])) == expected(oracle, pts[: 96 * m], full[:m]), m
            assert glv.last_geometry() == (16, 15), m
        assert glv.msm_fixed_base(R.encode_scalars(full)) == want_full and glv.last_geometry() == (8, 15)
    finally:
        glv.msm(pts[:96], R.encode_scalars([1]))  # drops the resident table


def test_a_chunked_host_upload_stays_whole_under_glv(oracle, pool):
    """MSM377_UPLOAD_CHUNK_MIN=100 on a fresh context: a host-buffer GLV call above the threshold is not cut into chunks
    (the phi half is made from the whole upload); the result is the oracle's, the geometry the GLV one."""
    n = 2049
    pts, ks = pool[: 96 * n], R.rand_scalars(0x1A80, n)
    ks[0], ks[1], ks[n - 1] = LAM, 2 * LAM, GC.EDGE
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM377_UPLOAD_CHUNK_MIN", "100")
        eng = msm.MsmEngine(1 << 12)
    try:
        eng.set_g1_form("weierstrass")
        eng.set_glv(True)
        assert eng.msm(pts, R.encode_scalars(ks)) == expected(oracle, pts, ks)
        assert eng.last_geometry() == (8, 15)
    finally:
        eng.close()


def test_glv_with_the_native_input_forms(glv, golden, pool):
    """Montgomery points, infinity flags and Montgomery scalars in front of k_decompose_glv: the goldens, and Montgomery
    scalars that decode to lambda and to 2 lambda (closed form: phi(P_0) + [2] phi(P_1) + P_2)."""
    pl = R.decode_points(pool[: 96 * 3])
    want = R.encode_result(R.add(R.add(M.phi(pl[0]), R.mul(M.phi(pl[1]), 2)), pl[2]))
    try:
        for pform, sform in (("mont_flag", "mont"), ("mont", "mont"), ("wire", "mont"), ("mont", "wire")):
            glv.set_input_format(pform, sform)
            for name, case in sorted(golden.items()):
                if name.startswith("g1_"):
                    pb = msm.encode_points_native(R.decode_points(case["points"]), pform)
                    sb = msm.encode_scalars_native(R.decode_scalars(case["scalars"]), sform)
                    assert glv.msm(pb, sb) == case["expected"], (name, pform, sform)
            pb, sb = msm.encode_points_native(pl, pform), msm.encode_scalars_native([LAM, 2 * LAM, 1], sform)
            assert glv.msm(pb, sb) == want, (pform, sform)
            assert glv.last_geometry() == (8, 15)
    finally:
        glv.set_input_format("wire", "wire")
