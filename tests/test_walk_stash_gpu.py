"""What the six walk kernels of the batch calls leave in the stash -- k_bm_accumulate, k_bmm_accumulate, k_cr_accumulate /
k_cr_fold, k_bmv_table / k_bmv_accumulate, k_bl2_accumulate, k_edbm_accumulate -- read back through msm377_read_walk_stash
and msm377_g1_read_walk_tables and held against tests/walk_model.py: the stash contract of tools/check_lazy_bounds.py
(NORMALISATION_OPERANDS) that tests/test_normalise_gpu.py takes its corner operands from, the identity form, the invariant,
the running products of k_bm_up / k_edbm_up on a real call, and the value of every point.  Values are bit exact or exact
residues.  The cases, their crafted lanes and the events they promise are tests/walk_cases.py; tests/test_walk_model_host.py
asserts every promise on the CPU and run_case repeats it before anything is launched.

Every case checks the whole last pass, stash first: box, identity form, invariant, running products, then the tie to the
call's own output records; then the outputs against the host twin; then the crafted lanes and at most 300 further scalar
multiplications against pyref.  A failing stash assertion says whether the output bytes were right.
tests/STAGES.md lists the seeded faults this file was run against.  Every test leaves the engine at width 0 and (wire, wire)."""
import contextlib
import random

import numpy as np
import pytest

import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import commit_rows_vectors as CR
import ed_batch_mul_vectors as EV
import pyref as R
import walk_cases as WC
import walk_model as WM
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import engine as E

pytestmark = pytest.mark.gpu

r = R.R_ORDER
MODEL_CAP = 300  # further scalar multiplications by pyref per case, beside the crafted lanes
KIND = {"batch_mul": E.WALK_BATCH_MUL, "multi": E.WALK_BATCH_MUL_MULTI, "commit": E.WALK_COMMIT_ROWS, "var": E.WALK_BATCH_MUL_VAR, "lincomb2": E.WALK_BATCH_LINCOMB2,
        "ed": E.WALK_ED_BATCH_MUL_MULTI}


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf) if buf else bytearray(16), dtype=torch.uint8).cuda()


def poisoned(nbytes):
    import torch

    return torch.full((max(16, nbytes),), 0xEE, dtype=torch.uint8, device="cuda")


@contextlib.contextmanager
def settings(engine, width=0, points="wire", scalars="wire"):
    engine.set_mul_window(width)
    engine.set_input_format(points, scalars)
    try:
        yield
    finally:
        engine.set_mul_window(0)
        engine.set_input_format("wire", "wire")


def code_of(call, *args, **kw):
    with pytest.raises(msm.MsmError) as e:
        call(*args, **kw)
    return e.value.code


def ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------ the calls ----

def point_records(points, form):
    """Device records of a list of points (None: a flagged input, mont_flag only)."""
    flagged = [i for i, pt in enumerate(points) if pt is None]
    pts = [R.G if pt is None else pt for pt in points]
    if form == "wire":
        assert not flagged
        return R.encode_points(pts)
    return VV.mont_records(pts, flag=form == "mont_flag", flagged=flagged)


def scalar_bytes(case, column=None):
    rows = case.get("device_rows", case["rows"])
    if column is None:
        return b"".join(R.encode_scalars(list(row)) for row in rows)
    return R.encode_scalars([row[column] for row in rows])


def launch(engine, case):
    """One device call of the case on poisoned outputs: (records, flag bytes or None, twin records, twin flags)."""
    n, call = case["n"], case["call"]
    rec = 64 if call == "ed" else 96
    d_out, d_inf = poisoned(rec * n), poisoned(n)
    if call == "batch_mul":
        base = V.base_bytes(case["bases"][0])
        d_s = dev(scalar_bytes(case))
        with settings(engine, case["c"], scalars=case["scalar_form"]):
            engine.batch_mul_device(base, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
        twin = msm.batch_mul_host(base, b"".join(R.encode_scalars(list(row)) for row in case["rows"]))
    elif call == "multi":
        bases = R.encode_points(list(case["bases"]))
        buf, out_stride, base_stride = WC.MV.pack(case["rows"], case["layout"])
        d_s = dev(buf)
        with settings(engine, case["c"]):
            engine.batch_mul_multi_device(bases, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), "wire", out_stride, base_stride)
        twin = msm.batch_mul_multi_host(bases, buf, "wire", case["layout"])
    elif call == "commit":
        k = len(case["bases"])
        d_s = dev(scalar_bytes(case))
        engine.commit_rows_device(d_s.data_ptr(), n, k, d_out.data_ptr(), d_inf.data_ptr())
        if k <= 48:  # the product's host twin; and where the generators' logarithms are known, the closed form beside it
            twin = msm.commit_rows_host(case["gens"], scalar_bytes(case))
            assert not case.get("logs") or twin == CR.closed_rows(case["logs"], case["rows"])
        else:  # k = 257: the closed form [sum_j s_ij g_j]G alone (one multiplication per row where the twin makes 257)
            twin = CR.closed_rows(case["logs"], case["rows"])
    elif call == "var":
        pts = point_records([p for p, in case["points"]], case["point_form"])
        sb = R.encode_scalars([case["rows"][0][0]]) if case["stride"] == 0 else scalar_bytes(case)
        d_p, d_s = dev(pts), dev(sb)
        with settings(engine, 0, points=case["point_form"]):
            engine.batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), "wire", case["stride"])
        twin = msm.batch_mul_var_host(pts, sb, "wire", case["point_form"])
    elif call == "lincomb2":
        form = case["point_form"]
        p, q = point_records([x[0] for x in case["points"]], form), point_records([x[1] for x in case["points"]], form)
        a = R.encode_scalars([case["rows"][0][0]]) if case["a_stride"] == 0 else scalar_bytes(case, 0)
        b = R.encode_scalars([case["rows"][0][1]]) if case["b_stride"] == 0 else scalar_bytes(case, 1)
        d_p, d_q, d_a, d_b = dev(p), dev(q), dev(a), dev(b)
        if case["in_place"]:
            d_out = d_p  # wire in, wire out: records of equal size
        with settings(engine, 0, points=form):
            engine.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), "wire", case["a_stride"], case["b_stride"])
        twin = msm.batch_lincomb2_host(p, q, a, b, "wire", form)
    else:
        bases = EV.bases_bytes(case["bases"])
        d_s = dev(scalar_bytes(case))
        with settings(engine, case["c"]):
            engine.ed_batch_mul_multi_device(bases, d_s.data_ptr(), n, d_out.data_ptr())
        twin = (msm.ed_batch_mul_multi_host(bases, scalar_bytes(case)), None)
    out = bytes(d_out.cpu().numpy()[: rec * n])
    flags = None if call == "ed" else bytes(d_inf.cpu().numpy()[:n])
    return out, flags, twin[0], twin[1]


# ------------------------------------------------------------------ the checks ----

def encode(call, pt):
    return R.ed_encode_result(pt) if call == "ed" else R.encode_result(pt)


def check_pass(engine, case, out, flags, twin, twin_flags, offset=0, m=None, k=None, segments=1, stride=0, out_first=0):
    """The stash of the last pass against the contract and the call's own outputs (out, flags, twin: outputs out_first and
    up of the call).  Returns the decoded points of the pass."""
    call, n = case["call"], case["n"]
    m = n if m is None else m
    rec = 64 if call == "ed" else 96
    outputs_right = out == twin and (flags is None or flags == twin_flags)
    verdict = "  [the call's output bytes were %s]" % ("right" if outputs_right else "WRONG")
    info, pts, prod = engine.read_walk_stash()
    ed = call == "ed"
    want = dict(kind=KIND[call], form=E.WALK_FORM_ED if ed else E.WALK_FORM_XYZZ, point_words=36 if ed else 52, product_words=9 if ed else 13, product_pad=3, n=n,
                pass_offset=offset, m=m, width=case["c"], k=k if k is not None else (len(case["bases"]) if case["bases"] else len(case["points"][0])), segments=segments, stride=stride)
    assert info._asdict() == want, (info, want)
    assert pts.shape == (m, want["point_words"]) and prod.shape == (m, want["product_words"] + 3)
    where = "%s/%s: " % (call, case["name"])
    try:
        decoded = (WM.check_ed_stash if ed else WM.check_g1_stash)(pts, where)
        WM.check_products("Fq" if ed else "Fp", pts, prod, where)
        for i, pt in enumerate(decoded):  # the tie: the normalisation's record is this point, every one of the pass
            o = offset + i - out_first
            if encode(call, pt) != out[rec * o : rec * o + rec] or (flags is not None and flags[o] != (1 if pt is None else 0)):
                raise AssertionError("%sstash point %d decodes to %s, output %d of the call holds %s (flag %s)" % (where, i, pt, offset + i, out[rec * o : rec * o + rec].hex(), flags and flags[o]))
    except AssertionError as e:
        raise AssertionError(str(e) + verdict) from None
    return decoded


def compare_outputs(case, out, flags, twin, twin_flags):
    rec = 64 if case["call"] == "ed" else 96
    if out != twin:
        bad = [i for i in range(case["n"]) if out[rec * i : rec * i + rec] != twin[rec * i : rec * i + rec]]
        raise AssertionError("%s/%s: %d outputs differ from the host twin, first %d" % (case["call"], case["name"], len(bad), bad[0]))
    assert flags is None or flags == twin_flags, "flag bytes differ from the host twin"


def compare_model(case, decoded, offset=0):
    """Every crafted lane, and further lanes up to MODEL_CAP scalar multiplications, against walk_model / pyref."""
    call = case["call"]
    terms = 1 if case.get("logs") else len(case["rows"][case["crafted"][0]])
    others = [i for i in range(offset, offset + len(decoded)) if i not in set(case["crafted"])]
    random.Random(case["name"]).shuffle(others)
    lanes = [i for i in case["crafted"] if offset <= i < offset + len(decoded)] + others[: MODEL_CAP // terms]
    for i in lanes:
        exp = WC.expected_point(case, i)
        assert decoded[i - offset] == exp, "%s/%s: lane %d: the stash holds %s, the model %s" % (call, case["name"], i, decoded[i - offset], exp)
    return len(lanes)


def run_case(engine, case, **layout):
    got = WC.events_of(case)
    assert case["promises"] <= got, sorted(case["promises"] - got)  # before anything runs on the GPU
    out, flags, twin, twin_flags = launch(engine, case)
    decoded = check_pass(engine, case, out, flags, twin, twin_flags, **layout)
    compare_outputs(case, out, flags, twin, twin_flags)
    lanes = compare_model(case, decoded)
    print("%s/%s: n = %d, %d stash points checked, %d against pyref" % (case["call"], case["name"], case["n"], len(decoded), lanes))
    return decoded


# ------------------------------------------------------------------ the cases ----

@pytest.mark.parametrize("case", WC.batch_mul_cases(), ids=ids(WC.batch_mul_cases()))
def test_batch_mul(engine, case):
    run_case(engine, case, k=1)
    assert code_of(engine.read_walk_tables) == E.ESTATE  # no per-point tables behind a fixed-base call


@pytest.mark.parametrize("case", WC.multi_cases(), ids=ids(WC.multi_cases()))
def test_batch_mul_multi(engine, case):
    decoded = run_case(engine, case)
    if case.get("cancels"):  # an output of O with no term O
        hit = [i for i in case["crafted"] if decoded[i] is None and all(R.mul(b, s) is not None for b, s in zip(case["bases"], case["rows"][i]))]
        assert hit, "no crafted lane sums to O from two terms that are not O"


@pytest.fixture(scope="module")
def generator_sets(engine):
    """One resident set at a time: the set of the case, built when the case before it used another."""
    state = {"gens": None}

    def use(gens):
        if state["gens"] != gens:
            engine.set_generators(gens, 8)
            state["gens"] = gens

    yield use
    engine.set_generators(None)


@pytest.mark.parametrize("case", WC.commit_cases(), ids=ids(WC.commit_cases()))
def test_commit_rows(engine, generator_sets, case):
    generator_sets(case["gens"])
    k, n = len(case["bases"]), case["n"]
    segs = WC.segments_of(k)
    assert (len(segs), segs[0][1]) == msm.commit_rows_plan(k)[:2]
    stride = -(-n // 256) * 256
    run_case(engine, case, segments=len(segs), stride=stride)  # segment 0: the fold, against the whole row
    if case["name"].startswith("relations"):
        assert set(WC.FOLD_EVENTS) <= WC.fold_events(case)
    for g in range(1, len(segs)):  # the partial sums k_cr_fold read and left
        j0, j1 = segs[g]
        _, pts, prod = engine.read_walk_stash(segment=g)
        assert prod is None and pts.shape == (n, 52)
        decoded = WM.check_g1_stash(pts, "commit/%s, segment %d: " % (case["name"], g))
        if case.get("logs"):
            wire, _ = CR.multiples_of_g([sum(s * lg for s, lg in zip(row[j0:j1], case["logs"][j0:j1])) for row in case["rows"]])
            bad = [i for i in range(n) if R.encode_result(decoded[i]) != wire[96 * i : 96 * i + 96]]
            assert not bad, "segment %d: the partial sums of rows %s differ from the sum over generators %d .. %d" % (g, bad[:4], j0, j1 - 1)
        for i in case["crafted"]:
            assert decoded[i] == WC.commit_partial(case, i, j0, j1), "segment %d, row %d" % (g, i)
    assert code_of(engine.read_walk_stash, segment=len(segs)) == E.EINVAL
    if len(segs) == 1:  # k = 16: one segment, no fold launched
        assert k == 16


def check_tables(engine, case, tables, offset=0, m=None):
    m = case["n"] if m is None else m
    for t in range(tables):
        info, words = engine.read_walk_tables(t)
        assert info == E.WalkTablesInfo(m, tables, 8)
        WM.check_table(words, [case["points"][offset + i][t] for i in range(m)], "%s/%s, table %d: " % (case["call"], case["name"], t))
    assert code_of(engine.read_walk_tables, tables) == E.EINVAL


@pytest.mark.parametrize("case", WC.var_cases(), ids=ids(WC.var_cases()))
def test_batch_mul_var(engine, case):
    run_case(engine, case, k=1)
    check_tables(engine, case, 1)  # every record of both read-backs


@pytest.mark.parametrize("case", WC.lincomb2_cases(), ids=ids(WC.lincomb2_cases()))
def test_batch_lincomb2(engine, case):
    run_case(engine, case, k=2)
    check_tables(engine, case, 2)


@pytest.mark.parametrize("case", WC.ed_cases(), ids=ids(WC.ed_cases()))
def test_ed_batch_mul(engine, case):
    run_case(engine, case)


# ------------------------------------------------------------------ more than one pass ----

def short_scalars(count, seed):
    """count 32-byte scalars below 2^16: the passes in front of the last one are cheap and their outputs are not read."""
    s = np.zeros((count, 32), dtype=np.uint8)
    s[:, :2] = np.random.default_rng(seed).integers(0, 256, size=(count, 2), dtype=np.uint8)
    return s.tobytes()


def test_batch_mul_last_pass_is_short(engine):
    """n = 2^20 + 300 at c = 8: the second pass is 300 outputs at offset 2^20, and the read-back describes that pass."""
    n, c, first = WC.MULTI_PASS["batch_mul"]
    tail = [c for c in WC.batch_mul_cases() if c["name"] == "G-c8-n257"][0]
    rows = (tail["rows"] + tail["rows"])[: n - first]
    case = dict(tail, name="two-passes", n=n, rows=[None] * first + rows, crafted=[first + i for i in tail["crafted"]])
    d_s, d_out, d_inf = dev(short_scalars(first, 1) + b"".join(R.encode_scalars(list(row)) for row in rows)), poisoned(96 * n), poisoned(n)
    with settings(engine, c):
        engine.batch_mul_device(V.base_bytes(R.G), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
    finish_last_pass(engine, case, first, d_out, d_inf, msm.batch_mul_host(V.base_bytes(R.G), b"".join(R.encode_scalars(list(row)) for row in rows)), k=1)


def finish_last_pass(engine, case, first, d_out, d_inf, twin, **layout):
    n, m = case["n"], case["n"] - first
    tail_out, tail_flags = bytes(d_out[96 * first : 96 * n].cpu().numpy()), bytes(d_inf[first:n].cpu().numpy())
    decoded = check_pass(engine, case, tail_out, tail_flags, twin[0], twin[1], offset=first, m=m, out_first=first, **layout)
    assert (tail_out, tail_flags) == twin
    compare_model(case, decoded, offset=first)
    return decoded


def test_batch_mul_var_last_pass_is_short(engine):
    """n = 2^17 + 257: the whole 257-point last pass, stash and tables, at offset 2^17."""
    import torch

    n, _, first = WC.MULTI_PASS["var"]
    tail = [c for c in WC.var_cases() if c["name"] == "wire-n257"][0]
    case = dict(tail, name="two-passes", n=n, rows=[None] * first + tail["rows"], points=[None] * first + tail["points"], crafted=[first + i for i in tail["crafted"]])
    pts, sb = point_records([p for p, in tail["points"]], "wire"), b"".join(R.encode_scalars(list(row)) for row in tail["rows"])
    d_p = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    engine.generate_bases_device(0x5EED, first, d_p.data_ptr())
    d_p[96 * first :] = dev(pts)
    d_s, d_out, d_inf = dev(short_scalars(first, 2) + sb), poisoned(96 * n), poisoned(n)
    engine.batch_mul_var_device(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
    finish_last_pass(engine, case, first, d_out, d_inf, msm.batch_mul_var_host(pts, sb), k=1)
    check_tables(engine, case, 1, offset=first, m=n - first)


def test_batch_lincomb2_last_pass_is_short(engine):
    """n = 2^16 + 257: the 257-pair last pass, stash and both tables, at offset 2^16."""
    import torch

    n, _, first = WC.MULTI_PASS["lincomb2"]
    tail = [c for c in WC.lincomb2_cases() if c["name"] == "wire-n257"][0]
    case = dict(tail, name="two-passes", n=n, rows=[None] * first + tail["rows"], points=[None] * first + tail["points"], crafted=[first + i for i in tail["crafted"]])
    p, q = (point_records([x[j] for x in tail["points"]], "wire") for j in (0, 1))
    a, b = (R.encode_scalars([row[j] for row in tail["rows"]]) for j in (0, 1))
    d_p, d_q = (torch.empty(96 * n, dtype=torch.uint8, device="cuda") for _ in (0, 1))
    engine.generate_bases_device(0x5EED, first, d_p.data_ptr())
    engine.generate_bases_device(0x5EEE, first, d_q.data_ptr())
    d_p[96 * first :], d_q[96 * first :] = dev(p), dev(q)
    d_a, d_b, d_out, d_inf = dev(short_scalars(first, 3) + a), dev(short_scalars(first, 4) + b), poisoned(96 * n), poisoned(n)
    engine.batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
    finish_last_pass(engine, case, first, d_out, d_inf, msm.batch_lincomb2_host(p, q, a, b), k=2)
    check_tables(engine, case, 2, offset=first, m=n - first)


# ------------------------------------------------------------------ MSM377_ESTATE ----

def test_state_rule(oracle):
    """Every arm: before the first batch call; after a batch call that returned an error (refused by the form check, and
    refused behind it by the base check); after msm377_g1_set_generators (one that builds, one that is refused); after
    n = 0; the tables after a batch call of another kind.  MSM, check and set-bases calls between a batch call and the
    read-back change nothing.
    What this does NOT reach: a table build that fails AFTER it has written the stash (a HIP error or an allocation that
    fails in mid-build) -- no argument provokes one, both refused calls here end before their build launches anything.
    The rule holds for that arm by construction, and that is what the test relies on: the description is forgotten where
    the call STARTS (forget_walk in the checks that open every batch call and in msm377_g1_set_generators) and is written
    again only behind the wait of a call that ran a pass, so no way out of a call in between can leave it valid."""
    import util

    small = [c for c in WC.batch_mul_cases() if c["name"] == "G-c8-n65"][0]
    var = [c for c in WC.var_cases() if c["name"] == "wire-n65"][0]
    with msm.MsmEngine(1 << 12) as eng:
        lib, ctx = msm.load_library(), eng._ctx
        words = np.full((4, 52), 0xEE, dtype=np.uint32)

        def refused():
            assert code_of(eng.read_walk_stash) == E.ESTATE and code_of(eng.read_walk_tables) == E.ESTATE
            assert lib.msm377_read_walk_stash(ctx, None, 0, 0, 4, words.ctypes.data, None) == E.ESTATE and (words == 0xEE).all()  # nothing written

        refused()  # before the first batch call
        n = 700
        points = util.oracle_gen_points(oracle, n, 0x1234567, 0x89AB)
        ks = R.encode_scalars(R.rand_scalars(0x4E51, n))
        exp = util.oracle_msm(oracle, points, ks)
        assert eng.msm(points, ks) == exp
        refused()  # an MSM is no batch call
        run_case(eng, small, k=1)
        _, before, before_prod = eng.read_walk_stash()
        assert eng.msm(points, ks) == exp  # an MSM, a check call and a set_bases in between change nothing
        assert eng.check_points(points).ok
        eng.set_bases(points)
        assert eng.msm_fixed_base(ks) == exp
        info, after, after_prod = eng.read_walk_stash()
        assert info.m == small["n"] and np.array_equal(before, after) and np.array_equal(before_prod, after_prod)
        assert code_of(eng.read_walk_tables) == E.ESTATE  # not a variable-base or pairwise call
        assert code_of(eng.read_walk_stash, first=60, count=6) == E.EINVAL and code_of(eng.read_walk_stash, segment=1) == E.EINVAL
        d_s, d_out = dev(R.encode_scalars([3, 4])), poisoned(208)
        assert code_of(eng.batch_mul_device, V.base_bytes(R.G), d_s.data_ptr(), 2, d_out.data_ptr(), 0, "mont") == E.EINVAL
        refused()  # after a batch call that returned an error
        run_case(eng, small, k=1)
        bad_base = R.P.to_bytes(48, "little") + R.G[1].to_bytes(48, "little")
        assert code_of(eng.batch_mul_device, bad_base, d_s.data_ptr(), 2, d_out.data_ptr()) == E.EINVAL
        refused()  # ... an error behind the form check
        run_case(eng, small, k=1)
        eng.batch_mul_device(V.base_bytes(R.G), d_s.data_ptr(), 0, d_out.data_ptr())
        refused()  # n = 0 ran no pass
        run_case(eng, var, k=1)
        assert eng.read_walk_tables(info_only=True)[0] == E.WalkTablesInfo(var["n"], 1, 8)
        eng.set_generators(R.encode_points([R.G, R.mul(R.G, 5)]), 8)
        refused()  # a table build went through the stash
        run_case(eng, var, k=1)
        assert code_of(eng.set_generators, R.encode_points([R.G] * 65), 16) == E.EINVAL
        refused()  # ... and a set_generators that fails forgets it too
        run_case(eng, var, k=1)
        run_case(eng, small, k=1)
        assert code_of(eng.read_walk_tables) == E.ESTATE and eng.read_walk_stash(info_only=True)[0].kind == E.WALK_BATCH_MUL
        got = eng.batch_mul(V.base_bytes(R.G), R.encode_scalars([r - 1, 0, 7]))  # a host-buffer call: its last piece
        info, pts, _ = eng.read_walk_stash()
        assert (info.n, info.m, info.pass_offset) == (3, 3, 0) and WM.check_g1_stash(pts) == [R.neg(R.G), None, R.mul(R.G, 7)]
        assert got == msm.batch_mul_host(V.base_bytes(R.G), R.encode_scalars([r - 1, 0, 7]))
        eng.set_generators(None)
