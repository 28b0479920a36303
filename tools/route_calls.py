#!/usr/bin/env python3
"""One call of every route of the stage sequencer, fixed seeds, a few thousand points, contexts of 2^17 points; every
answer is checked against the CPU oracle (pyref's group law where a point lies outside the prime-order subgroup).  Prints
"ok" and nothing else.  Meant to run under a kernel trace, once per build (MSM377_LIB), so that the launches of two builds
can be compared route by route: the order of the calls below is the order of the trace.
  route_calls.py            every route
  route_calls.py existing   every route but the last one (the twin's knobs)
  route_calls.py twin       that one alone: a batch of 4 on a context whose knobs differ from the environment's when its
                            twin is made -- the twin's half runs its owner's launch shapes"""
import os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import ESCALAR, combine_partials_bytes

CAP, N = 1 << 17, 2049
BIG = (1 << 253) + 12345  # fits sixteen equal windows only
T2 = (R.P - 1, 0)  # a point of order two: no Edwards record
oracle = util.load_oracle()
which = sys.argv[1] if len(sys.argv) > 1 else "all"


def engine(**env):
    """A context with knobs that are read at creation."""
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return msm.MsmEngine(CAP)
    finally:
        for k in env:
            del os.environ[k]


def dev(buf):
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def expect(got, exp, what):
    if got != exp:
        sys.exit("route_calls: wrong answer on route: " + what)


pts = util.oracle_gen_points(oracle, N, 0x377377377, 0x5CA1A5)
kl = R.rand_scalars(0xC0FFEE, N)
kl_big = list(kl)
kl_big[1000] = BIG
ks, ks_big = R.encode_scalars(kl), R.encode_scalars(kl_big)
exp, exp_big = util.oracle_msm(oracle, pts, ks), util.oracle_msm(oracle, pts, ks_big)
pl = R.decode_points(pts)


def with_t2(i):
    """The points with (-1, 0) at index i, and the sum of the plain scalars over them."""
    bad = bytearray(pts)
    bad[96 * i : 96 * i + 96] = R.encode_points([T2])
    total = R.add(R.add(R.decode_result(exp), R.neg(R.mul(pl[i], kl[i]))), R.mul(T2, kl[i]))
    return bytes(bad), R.encode_result(total)


d_p, d_s, d_big = dev(pts), dev(ks), dev(ks_big)
pp, sp, bp = d_p.data_ptr(), d_s.data_ptr(), d_big.data_ptr()
ks2 = R.encode_scalars(R.rand_scalars(0xBA7C4, N))
exp2 = util.oracle_msm(oracle, pts, ks2)
d_b = dev(ks + ks2 + ks2 + ks)


def twin_route():
    """The variables are gone when the first batch of 4 makes the twin: both halves reduce with coop_threads = 2^20.  The
    column launches take the first quad level as an argument, so (kernel, grid, workgroup) shows the knob only in the
    second context, whose levels run one launch each: k_tree_step below that level, k_tree_step_quad from it on."""
    for env in ({"MSM377_COOP_THREADS": 1048576}, {"MSM377_COOP_THREADS": 1048576, "MSM377_REDUCE_COLUMNS": 0}):
        owner = engine(**env)
        owner.set_narrow_max(0)
        owner.set_bases(pts)
        expect(owner.msm_fixed_base_batch_device(d_b.data_ptr(), N, 4), [exp, exp2, exp2, exp], "batch of 4, knobs of the owner: %s" % sorted(env))
        owner.close()


if which == "twin":
    twin_route()
    print("ok")
    sys.exit(0)
eng = engine()

# per-call Edwards form: narrow, even16, each with a scalar of 2^253 and more
expect(eng.msm_device(pp, sp, N), exp, "narrow")
expect(eng.msm_device(pp, bp, N), exp_big, "narrow, big scalar")
eng.set_narrow_max(0)
expect(eng.msm_device(pp, sp, N), exp, "even16")
expect(eng.msm_device(pp, bp, N), exp_big, "even16, big scalar")
eng.set_narrow_max()

# fixed base on the three tables, full width and short; the 20-bit one also with a big scalar
kl64 = [k & ((1 << 64) - 1) for k in kl]
kl64[N - 1] |= 1 << 63
ks64, exp64 = msm.encode_scalars(kl64, 8), util.oracle_msm(oracle, pts, R.encode_scalars(kl64))
d_64 = dev(ks64)
for name in ("plain", "precomputed16", "precomputed20"):
    if name == "plain":
        eng.set_bases(pts)
    else:
        eng.set_precompute_window(int(name[-2:]))
        eng.set_bases_precomputed(pts)
    expect(eng.msm_fixed_base_device(sp, N), exp, "fixed base, " + name)
    expect(eng.msm_fixed_base_short_device(d_64.data_ptr(), N, 8, 64), exp64, "short fixed base, " + name)
    if name == "precomputed20":
        expect(eng.msm_fixed_base_device(bp, N), exp_big, "20-bit table, big scalar")
eng.set_precompute_window(16)

# short calls through device and host buffers, and a broken promise
expect(eng.msm_short_device(pp, d_64.data_ptr(), N, 8, 64), exp64, "short device")
expect(eng.msm_short(pts, ks64, 8, 64), exp64, "short host")
try:
    eng.msm_short_device(pp, sp, N, 32, 64)
    sys.exit("route_calls: a broken width promise went through")
except msm.MsmError as e:
    expect(e.code, ESCALAR, "broken promise")

# batches over a resident set: 2 on one context, 4 on the twin as well
eng.set_bases(pts)
expect(eng.msm_fixed_base_batch_device(d_b.data_ptr(), N, 2), [exp, exp2], "batch of 2")
expect(eng.msm_fixed_base_batch_device(d_b.data_ptr(), N, 4), [exp, exp2, exp2, exp], "batch of 4")

# a two-torsion point: per call, and in a resident set
bad, exp_bad = with_t2(777)
d_bad = dev(bad)
expect(eng.msm_device(d_bad.data_ptr(), sp, N), exp_bad, "two-torsion point per call")
eng.set_bases(bad)
expect(eng.msm_fixed_base_device(sp, N), exp_bad, "two-torsion point in a resident set")

# host buffers in one piece; window partials; stage capture
expect(eng.msm(pts, ks), exp, "host buffers unchunked")
expect(eng.combine_partials(eng.window_partials_device(pp, sp, N, 0, 16)), exp, "window partials")
for mode in (1, 2):
    eng.set_stage_capture(mode)
    expect(eng.msm_device(pp, sp, N), exp, "stage capture %d" % mode)
eng.set_stage_capture(0)

# Weierstrass form: plain, GLV, GLV with a half scalar out of range; GLV window partials
eng.set_g1_form("weierstrass")
expect(eng.msm_device(pp, sp, N), exp, "Weierstrass")
eng.set_glv(True)
expect(eng.msm_device(pp, sp, N), exp, "GLV")
kl_glv = list(kl)
kl_glv[5] = (1 << 254) + 7  # a half scalar of 2^127 and more
ks_glv = R.encode_scalars(kl_glv)
d_glv = dev(ks_glv)
expect(eng.msm_device(pp, d_glv.data_ptr(), N), util.oracle_msm(oracle, pts, ks_glv), "GLV, half scalar out of range")
expect(combine_partials_bytes(eng.glv_window_partials_device(pp, sp, N, 0, 8), 8), exp, "GLV window partials")
eng.set_glv("auto")
eng.set_g1_form("edwards")
eng.close()

# per-call affine records, and window partials through the affine gate
aff = engine(MSM377_AFFINE_MIN=1)
expect(aff.msm_device(pp, sp, N), exp, "affine records")
expect(aff.combine_partials(aff.window_partials_device(pp, sp, N, 0, 16)), exp, "window partials, affine gate")
aff.close()

# host buffers in chunks: plain, a big scalar, an exceptional point in a later chunk
chunked = engine(MSM377_UPLOAD_CHUNK_MIN=100)
expect(chunked.msm(pts, ks), exp, "host buffers chunked")
expect(chunked.msm(pts, ks_big), exp_big, "host buffers chunked, big scalar")
bad, exp_bad = with_t2(N - 3)
expect(chunked.msm(bad, ks), exp_bad, "host buffers chunked, exceptional point in the last chunk")

# Edwards-BLS12: device, chunked, chunked with a big scalar
ed_pts = util.oracle_ed_gen_points(oracle, N, 0xED377, 0xED5CA1A5)
d_ed = dev(ed_pts)
ed_exp, ed_exp_big = util.oracle_ed_msm(oracle, ed_pts, ks), util.oracle_ed_msm(oracle, ed_pts, ks_big)
expect(chunked.ed_msm_device(d_ed.data_ptr(), sp, N), ed_exp, "Edwards-BLS12 device")
expect(chunked.ed_msm(ed_pts, ks), ed_exp, "Edwards-BLS12 chunked")
expect(chunked.ed_msm(ed_pts, ks_big), ed_exp_big, "Edwards-BLS12 chunked, big scalar")
chunked.close()

# launch shapes decided inside the pass (sequencer.hip launch_record and its stage functions): one knob per context
for knob, value, paths in (
    ("MSM377_REDUCE_COLUMNS", 0, ("main", "narrow")),  # one launch per reduction level: k_tree_step / k_tree_step_quad
    ("MSM377_TAIL_LDS", 0, ("main",)),                 # k_reduce_tail in global memory
    ("MSM377_TAIL_FROM", 4, ("main",)),                # a stretch of buckets beyond the LDS of a CU: k_reduce_tail
    ("MSM377_TAIL_FROM", 6, ("main",)),                # 104 KB of LDS: the dynamic-LDS attribute in front of k_reduce_tail_lds
    ("MSM377_SORT_ELEM", 4, ("main",)),
    ("MSM377_NARROW_QUAD_ITEMS", 0, ("narrow",)),
    ("MSM377_COOP_THREADS", 1048576, ("main",)),
    ("MSM377_ZERO_COPY_OUT", 0, ("narrow",)),
):
    knobbed = engine(**{knob: value})
    for path in paths:
        knobbed.set_narrow_max(0 if path == "main" else 1 << 16)
        expect(knobbed.msm_device(pp, sp, N), exp, "%s=%d, %s path" % (knob, value, path))
    knobbed.close()

# a short call on the narrow path; a shard of three windows beside the records of a whole call; stage timing
plain = engine()
expect(plain.msm_short_device(pp, d_64.data_ptr(), N, 8, 64), exp64, "short device, narrow path")
W = len(plain.window_partials_device(pp, sp, N, 0, 1))
whole, shard = plain.window_partials_device(pp, sp, N, 0, 16), plain.window_partials_device(pp, sp, N, 5, 3)
expect(plain.combine_partials(whole[: 5 * W] + shard + whole[8 * W :]), exp, "window partials [5, 8)")
for mode in (1, 2):
    plain.set_timing(mode)
    expect(plain.msm_device(pp, sp, N), exp, "timing %d" % mode)
plain.set_timing(0)
plain.close()
if which == "all":
    twin_route()
print("ok")
