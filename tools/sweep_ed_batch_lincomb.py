#!/usr/bin/env python3
"""Edwards-BLS12 k-term linear combination (msm377_ed_batch_lincomb_device), inputs and outputs resident.

Every shape alternates, repetition by repetition in one process after a warm-up of all three,
       A = way A on the parent's calls: k msm377_ed_batch_mul_var_device calls, joined by k - 1
           msm377_ed_batch_lincomb2_device calls with a = b = 1 (stride-0 scalars)
       B = way B: floor(k / 2) msm377_ed_batch_lincomb2_device calls, plus one msm377_ed_batch_mul_var_device call for odd k,
           joined the same way
       C = msm377_ed_batch_lincomb_device(terms, k, n)
on the points of ed_generate_bases_device and the same scalars, and compares the bytes of all three at every shape.
k in {3, 4, 8} at n in {2^12, 2^16, 2^20} with full-width uniform scalars, and at 2^20 with 64-bit scalars.  The call is to
beat the better way at every one of these shapes with the medians outside both quartile spreads: a line says "met" or
"MISSED".  The model beside each ratio counts field products: 64 (29 + 7k) per output for the joint walk against the ways'
walks (2 304 per variable-base walk, 2 752 per pairwise walk) plus 14 per joining pass (a = b = 1: only the last step
runs, two additions).  What a joining pass costs beyond its products -- two table builds, two normalisations -- is what the
measured ratio shows and the model does not.

Recorded without a gate:
  - k = 1 against msm377_ed_batch_mul_var_device and k = 2 against msm377_ed_batch_lincomb2_device at 2^20: what the LDS
    digits and the run-time loop over the terms cost (the older calls remain the ones to use there);
  - the call over its floor: n x 64 (29 + 7k) products at the product rate k_accumulate<EdDev> reaches in an
    msm377_ed_msm_device of 2^20 points in this session.

    python tools/sweep_ed_batch_lincomb.py [--repeats 30] [--warmup 3] > profiles/ed_batch_lincomb/sweep.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import webgpu_msm_bls12_377_amd as msm  # noqa: E402

MAX_TERMS = 8
VAR_WALK = 64 * (29 + 7)
PAIR_WALK = 64 * (29 + 14)
JOIN = 2 * 7  # a = b = 1: only the last step runs, two additions to O and to P


def walk_products(k):
    return 64 * (29 + 7 * k)


def way_products(k, way):
    if way == "A":
        return k * VAR_WALK + (k - 1) * JOIN
    parts = (k + 1) // 2
    return (k // 2) * PAIR_WALK + (k % 2) * VAR_WALK + (parts - 1) * JOIN


def fmt(ts):
    q = statistics.quantiles(ts, n=4)
    return "%.3f [%.3f..%.3f]" % (statistics.median(ts), q[0], q[2])


def quartiles(ts):
    q = statistics.quantiles(ts, n=4)
    return q[0], q[2]


def alternate(calls, repeats, warmup):
    for _ in range(warmup):
        for call in calls:
            call()
    times = [[] for _ in calls]
    for _ in range(repeats):
        for ts, call in zip(times, calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--terms", default="3,4,8")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    ks = [int(k) for k in args.terms.split(",")]
    cap = 1 << 20
    eng = msm.MsmEngine(cap, device=0)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    gen = torch.Generator().manual_seed(0xBA7C6)
    d_pts, d_full, d_short = [], [], []
    for t in range(MAX_TERMS):
        d_x = torch.empty(64 * cap, dtype=torch.uint8, device="cuda")
        eng.ed_generate_bases_device(0x377E0 + t, cap, ptr(d_x))
        d_pts.append(d_x)
        d_s = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
        d_full.append(d_s)
        d_c = d_s.clone()
        d_c[:, 8:] = 0
        d_short.append(d_c)
    d_tmp = [torch.empty(64 * cap, dtype=torch.uint8, device="cuda") for _ in range(MAX_TERMS)]
    d_out = {w: torch.empty(64 * cap, dtype=torch.uint8, device="cuda") for w in "ABC"}
    d_one = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_one[0] = 1

    def join(parts, n, out):  # parts[0] + parts[1] -> out, then out += parts[j] in place
        eng.ed_batch_lincomb2_device(ptr(parts[0]), ptr(parts[1]), ptr(d_one), ptr(d_one), n, ptr(out), 64, 64, 0, 0)
        for part in parts[2:]:
            eng.ed_batch_lincomb2_device(ptr(out), ptr(part), ptr(d_one), ptr(d_one), n, ptr(out), 64, 64, 0, 0)

    def way_a(k, n, scalars):
        for t in range(k):
            eng.ed_batch_mul_var_device(ptr(d_pts[t]), ptr(scalars[t]), n, ptr(d_tmp[t]))
        join(d_tmp[:k], n, d_out["A"])

    def way_b(k, n, scalars):
        parts = []
        for t in range(0, k - 1, 2):
            eng.ed_batch_lincomb2_device(ptr(d_pts[t]), ptr(d_pts[t + 1]), ptr(scalars[t]), ptr(scalars[t + 1]), n, ptr(d_tmp[t // 2]))
            parts.append(d_tmp[t // 2])
        if k % 2:
            eng.ed_batch_mul_var_device(ptr(d_pts[k - 1]), ptr(scalars[k - 1]), n, ptr(d_tmp[k // 2]))
            parts.append(d_tmp[k // 2])
        join(parts, n, d_out["B"])

    def call(k, n, scalars, out=None):
        eng.ed_batch_lincomb_device([(ptr(d_pts[t]), ptr(scalars[t]), 64, 32) for t in range(k)], n, ptr(out if out is not None else d_out["C"]))

    version = msm.load_library().msm377_version().decode()
    print("# %s; ms, median [q1..q3] of %d repetitions alternating A, B, C after %d warm-up rounds; inputs and outputs resident" % (version, args.repeats, args.warmup))
    print("# products per output: joint walk 64 (29 + 7k); a variable-base walk %d, a pairwise walk %d, a joining pass %d" % (VAR_WALK, PAIR_WALK, JOIN))

    # the product rate of the Edwards-BLS12 bucket accumulation in this session
    n = 1 << 20
    d_msm = d_full[0].clone()
    d_msm[:, 31] &= 0x0F  # below 2^252: no rerun
    eng.set_timing(2)
    acc = []
    for i in range(args.warmup + 10):
        eng.ed_msm_device(ptr(d_pts[0]), ptr(d_msm), n)
        if i >= args.warmup:
            acc.append(eng.stage_ms()["accumulate_kernel"])
    eng.set_timing(0)
    per_add = eng.accumulate_products()
    rate = 16 * n * per_add / statistics.median(acc) * 1e3
    print("ed_msm_device n = 2^20, accumulation kernel | %s | 16 x n additions x %d products: %.1f G products/s" % (fmt(acc), per_add, rate / 1e9), flush=True)

    print("# A = way A, B = way B (the parent's calls), C = ed_batch_lincomb_device; gate: C beats the better way, medians outside both quartile spreads")
    shapes = [("full-width", d_full, n) for n in sizes] + [("64-bit", d_short, 1 << 20)]
    for k in ks:
        for name, scalars, n in shapes:
            ta, tb, tc = alternate([lambda: way_a(k, n, scalars), lambda: way_b(k, n, scalars), lambda: call(k, n, scalars)], args.repeats, args.warmup)
            same = all(torch.equal(d_out[w][: 64 * n], d_out["C"][: 64 * n]) for w in "AB")
            best_name, best = min((("A", ta), ("B", tb)), key=lambda x: statistics.median(x[1]))
            mb, mc = statistics.median(best), statistics.median(tc)
            clear = quartiles(tc)[1] < quartiles(best)[0]
            model = walk_products(k) / way_products(k, best_name)
            print("k = %d %-10s n = 2^%-2d | A %s | B %s | C %s | C / %s = %.3f (products: %.3f) | %.2f M outputs/s | C / floor %.2f | bytes %s | %s" % (
                k, name, n.bit_length() - 1, fmt(ta), fmt(tb), fmt(tc), best_name, mc / mb, model, n / mc / 1e3, mc / (walk_products(k) * n / rate * 1e3),
                "equal" if same else "DIFFER", "met" if mc < mb and clear else "MISSED"), flush=True)

    print("# no gate: k = 1 against ed_batch_mul_var_device, k = 2 against ed_batch_lincomb2_device, n = 2^20 full-width: the cost of the LDS digits and of the run-time loop")
    n = 1 << 20
    old1 = lambda: eng.ed_batch_mul_var_device(ptr(d_pts[0]), ptr(d_full[0]), n, ptr(d_out["A"]))  # noqa: E731
    old2 = lambda: eng.ed_batch_lincomb2_device(ptr(d_pts[0]), ptr(d_pts[1]), ptr(d_full[0]), ptr(d_full[1]), n, ptr(d_out["A"]))  # noqa: E731
    for k, old in ((1, old1), (2, old2)):
        to, tc = alternate([old, lambda: call(k, n, d_full)], args.repeats, args.warmup)
        same = torch.equal(d_out["A"], d_out["C"])
        print("k = %d full-width n = 2^20 | older call %s | C %s | C / older = %.3f | bytes %s" % (k, fmt(to), fmt(tc), statistics.median(tc) / statistics.median(to), "equal" if same else "DIFFER"), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
