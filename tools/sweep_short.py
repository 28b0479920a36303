#!/usr/bin/env python3
"""Short-scalar G1 MSM against the full-width call on the same values, inputs resident.

For n in 2^14, 2^16, 2^18, 2^20 and scalar widths 8, 32, 64, 128, 253 bits:
    A = msm377_g1_msm_device on the scalars zero-extended to 32 bytes
    B = msm377_g1_msm_short_device on the compact scalars (the smallest stride that fits) with the width declared
A and B alternate call by call in one process (they share whatever else runs on the host), after a warm-up of both;
the table gives the median and the spread (min .. max, and the interquartile range) of each over REPEATS calls, the
geometry B ran, and whether B's median exceeds A's by more than A's own spread (IQR).  Results are checked against
each other once per point (A and B must agree bit for bit).

    python tools/sweep_short.py [--repeats 30] [--warmup 5] > profiles/short_scalars/sweep.txt
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import webgpu_msm_bls12_377_amd as msm  # noqa: E402


def stride_for(bits):
    return 4 if bits <= 32 else 8 if bits <= 64 else 16 if bits <= 128 else 32


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="14,16,18,20")
    ap.add_argument("--widths", default="8,32,64,128,253")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    widths = [int(w) for w in args.widths.split(",")]
    cap = max(sizes)
    eng = msm.MsmEngine(cap, device=0)
    d_points = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    eng.generate_bases_device(0x377, cap, d_points.data_ptr())
    torch.cuda.synchronize()
    pp = d_points.data_ptr()
    print("# %s; A = msm_device on zero-extended scalars, B = msm_short_device; ms per call, %d alternating repeats after %d warm-up calls of each"
          % (msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# %-5s %-5s %-9s | %-31s | %-31s | %-7s %s" % ("n", "bits", "geometry", "A median [q1..q3] (min..max)", "B median [q1..q3] (min..max)", "B/A", "verdict"))
    for bits in widths:
        sb = stride_for(bits)
        rng = random.Random(0x5A0 + bits)
        # cap scalars below 2^bits (bit bits - 1 set in the first): every n takes a prefix
        raw = bytearray(rng.getrandbits(8 * sb * cap).to_bytes(sb * cap, "little"))
        ks = [int.from_bytes(raw[sb * i : sb * i + sb], "little") & ((1 << bits) - 1) for i in range(cap)]
        ks[0] |= 1 << (bits - 1)
        d_wide = torch.frombuffer(bytearray(msm.encode_scalars(ks, 32)), dtype=torch.uint8).cuda()
        d_short = torch.frombuffer(bytearray(msm.encode_scalars(ks, sb)), dtype=torch.uint8).cuda()
        del ks, raw
        torch.cuda.synchronize()
        wp, sp = d_wide.data_ptr(), d_short.data_ptr()
        for n in sizes:
            a_out = b_out = None
            for _ in range(args.warmup):
                a_out = eng.msm_device(pp, wp, n)
                b_out = eng.msm_short_device(pp, sp, n, sb, bits)
            geom = eng.last_geometry()
            assert a_out == b_out, "A and B disagree at n=%d bits=%d" % (n, bits)
            ta, tb = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                eng.msm_device(pp, wp, n)
                t1 = time.perf_counter()
                eng.msm_short_device(pp, sp, n, sb, bits)
                t2 = time.perf_counter()
                ta.append((t1 - t0) * 1e3)
                tb.append((t2 - t1) * 1e3)
            ma, mb = statistics.median(ta), statistics.median(tb)
            (a1, a3), (b1, b3) = quartiles(ta), quartiles(tb)
            verdict = "B slower than A beyond A's spread" if mb > ma + (a3 - a1) else "ok"
            print("2^%-4d %-5d (%2d, %2d)  | %.3f [%.3f..%.3f] (%.3f..%.3f) | %.3f [%.3f..%.3f] (%.3f..%.3f) | %.3f   %s"
                  % (n.bit_length() - 1, bits, geom[0], geom[1], ma, a1, a3, min(ta), max(ta), mb, b1, b3, min(tb), max(tb), mb / ma, verdict), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
