#!/usr/bin/env python3
"""Native input forms against the wire format on the same logical inputs, inputs resident.

For n in 2^16 and 2^20:
    per-call    A = msm377_g1_msm_device on wire points and scalars
                B = the same call on (MONT_FLAG, MONT): 104-byte Montgomery records (none flagged), Montgomery scalars
    fixed-base  one resident base set (msm377_g1_set_bases_device, from the native records)
                A = msm377_g1_msm_fixed_base_device on wire scalars, B = on Montgomery scalars
    batch 64    A / B = msm377_g1_msm_fixed_base_batch_device over 64 x n scalars, ms per MSM
A and B alternate call by call in one process, after a warm-up of both; the table gives the median and the spread
(interquartile range, min .. max) of each over REPEATS calls and B - A, the cost of the import pass as a caller sees it.
Results are checked against each other once per row (A and B must agree bit for bit).

    python tools/sweep_native.py [--repeats 30] [--warmup 5] > profiles/native_inputs/sweep.txt
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
from webgpu_msm_bls12_377_amd.host.codecs import G1_P, G1_R  # noqa: E402

BATCH = 64


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return q[0], q[2]


def to_native(points_wire: bytes, scalars_wire: bytes):
    """Wire buffers -> (mont_flag records, mont scalars), no point flagged."""
    n = len(scalars_wire) // 32
    pts = bytearray(104 * n)
    for i in range(n):
        for c in (0, 48):
            v = int.from_bytes(points_wire[96 * i + c : 96 * i + c + 48], "little")
            pts[104 * i + c : 104 * i + c + 48] = ((v << 384) % G1_P).to_bytes(48, "little")
    ks = bytearray(32 * n)
    for i in range(n):
        k = int.from_bytes(scalars_wire[32 * i : 32 * i + 32], "little")
        ks[32 * i : 32 * i + 32] = ((k << 256) % G1_R).to_bytes(32, "little")
    return bytes(pts), bytes(ks)


def alternate(call_a, call_b, repeats, warmup, per=1):
    a_out = b_out = None
    for _ in range(warmup):
        a_out, b_out = call_a(), call_b()
    assert a_out == b_out, "A and B disagree"
    ta, tb = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call_a()
        t1 = time.perf_counter()
        call_b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3 / per)
        tb.append((t2 - t1) * 1e3 / per)
    return ta, tb


def row(case, n, ta, tb):
    ma, mb = statistics.median(ta), statistics.median(tb)
    (a1, a3), (b1, b3) = quartiles(ta), quartiles(tb)
    print("%-10s 2^%-3d | %.3f [%.3f..%.3f] (%.3f..%.3f) | %.3f [%.3f..%.3f] (%.3f..%.3f) | %+.3f  %+.1f%%"
          % (case, n.bit_length() - 1, ma, a1, a3, min(ta), max(ta), mb, b1, b3, min(tb), max(tb), mb - ma, 100.0 * (mb - ma) / ma), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="16,20")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    cap = max(sizes)
    eng = msm.MsmEngine(cap, device=0)
    d_wire = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    eng.generate_bases_device(0x377, cap, d_wire.data_ptr())
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(0x1A71FE)
    sc = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen)
    sc[:, 31] &= 0x0F  # below 2^252 < r
    scalars_wire = bytes(sc.numpy().tobytes())
    native_points, native_scalars = to_native(bytes(d_wire.cpu().numpy().tobytes()), scalars_wire)
    d_np = torch.frombuffer(bytearray(native_points), dtype=torch.uint8).cuda()
    d_sw = torch.frombuffer(bytearray(scalars_wire), dtype=torch.uint8).cuda()
    d_sn = torch.frombuffer(bytearray(native_scalars), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    print("# %s; A = wire format, B = (MONT_FLAG, MONT) on the same logical inputs; ms per MSM, %d alternating repeats after %d warm-up calls of each"
          % (msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# %-9s %-5s | %-38s | %-38s | B - A" % ("case", "n", "A median [q1..q3] (min..max)", "B median [q1..q3] (min..max)"))

    def wire(fn):
        def call():
            eng.set_input_format("wire", "wire")
            return fn()
        return call

    def nat(fn):
        def call():
            eng.set_input_format("mont_flag", "mont")
            return fn()
        return call

    for n in sizes:
        ta, tb = alternate(wire(lambda: eng.msm_device(d_wire.data_ptr(), d_sw.data_ptr(), n)), nat(lambda: eng.msm_device(d_np.data_ptr(), d_sn.data_ptr(), n)),
                           args.repeats, args.warmup)
        row("per-call", n, ta, tb)
        eng.set_input_format("mont_flag", "mont")
        eng.set_bases_device(d_np.data_ptr(), n)
        ta, tb = alternate(wire(lambda: eng.msm_fixed_base_device(d_sw.data_ptr(), n)), nat(lambda: eng.msm_fixed_base_device(d_sn.data_ptr(), n)), args.repeats, args.warmup)
        row("fixed-base", n, ta, tb)
        d_bw, d_bn = d_sw[: 32 * n].repeat(BATCH), d_sn[: 32 * n].repeat(BATCH)
        torch.cuda.synchronize()
        ta, tb = alternate(wire(lambda: eng.msm_fixed_base_batch_device(d_bw.data_ptr(), n, BATCH)), nat(lambda: eng.msm_fixed_base_batch_device(d_bn.data_ptr(), n, BATCH)),
                           args.repeats, max(1, args.warmup // 2), per=BATCH)
        row("batch-%d" % BATCH, n, ta, tb)
        del d_bw, d_bn
    eng.set_input_format("wire", "wire")
    eng.close()


if __name__ == "__main__":
    main()
