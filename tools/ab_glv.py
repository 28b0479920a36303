#!/usr/bin/env python3
"""One GLV MSM at 2^20 (Weierstrass form, set_glv(True), inputs resident in HBM) on the library MSM377_LIB names:
median, fastest and slowest of 15 calls after 3 warm-up calls, host clock around each call.  Interleave builds as
tools/ab_libs.sh does:
  for r in 1 2 3 4; do for lib in ab/libmsm377_parent.so webgpu-msm-bls12-377_amd/csrc/libmsm377.so; do
    MSM377_LIB=$lib python3 tools/ab_glv.py; done; done"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import webgpu_msm_bls12_377_amd as msm
import bench

n = 1 << 20
eng = msm.MsmEngine(n, device=0)
eng.set_g1_form("weierstrass")
eng.set_glv(True)
d_points = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
eng.generate_bases_device(0x377, n, d_points.data_ptr())
d_scalars = torch.frombuffer(bytearray(bench.seeded_scalars(0x5CA1A5, n)), dtype=torch.uint8).cuda()
torch.cuda.synchronize()
ts = []
for i in range(18):
    t0 = time.perf_counter()
    out = eng.msm_device(d_points.data_ptr(), d_scalars.data_ptr(), n)
    ts.append((time.perf_counter() - t0) * 1e3)
assert eng.last_geometry() == (8, 15)
ts = sorted(ts[3:])
print("%-44s median %.4f ms  min %.4f  max %.4f  result %s" % (os.environ.get("MSM377_LIB", "tree"), ts[len(ts) // 2], ts[0], ts[-1], out[:8].hex()))
eng.close()
