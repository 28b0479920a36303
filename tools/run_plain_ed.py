#!/usr/bin/env python3
"""A few Edwards-BLS12 MSMs (device buffers, then host buffers) with stage timing and stage capture off, for a kernel
trace: python tools/run_plain_ed.py LOG_N [CALLS].  MSM377_LIB selects another build of the library."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import webgpu_msm_bls12_377_amd as msm
import bench

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n = 1 << log_n
eng = msm.MsmEngine(n, device=0)
d_points = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
eng.ed_generate_bases_device(0xED, n, d_points.data_ptr())
ks = bench.seeded_scalars(0x5CA1A5, n)  # below r < 2^253: the even geometry, no rerun
d_scalars = torch.frombuffer(bytearray(ks), dtype=torch.uint8).cuda()
torch.cuda.synchronize()
for _ in range(calls):
    out = eng.ed_msm_device(d_points.data_ptr(), d_scalars.data_ptr(), n)
points = d_points.cpu().numpy().tobytes()
assert eng.ed_msm(points, ks) == out
print(out[:8].hex())
