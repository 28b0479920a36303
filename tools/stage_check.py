#!/usr/bin/env python3
"""Kernel times of the point validation (kernels/validate.hpp) at 2^LOG_N generated G1 points, HIP events around each
launch: python tools/stage_check.py [LOG_N] [REPS].  Prints k_check_curve beside k_convert_bases<TeDev> on the same
buffer in the same run (the projective Edwards conversion: MSM377_AFFINE_MIN is raised so that msm_device uses it),
k_check_subgroup, its share of the int32 multiply-add roof, and the wall time of whole check calls."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n = 1 << log_n
os.environ["MSM377_AFFINE_MIN"] = str(2 * n)
import torch
import webgpu_msm_bls12_377_amd as msm
import bench

MAD_ROOF = 33.6e12  # int32 multiply-adds per second, profiles/microbench_r01.txt
# the chain (consts_gen.hpp G1_NAF_LEN): 252 doublings, 68 additions.  Executed v_mad_u64_u32 per point from the ISA
# (tools/isa_mix.py on k_check_subgroup<G1Check>: 2 631 per doubling -- 3 squarings of 259, 4 products of 337, a double
# product of 506 --, 3 046 per addition, 674 to load the point), and the nominal count by products: 9 and 10 x 337
MADS_EXECUTED = 252 * 2631 + 68 * 3046 + 674
MADS_NOMINAL = (252 * 9 + 68 * 10) * 337

eng = msm.MsmEngine(n, device=0)
d_points = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
eng.generate_bases_device(0x377, n, d_points.data_ptr())
d_scalars = torch.frombuffer(bytearray(bench.seeded_scalars(0x5CA1A5, n)), dtype=torch.uint8).cuda()
torch.cuda.synchronize()
for _ in range(3):  # untimed: clocks settle, code objects load
    eng.msm_device(d_points.data_ptr(), d_scalars.data_ptr(), n)
    assert eng.check_points_device(d_points.data_ptr(), n, 7).ok
wall = {}
for flags in (1, 3, 7):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.check_points_device(d_points.data_ptr(), n, flags)
        ts.append((time.perf_counter() - t0) * 1e3)
    wall[flags] = statistics.median(ts)
eng.set_timing(True)
conv, curve, sub = [], [], []
for _ in range(reps):  # interleaved
    eng.msm_device(d_points.data_ptr(), d_scalars.data_ptr(), n)
    conv.append(eng.stage_ms()["convert"])
    eng.check_points_device(d_points.data_ptr(), n, 7)
    st = eng.stage_ms()
    curve.append(st["convert"])
    sub.append(st["accumulate_kernel"])
eng.set_timing(False)
sub_ms = statistics.median(sub)
res = {
    "n": n, "reps": reps, "device": torch.cuda.get_device_name(0),
    "k_convert_bases_TeDev_us": round(statistics.median(conv) * 1e3, 1),
    "k_check_curve_us": round(statistics.median(curve) * 1e3, 1),
    "k_check_curve_us_all": [round(x * 1e3, 1) for x in curve],
    "k_check_subgroup_ms": round(sub_ms, 3),
    "k_check_subgroup_ms_all": [round(x, 3) for x in sub],
    "mads_per_point_executed": MADS_EXECUTED, "mads_per_point_nominal": MADS_NOMINAL,
    "mad_roof_fraction_executed": round(MADS_EXECUTED * n / (sub_ms * 1e-3) / MAD_ROOF, 3),
    "mad_roof_fraction_nominal": round(MADS_NOMINAL * n / (sub_ms * 1e-3) / MAD_ROOF, 3),
    "check_call_wall_ms": {"canonical": round(wall[1], 3), "canonical+curve": round(wall[3], 3), "all": round(wall[7], 3)},
}
print(json.dumps(res))
