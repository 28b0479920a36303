// Variable-base batch multiplication on Edwards-BLS12 (msm377_ed_batch_mul_var*): out[i] = [s_i]P_i, every output its own
// 64-byte wire point, n scalars or ONE scalar for all points (record scanning [view_key] nonce_i, the ElGamal / ECDH halves
// [r_i]PK_i).  The structure is that of kernels/batch_mul_var.hpp -- per-point tables [1..8]P_i through the stash and the
// normalisation, the signed 4-bit recode of batch_mul_var_recode.hpp, a thread per output -- on the complete law of
// ed_ext.hpp / te377.hpp: no identity / equal / opposite exits anywhere, no flags, every curve point a legal input (the
// identity, orders 2 and 4, P + T), mixed freely within one wave.  The law is complete ON THE CURVE only and the pass's one
// batched inversion needs every Z non-zero: the call refuses a point that is not on the curve before it launches anything
// here (sequencer.hip edbmv_check_points, k_check_curve<EdCheck>).
//
//   k_edbmv_table       a thread per point: wire x || y to Montgomery form, then [e]P_i, e = 1 .. 8, as extended points into
//                       the stash at (e - 1) m + i (m: the points of this pass) with the canonical Ed:: formulas -- one dbl,
//                       six madd; normalise<EdMul>(EDBM_FORM_TABLE) makes 128-byte records (y - x, y + x, 2dxy) of them
//   k_edbmv_accumulate  THE HOT KERNEL: a thread per output walks the 64 signed digits of its scalar from the top into ONE
//                       lazy accumulator: acc = carry ? P : O, then 64 steps acc = 16 acc + d_w P -- three T-less lazy
//                       doublings (EdLazy::dbl_nt, 7 products), one full one (8) and one EdLazy::madd_affine (7):
//                       64 x 36 = 2 304 products per output, no canon and no modular add / sub between them
// Device code; included by sequencer.hip only (after kernels/ed_batch_mul.hpp and kernels/batch_mul_var.hpp).
#pragma once
#include "../batch_mul_var_recode.hpp"
#include "batch_mul_var.hpp"
#include "ed_batch_mul.hpp"

namespace msm377 {
namespace {

// Runs once per point beside the 2 304 products of the walk.  Every value is canonical (Fq::mul / add / sub), as the
// normalisation asks of the stash.
__global__ void __launch_bounds__(BM_THREADS) k_edbmv_table(const uint8_t* __restrict__ points, uint64_t m, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (i >= m) return;
  uint32_t raw[16];
  load_words16(reinterpret_cast<const uint32_t*>(points + i * 64), raw, 4);
  Ed::Ext acc;
  acc.x = Fq::to_mont(Fq::from_words<8>(raw));
  acc.y = Fq::to_mont(Fq::from_words<8>(raw + 8));
  acc.t = Fq::mul(acc.x, acc.y);
  acc.z = Fq::one();
  const Ed::Base p = Ed::make_base(acc.x, acc.y);
  edbm_store_point(stash, i, acc.x, acc.y, acc.t, acc.z);
  acc = Ed::dbl(acc);
#pragma unroll 1
  for (uint32_t e = 1; e < (uint32_t)BMV_ENTRIES; e++) {
    edbm_store_point(stash, (uint64_t)e * m + i, acc.x, acc.y, acc.t, acc.z);
    acc = Ed::madd(acc, p);
  }
}

// One step's four doublings.  MSM377_EDBMV_CANON_DBL (a build switch of the measurement in profiles/ed_batch_mul_var only)
// runs the canonical Ed::dbl_nt / Ed::dbl in their place, on canonical values.
__device__ __forceinline__ EdLazy::Ext edbmv_dbl4(EdLazy::Ext acc) {
#if defined(MSM377_EDBMV_CANON_DBL)
  Ed::Ext c;
  c.x = Fq::canon(acc.x);
  c.y = Fq::canon(acc.y);
  c.t = Fq::zero();
  c.z = Fq::canon(acc.z);
#pragma unroll 1
  for (int k = 0; k < BMV_WIDTH - 1; k++) c = Ed::dbl_nt(c);
  c = Ed::dbl(c);
  acc.x = c.x;
  acc.y = c.y;
  acc.t = c.t;
  acc.z = c.z;
  return acc;
#else
#pragma unroll 1
  for (int k = 0; k < BMV_WIDTH - 1; k++) acc = EdLazy::dbl_nt(acc);
  return EdLazy::dbl(acc);
#endif
}

// ---- the hot kernel ----
// table: BMV_ENTRIES x m records, [e]P_i at (e - 1) m + i.  scalars: m x 8 words, or 8 words for all (stride_words = 0),
// read as integers and not reduced.  `started`: the lane has left the start value O (a carry, or a non-zero digit so
// far); leading windows in which no lane of the wave has started and every digit is zero are skipped (16 O + 0 = O):
// short scalars and the one-scalar form pay for their own length only.  Inside a window a lane with a zero digit sits the
// addition out.  The accumulator is a lazy point throughout (te377.hpp: every coordinate the output of a lazy product;
// tools/check_lazy_bounds.py replays the chain) and leaves the kernel canonical (Fq::canon: any N-form value below 8 q).
// The carry is the digit of 2^256: step 64 of the same loop, an addition to O without doublings, so that the kernel holds
// ONE copy of the addition.
// Code object (profiles/ed_batch_mul_var/device_code.txt): 102 VGPRs, no scratch, no spill, four waves per SIMD.
// Measured (profiles/ed_batch_mul_var/): 1.82 ms per 2^17 outputs against 2.56 ms for k_check_subgroup<EdCheck>'s chain of
// 2 616 canonical products; with the canonical doublings in place of the lazy ones the call takes 24.1 instead of 19.3 ms.
__global__ void __launch_bounds__(BM_THREADS, 4) k_edbmv_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint64_t m, uint32_t stride_words,
                                                                    uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < m;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = 0;  // an idle lane walks the zero scalar: no digit, no load
  if (live) load_words16(scalars + i * stride_words, s, 2);
  const uint32_t carry = bmv_pack(s);
  EdLazy::Ext acc = EdLazy::identity();
  bool started = false;
#pragma unroll 1
  for (int w = BMV_WINDOWS; w >= 0; w--) {  // step 64 is the carry's: the digit of 2^256, on acc = O (ONE copy of the addition)
    const int32_t d = w == BMV_WINDOWS ? (int32_t)carry : bmv_next(s);
    const bool act = d != 0;
    started |= act;
    if (__ballot(started) == 0) continue;  // wave-uniform
    if (w != BMV_WINDOWS) acc = edbmv_dbl4(acc);
    if (act) {                             // (never an idle lane)
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
      acc = EdLazy::madd_affine(acc, EdDev::load_base(table, (uint32_t)((uint64_t)(mag - 1u) * m + i)), d < 0);
    }
  }
  if (live) edbm_store_point(stash, i, Fq::canon(acc.x), Fq::canon(acc.y), Fq::canon(acc.t), Fq::canon(acc.z));
}

}  // namespace
}  // namespace msm377
