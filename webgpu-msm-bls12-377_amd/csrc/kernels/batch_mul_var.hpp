// Variable-base batch multiplication (msm377_g1_batch_mul_var*): out[i] = [s_i]P_i, every output its own affine point
// (an SRS update [tau^i]P_i, key specialisation [delta^-1]L_i, each half of an inner-product basis fold).  Nothing in the
// reference corresponds to this; the fixed-base call (kernels/batch_mul.hpp) lends the stash, the on-device
// normalisation (k_bm_up / k_bm_across / k_bm_down) and the table record.
//
//   k_bmv_table       a thread per point: the point from the context's point form, then [e]P_i, e = 1 .. 8, as XYZZ into
//                     the stash at (e - 1) m + i (m: the points of this pass); normalise<G1Mul>(BM_FORM_TABLE) makes
//                     128-byte affine records of them
//   k_bmv_accumulate  THE HOT KERNEL: a thread per output walks the 64 signed 4-bit digits of its scalar from the top
//                     (batch_mul_var_recode.hpp): acc = carry ? P : O, then 64 steps acc = 16 acc + d_w P -- four
//                     doublings of 9 products and one mixed addition of 10 per 4 bits, 64 x 46 = 2 944 products per
//                     output against 256 x (9 + 10) = 4 864 for a binary walk on which a wave adds at every bit
// A fixed window, not NAF: a wave pays for an addition whenever ANY lane has a non-zero digit, so a 1/3-dense NAF costs a
// wave about 256 doublings and 256 additions; fixed windows put every lane's addition on the same step.
// A pass is BMV_PASS = 2^17 points: its 8 x 2^17 table entries are exactly one normalisation chunk.
//
// Every curve point is a legal input (orders 2, 3, 4, 6, points outside the prime-order subgroup, P + T), mixed freely
// within one wave, so dbl / madd keep their identity / equal / opposite exits and the result is followed through:
//   * a table entry may be O ([2]P for order 2, [3]P for order 3, ..): its record carries the flag word and the
//     addition is skipped like a zero digit; a flagged INPUT makes all eight entries O, hence the output;
//   * acc = +-entry and acc = O in the middle of the walk (small orders: all the time) are madd's own exits.
// Device code; included by sequencer.hip only (after kernels/batch_mul.hpp).
#pragma once
#include "../batch_mul_var_recode.hpp"
#include "batch_mul.hpp"

namespace msm377 {
namespace {

constexpr uint64_t BMV_PASS = BM_CHUNK / BMV_ENTRIES;  // 2^17 points: 256 CUs x two 256-thread workgroups
static_assert(BMV_PASS * BMV_ENTRIES == BM_CHUNK && BMV_PASS % BM_THREADS == 0, "a pass's table is one normalisation chunk");

// POINT_FORM: MSM377_POINTS_WIRE / _MONT (96-byte records, 16-byte loads) or MSM377_POINTS_MONT_FLAG (104-byte records,
// 8-byte loads; a flagged record's coordinate bytes are never interpreted).  The conversions are those of
// kernels/import.hpp (one product with 2^22 takes v = x 2^384 to x) and kernels/convert.hpp (x -> the 2^406 limbs).
// Runs once per point beside the 2 944 products of the walk: one doubling and six madd's.  Code object: 256 VGPRs, no
// scratch, one workgroup per CU (dbl_affine and madd side by side, as in k_bmm_entries); 0.17 ms per 2^17 points.
template <uint32_t POINT_FORM>
__global__ void __launch_bounds__(BM_THREADS) k_bmv_table(const uint8_t* __restrict__ points, uint64_t m, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (i >= m) return;
  uint32_t w[24];
  bool flagged = false;
  if constexpr (POINT_FORM == MSM377_POINTS_MONT_FLAG) {
    const uint2* s = reinterpret_cast<const uint2*>(points + i * 104);
    flagged = (s[12].x & 0xffu) != 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const uint2 v = s[k];
      w[2 * k] = v.x;
      w[2 * k + 1] = v.y;
    }
  } else {
    load_words16(reinterpret_cast<const uint32_t*>(points + i * 96), w, 6);
  }
  if (flagged) {
    const G1XYZZ o = G1::identity();
#pragma unroll 1
    for (uint32_t e = 0; e < (uint32_t)BMV_ENTRIES; e++) bm_store_point(stash, (uint64_t)e * m + i, o);
    return;
  }
  G1Affine p;
  p.x = Fp::from_words<12>(w);
  p.y = Fp::from_words<12>(w + 12);
  if constexpr (POINT_FORM != MSM377_POINTS_WIRE) {
    const Fp::El c = Fp::from_const(G1Consts::IMPORT_MONT384);
    p.x = Fp::mul(p.x, c);
    p.y = Fp::mul(p.y, c);
  }
  p.x = Fp::to_mont(p.x);
  p.y = Fp::to_mont(p.y);
  G1XYZZ acc = G1::from_affine(p);
  bm_store_point(stash, i, acc);
  acc = G1::dbl_affine(p);  // Y = 0 (order 2): ZZ = 0, the identity
#pragma unroll 1
  for (uint32_t e = 1; e < (uint32_t)BMV_ENTRIES; e++) {
    bm_store_point(stash, (uint64_t)e * m + i, bm_tidy(acc));
    acc = G1::madd(acc, p);  // identity, equal and opposite points handled inside
  }
}

// ---- the hot kernel ----
// table: BMV_ENTRIES x m records, [e]P_i at (e - 1) m + i.  scalars: m x 8 words, or 8 words for all (stride_words = 0).
// Leading windows in which every lane of the wave still holds acc = O and a zero digit are skipped (short scalars);
// inside a window a lane with a zero digit or a flagged entry sits the addition out.
// Code object (-Rpass-analysis=kernel-resource-usage, gfx950): 205 VGPRs, no VGPR spill, 2 waves per SIMD (two workgroups
// per CU); 100 bytes of scratch per lane, the 25 accumulator limbs that k_bm_accumulate also keeps there across madd's four
// exits -- the same figures as that kernel: G1::dbl in a rolled inner loop of four beside G1::madd did not overflow the
// way k_bmm_entries' pair did.
// Measured (profiles/batch_mul_var/sweep.txt): 5.90 ms per 2^17 outputs against 5.78 ms for k_check_subgroup's chain of
// 2 948 products.
__global__ void __launch_bounds__(BM_THREADS, 2) k_bmv_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint64_t m, uint32_t stride_words,
                                                                  uint32_t scalars_mont, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < m;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = 0;  // an idle lane walks the zero scalar: no digit, no load
  if (live) {
    load_words16(scalars + i * stride_words, s, 2);
    if (scalars_mont) {  // v -> v 2^-256 mod r, fully reduced: the product of kernels/import.hpp
      const Fq::El v = Fq::mul(Fq::from_words<8>(s), Fq::from_const(EdConsts::IMPORT_MONT256));
      Fq::to_words<8>(v, s);
    }
  }
  const uint32_t carry = bmv_pack(s);
  G1XYZZ acc = G1::identity();
  if (carry) {  // (never an idle lane)
    G1Affine q;
    if (bm_load_record(table, i, q)) acc = G1::from_affine(q);
  }
#pragma unroll 1
  for (uint32_t w = 0; w < (uint32_t)BMV_WINDOWS; w++) {
    const int32_t d = bmv_next(s);
    const bool act = d != 0;
    if (__ballot(act || !G1::is_identity(acc)) == 0) continue;  // wave-uniform: 16 O + 0 = O
#pragma unroll 1
    for (int k = 0; k < BMV_WIDTH; k++) acc = G1::dbl(acc);  // O stays O
    if (act) {
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
      G1Affine q;
      if (bm_load_record(table, (uint64_t)(mag - 1u) * m + i, q)) acc = G1::madd(acc, q, d < 0);
    }
  }
  if (live) bm_store_point(stash, i, bm_tidy(acc));
}

}  // namespace
}  // namespace msm377
