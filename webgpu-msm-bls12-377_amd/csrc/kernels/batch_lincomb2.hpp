// Pairwise linear combination (msm377_g1_batch_lincomb2*): out[i] = [a_i]P_i + [b_i]Q_i, every output its own affine point
// (an inner-product basis fold G'_i = [x^-1]G_i + [x]G_{i+n/2}, an SRS update with a blinding term, a random linear
// combination of two key vectors, plain P_i + Q_i).  Nothing in the reference corresponds to this; the variable-base call
// (kernels/batch_mul_var.hpp) lends k_bmv_table, the nibble packing and -- through it -- the fixed-base call's stash,
// normalisation and table record.
//
//   k_bmv_table       launched twice per pass: [1..8]P_i into the stash at (e - 1) m + i, [1..8]Q_i at (8 + e - 1) m + i
//                     (the second launch's stash pointer is 8 m pieces further on); ONE normalise<G1Mul>(BM_FORM_TABLE) over
//                     the 16 m entries makes 128-byte affine records of both halves
//   k_bl2_accumulate  THE HOT KERNEL: a thread per output walks the signed 4-bit digits of BOTH scalars from the top
//                     (batch_mul_var_recode.hpp) and shares the doublings: acc = 16 acc + da_w P + db_w Q -- four doublings
//                     of 9 products and two mixed additions of 10 per 4 bits, 64 x 56 = 3 584 products per output against
//                     2 x 2 944 = 5 888 for two variable-base walks (and an addition that nothing offers)
// A pass is BL2_PASS = 2^16 pairs: its 16 x 2^16 table entries are exactly one normalisation chunk, in the var call's
// ctx->bm.var_table.
//
// Every curve point is a legal input in either array, mixed freely within one wave, and so is every relation between the
// two (Q = P, Q = -P, Q a multiple of P, a result of O with P != +-Q): the two additions of a step are two madd's one
// after the other, each with its identity / equal / opposite exits, never a precomputed P + Q.  Exits as in
// k_bmv_accumulate: a zero digit or a flagged entry sits the addition out.
// Device code; included by sequencer.hip only (after kernels/batch_mul_var.hpp).
#pragma once
#include "batch_mul_var.hpp"

namespace msm377 {
namespace {

constexpr uint32_t BL2_TERMS = 2;
constexpr uint64_t BL2_PASS = BM_CHUNK / (BL2_TERMS * BMV_ENTRIES);  // 2^16 pairs: 256 CUs x one 256-thread workgroup
static_assert(BL2_PASS * BL2_TERMS * BMV_ENTRIES == BM_CHUNK && BL2_PASS % BM_THREADS == 0, "a pass's two tables are one normalisation chunk");

// One scalar of lane i as packed digits (bmv_pack); returns the final carry.  stride_words: 8, or 0 (one scalar for all:
// only its 32 bytes are read).  An idle lane walks the zero scalar: no digit, no load.
__device__ __forceinline__ uint32_t bl2_load_scalar(const uint32_t* __restrict__ scalars, uint64_t i, uint32_t stride_words, uint32_t scalars_mont, bool live, uint32_t* s) {
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = 0;
  if (live) {
    load_words16(scalars + i * stride_words, s, 2);
    if (scalars_mont) {  // v -> v 2^-256 mod r, fully reduced: the product of kernels/import.hpp
      const Fq::El v = Fq::mul(Fq::from_words<8>(s), Fq::from_const(EdConsts::IMPORT_MONT256));
      Fq::to_words<8>(v, s);
    }
  }
  return bmv_pack(s);
}

// ---- the hot kernel ----
// table: 16 x m records, [e]P_i at (e - 1) m + i and [e]Q_i at (8 + e - 1) m + i.  The two final carries are a leading
// 65th step whose digits are the carries (entry [1] of each table; the four doublings of acc = O are harmless), so there
// is ONE madd site, inside a rolled two-turn loop over the terms: a separate from_affine / madd in front of the loop cost
// 256 VGPRs with 52 spilled.  A step in which every lane of the wave holds acc = O and two zero digits is skipped: with
// a = b = 1 only the last step runs (plain batch addition), short scalars pay for their length.
// Code object (-Rpass-analysis=kernel-resource-usage, gfx950): 217 VGPRs (k_bmv_accumulate's 205 and the second packed
// scalar), no VGPR spill, 2 waves per SIMD (two workgroups per CU); 100 bytes of scratch per lane, the 25 accumulator limbs
// that k_bmv_accumulate also keeps there across madd's four exits.
__global__ void __launch_bounds__(BM_THREADS, 2) k_bl2_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t m,
                                                                  uint32_t a_stride_words, uint32_t b_stride_words, uint32_t scalars_mont, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < m;
  uint32_t sa[8], sb[8];
  const uint32_t carry_a = bl2_load_scalar(a, i, a_stride_words, scalars_mont, live, sa);
  const uint32_t carry_b = bl2_load_scalar(b, i, b_stride_words, scalars_mont, live, sb);
  G1XYZZ acc = G1::identity();
#pragma unroll 1
  for (uint32_t w = 0; w <= (uint32_t)BMV_WINDOWS; w++) {
    int32_t da = (int32_t)carry_a, db = (int32_t)carry_b;  // step 0: s = carry 2^256 + ..
    if (w) {
      da = bmv_next(sa);
      db = bmv_next(sb);
    }
    if (__ballot(da != 0 || db != 0 || !G1::is_identity(acc)) == 0) continue;  // wave-uniform: 16 O + 0 + 0 = O
#pragma unroll 1
    for (int k = 0; k < BMV_WIDTH; k++) acc = G1::dbl(acc);  // O stays O
#pragma unroll 1
    for (uint32_t t = 0; t < BL2_TERMS; t++) {
      const int32_t d = t ? db : da;
      if (d != 0) {  // (never an idle lane)
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
        G1Affine q;
        if (bm_load_record(table, (uint64_t)(t * BMV_ENTRIES + mag - 1u) * m + i, q)) acc = G1::madd(acc, q, d < 0);
      }
    }
  }
  if (live) bm_store_point(stash, i, bm_tidy(acc));
}

}  // namespace
}  // namespace msm377
