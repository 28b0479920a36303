// Pairwise linear combination on Edwards-BLS12 (msm377_ed_batch_lincomb2*): out[i] = [a_i]P_i + [b_i]Q_i, every output its
// own 64-byte wire point (Schnorr verification R_i = [s_i]G + [c_i]PK_i, ElGamal decryption and re-randomisation, plain
// P_i + Q_i).  The structure is that of kernels/batch_lincomb2.hpp -- two per-point tables through the stash and ONE
// normalisation, the signed 4-bit recode of batch_mul_var_recode.hpp, a thread per output, the doublings shared by both
// terms -- on the complete law and the lazy forms of kernels/ed_batch_mul_var.hpp: no identity / equal / opposite exits, no
// flags, every curve point a legal input in either array and every relation between the two (Q = +-P, Q = [m]P, a sum of O
// from two terms that are not O) followed through by the law itself.  The call refuses a point that is not on the curve
// before it launches anything here (sequencer.hip edbl2_check_points, k_check_curve<EdCheck>).
//
//   k_edbl2_table       a thread per (pair, term): wire x || y to Montgomery form, then [e]P_i, e = 1 .. 8, into the stash at
//                       (e - 1) m + i and [e]Q_i at (8 + e - 1) m + i with the canonical Ed:: formulas -- one dbl, six madd;
//                       an array of stride 0 is ONE point, read by every thread of its term.  ONE
//                       normalise<EdMul>(EDBM_FORM_TABLE) over the 16 m entries makes 128-byte records of both halves
//   k_edbl2_accumulate  THE HOT KERNEL: a thread per output walks the 64 signed digits of BOTH scalars from the top into ONE
//                       lazy accumulator: acc = 16 acc + da_w P + db_w Q -- edbmv_dbl4 (three T-less lazy doublings of 7
//                       products, one full one of 8) and two EdLazy::madd_affine (7): 64 x 43 = 2 752 products per output
//                       against 2 x 2 304 for two variable-base walks (and an addition that nothing offers)
// A pass is EDBL2_PASS = 2^16 pairs: its 16 x 2^16 table entries are exactly one normalisation chunk, in ctx->bm.var_table.
// Device code; included by sequencer.hip only (after kernels/ed_batch_mul_var.hpp).
#pragma once
#include "ed_batch_mul_var.hpp"

namespace msm377 {
namespace {

constexpr uint32_t EDBL2_TERMS = 2;
constexpr uint64_t EDBL2_PASS = BM_CHUNK / (EDBL2_TERMS * BMV_ENTRIES);  // 2^16 pairs: 256 CUs x one 256-thread workgroup
static_assert(EDBL2_PASS * EDBL2_TERMS * BMV_ENTRIES == BM_CHUNK && EDBL2_PASS % BM_THREADS == 0, "a pass's two tables are one normalisation chunk");

// blockIdx.y is the term: 0 reads p, 1 reads q.  stride 64, or 0: record 0 for every i.  Every value is canonical
// (Fq::mul / add / sub), as the normalisation asks of the stash.
__global__ void __launch_bounds__(BM_THREADS) k_edbl2_table(const uint8_t* __restrict__ p, const uint8_t* __restrict__ q, uint32_t p_stride, uint32_t q_stride, uint64_t m,
                                                            uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (i >= m) return;
  const uint32_t term = blockIdx.y;
  const uint8_t* rec = term ? q + i * q_stride : p + i * p_stride;
  const uint64_t at = (uint64_t)term * BMV_ENTRIES * m + i;
  uint32_t raw[16];
  load_words16(reinterpret_cast<const uint32_t*>(rec), raw, 4);
  Ed::Ext acc;
  acc.x = Fq::to_mont(Fq::from_words<8>(raw));
  acc.y = Fq::to_mont(Fq::from_words<8>(raw + 8));
  acc.t = Fq::mul(acc.x, acc.y);
  acc.z = Fq::one();
  const Ed::Base b = Ed::make_base(acc.x, acc.y);
  edbm_store_point(stash, at, acc.x, acc.y, acc.t, acc.z);
  acc = Ed::dbl(acc);
#pragma unroll 1
  for (uint32_t e = 1; e < (uint32_t)BMV_ENTRIES; e++) {
    edbm_store_point(stash, (uint64_t)e * m + at, acc.x, acc.y, acc.t, acc.z);
    acc = Ed::madd(acc, b);
  }
}

// One scalar of lane i as packed digits (bmv_pack); returns the final carry.  stride_words: 8, or 0 (one scalar for all:
// only its 32 bytes are read).  An idle lane walks the zero scalar: no digit, no load.
__device__ __forceinline__ uint32_t edbl2_load_scalar(const uint32_t* __restrict__ scalars, uint64_t i, uint32_t stride_words, bool live, uint32_t* s) {
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = 0;
  if (live) load_words16(scalars + i * stride_words, s, 2);
  return bmv_pack(s);
}

// ---- the hot kernel ----
// table: 16 x m records, [e]P_i at (e - 1) m + i and [e]Q_i at (8 + e - 1) m + i.  a, b: m x 8 words each, or 8 words for
// all (stride 0), read as integers and not reduced.  The walk is k_edbmv_accumulate's with two digits per step: `started`
// (the lane has left the start value O), the wave-uniform skip of leading steps in which no lane has started and every
// digit of both scalars is zero, a lane with a zero digit sitting that addition out, and the two final carries as step 64 of
// the same loop, additions to O without doublings -- so the kernel holds ONE copy of the addition, inside a rolled two-turn
// loop over the terms.  With a = b = 1 only the last step runs: plain P_i + Q_i.  The accumulator is a lazy point
// throughout: the second addition of a step reads what the first returned, and the next step's first dbl_nt what the
// second returned, with no canon between them (te377.hpp; tools/check_lazy_bounds.py replays both), and it leaves the
// kernel canonical (Fq::canon).
// Code object (profiles/ed_batch_lincomb2/device_code.txt).
__global__ void __launch_bounds__(BM_THREADS, 4) k_edbl2_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t m,
                                                                    uint32_t a_stride_words, uint32_t b_stride_words, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < m;
  uint32_t sa[8], sb[8];
  const uint32_t carry_a = edbl2_load_scalar(a, i, a_stride_words, live, sa);
  const uint32_t carry_b = edbl2_load_scalar(b, i, b_stride_words, live, sb);
  EdLazy::Ext acc = EdLazy::identity();
  bool started = false;
#pragma unroll 1
  for (int w = BMV_WINDOWS; w >= 0; w--) {  // step 64 is the carries': the digits of 2^256, on acc = O
    int32_t da = (int32_t)carry_a, db = (int32_t)carry_b;
    if (w != BMV_WINDOWS) {
      da = bmv_next(sa);
      db = bmv_next(sb);
    }
    started |= (da | db) != 0;
    if (__ballot(started) == 0) continue;  // wave-uniform: 16 O + 0 + 0 = O
    if (w != BMV_WINDOWS) acc = edbmv_dbl4(acc);
#pragma unroll 1
    for (uint32_t t = 0; t < EDBL2_TERMS; t++) {
      const int32_t d = t ? db : da;
      if (d != 0) {  // (never an idle lane)
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
        acc = EdLazy::madd_affine(acc, EdDev::load_base(table, (uint32_t)((uint64_t)(t * BMV_ENTRIES + mag - 1u) * m + i)), d < 0);
      }
    }
  }
  if (live) edbm_store_point(stash, i, Fq::canon(acc.x), Fq::canon(acc.y), Fq::canon(acc.t), Fq::canon(acc.z));
}

}  // namespace
}  // namespace msm377
