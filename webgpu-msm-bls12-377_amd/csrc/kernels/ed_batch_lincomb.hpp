// k-term linear combination on Edwards-BLS12 (msm377_ed_batch_lincomb*): out[i] = sum_{j<k} [s_ij]P_ij, 1 <= k <= 8, every
// output its own 64-byte wire point and every term its own array of points and of scalars (a Schnorr check as one sum
// [s_i]G - [c_i]PK_i - R_i, both halves of a DLEQ proof, address derivation, ElGamal re-encryption).  The structure is that
// of kernels/ed_batch_lincomb2.hpp with the number of terms a run-time value: per-point tables through the stash and the
// normalisation, the signed 4-bit recode of batch_mul_var_recode.hpp, a thread per output, the doublings shared by all
// terms, the complete law and the lazy forms throughout.  The call refuses a point that is not on the curve before it
// launches anything here (sequencer.hip edbl_check_points, k_check_curve<EdCheck>).
//
//   k_edbl_table       k_edbl2_table with the pointer and the stride of a term taken from a by-value struct: a thread per
//                      (output, term of this round), [e]P, e = 1 .. 8, into the stash at ((tt * 8) + e - 1) m + i, tt the
//                      term's place in the round.  A normalisation chunk holds the tables of TWO terms of a full pass, so
//                      the k tables are built in ceil(k / 2) rounds of one launch and one
//                      normalise<EdMul>(EDBM_FORM_TABLE) each, round r into the records from r * 16 m on
//   k_edbl_accumulate  THE HOT KERNEL: k_edbl2_accumulate with a run-time k: acc = 16 acc + sum_t d_tw P_t per step --
//                      edbmv_dbl4 (29 products) and up to k EdLazy::madd_affine (7 each) from ONE site inside a rolled loop:
//                      64 x (29 + 7k) products per output against 2 304 per term for separate walks
// Where the digits live: k x 8 words per lane do not fit beside the accumulator, so the packed digits (bmv_pack) of a
// workgroup are kept in LDS, word-major -- [term][word][lane], 8 KB per term, 64 KB at k = 8 -- and a lane reads the nibble
// of (term, window) from its own column: consecutive lanes, consecutive banks.  Each lane reads only what it wrote itself,
// so the kernel has no barrier.  The k final carries are one bit mask in a register.
// A pass is EDBL_PASS = 2^16 outputs whatever k: 2^16 threads are one wave per SIMD already (README, pairwise call), so the
// tables of a pass are k x 2^19 records, in an allocation of the call's own (EdBatchMulState::lincomb_table).
// Device code; included by sequencer.hip only (after kernels/ed_batch_lincomb2.hpp).
#pragma once
#include "ed_batch_lincomb2.hpp"

namespace msm377 {
namespace {

constexpr uint32_t EDBL_MAX_TERMS = 8;                                   // MSM377_LINCOMB_MAX_TERMS
constexpr uint32_t EDBL_ROUND_TERMS = 2;                                 // tables of a full pass per normalisation chunk
constexpr uint64_t EDBL_PASS = BM_CHUNK / (EDBL_ROUND_TERMS * BMV_ENTRIES);  // 2^16 outputs
constexpr uint32_t EDBL_TERM_LDS_WORDS = 8 * BM_THREADS;                 // the packed digits of one term of a workgroup
static_assert(EDBL_PASS * EDBL_ROUND_TERMS * BMV_ENTRIES == BM_CHUNK && EDBL_PASS % BM_THREADS == 0, "a round's two tables are one normalisation chunk");
static_assert(EDBL_MAX_TERMS * EDBL_TERM_LDS_WORDS * 4 == 65536, "the digits of eight terms are the 64 KB a workgroup gets without opting in");
static_assert(EDBL_MAX_TERMS * 4 == 32, "one nibble per term in one register");
static_assert((uint64_t)EDBL_MAX_TERMS * BMV_ENTRIES * EDBL_PASS <= UINT32_MAX, "a record index of the tables is 32 bits");

// The terms of one pass, by value: the pointers are the pass's own (already moved to its first output).
struct EdblTerms {
  const uint8_t* points[EDBL_MAX_TERMS];
  const uint32_t* scalars[EDBL_MAX_TERMS];
  uint32_t point_stride[EDBL_MAX_TERMS];  // bytes: 64, or 0 (record 0 for every i)
  uint32_t scalar_words[EDBL_MAX_TERMS];  // words: 8, or 0 (one scalar for all: only its 32 bytes are read)
};

// blockIdx.y is the term's place in the round: term first_term + blockIdx.y.  Every value is canonical (Fq::mul / add /
// sub), as the normalisation asks of the stash.
__global__ void __launch_bounds__(BM_THREADS) k_edbl_table(const EdblTerms terms, uint32_t first_term, uint64_t m, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (i >= m) return;
  const uint32_t term = first_term + blockIdx.y;
  const uint8_t* rec = terms.points[term] + i * terms.point_stride[term];
  const uint64_t at = (uint64_t)blockIdx.y * BMV_ENTRIES * m + i;
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

// ---- the hot kernel ----
// table: k x 8 x m records, [e]P_ti at ((t * 8) + e - 1) m + i.  Dynamic LDS: k x EDBL_TERM_LDS_WORDS words.  The walk is
// k_edbl2_accumulate's: `started` (the lane has left the start value O), the wave-uniform skip of leading steps in which no
// lane has started and every digit of every term is zero, a lane with a zero digit sitting that addition out, and the k
// final carries as step 64 of the same loop, additions to O without doublings.  A step's k digits are gathered as biased
// nibbles in ONE register (nibble t = digit + 7; a term at or above k, or a zero digit: 7), so "every digit zero" is one
// compare and the rolled loop over the terms holds ONE copy of the addition.  An idle lane walks zero scalars: no digit,
// no load.  With every scalar 1 only the last step runs: the plain sum of the k points.  The accumulator is a lazy point
// throughout: up to eight additions in a row read what the one before returned, and the next step's first dbl_nt what the
// last returned, with no canon between them (te377.hpp; tools/check_lazy_bounds.py replays the chain of
// MSM377_LINCOMB_MAX_TERMS), and it leaves the kernel canonical (Fq::canon).
// Code object (profiles/ed_batch_lincomb/device_code.txt).
__global__ void __launch_bounds__(BM_THREADS, 4) k_edbl_accumulate(const uint32_t* __restrict__ table, const EdblTerms terms, uint32_t k, uint64_t m, uint4* __restrict__ stash) {
  extern __shared__ uint32_t edbl_digits[];  // [term][word][lane]
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + lane;
  const bool live = i < m;
  uint32_t carries = 0;
#pragma unroll 1
  for (uint32_t t = 0; t < k; t++) {
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = 0;
    if (live) load_words16(terms.scalars[t] + i * terms.scalar_words[t], s, 2);
    carries |= bmv_pack(s) << t;
#pragma unroll
    for (int j = 0; j < 8; j++) edbl_digits[t * EDBL_TERM_LDS_WORDS + j * BM_THREADS + lane] = s[j];
  }
  constexpr uint32_t ALL_ZERO = 0x77777777u;  // BMV_BIAS in every nibble
  EdLazy::Ext acc = EdLazy::identity();
  bool started = false;
#pragma unroll 1
  for (int w = BMV_WINDOWS; w >= 0; w--) {  // step 64 is the carries': the digits of 2^256, on acc = O
    uint32_t nib = ALL_ZERO;
    if (w == BMV_WINDOWS) {
#pragma unroll 1
      for (uint32_t t = 0; t < k; t++) nib += ((carries >> t) & 1u) << (4 * t);
    } else {
      const uint32_t at = (uint32_t)(w >> 3) * BM_THREADS + lane, shift = 4u * ((uint32_t)w & 7u);
#pragma unroll 1
      for (uint32_t t = 0; t < k; t++) {
        const uint32_t n4 = (edbl_digits[t * EDBL_TERM_LDS_WORDS + at] >> shift) & 15u;
        nib = (nib & ~(15u << (4 * t))) | (n4 << (4 * t));
      }
    }
    started |= nib != ALL_ZERO;
    if (__ballot(started) == 0) continue;  // wave-uniform: 16 O + 0 + ... + 0 = O
    if (w != BMV_WINDOWS) acc = edbmv_dbl4(acc);
#pragma unroll 1
    for (uint32_t t = 0; t < k; t++) {
      const int32_t d = (int32_t)((nib >> (4 * t)) & 15u) - BMV_BIAS;
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
