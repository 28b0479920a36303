// Row commitments (msm377_g1_commit_rows*): out[i] = sum_{j<k} [s_ij]G_j over a resident set of up to MSM377_GEN_MAX
// generators, every output its own affine point (Pedersen vector commitments).  The window tables, their two build
// kernels, the signed recode, the mixed addition, the stash and the normalisation are those of kernels/batch_mul.hpp and
// kernels/batch_mul_multi.hpp; the set is ONE allocation, table j at record j * bm_table_records(c), which the one table
// builder (sequencer.hip build_mul_tables) fills pass by pass, in place.  New here:
//
//   k_cr_accumulate   THE HOT KERNEL: grid (row blocks, S).  Thread (i, g) walks the tables of segment g of the plan
//                     (commit_rows_plan.hpp: at most 16 generators) with the scalars of row i into one accumulator and
//                     leaves the partial sum at stash index g * stride + i
//   k_cr_fold         thread i adds the S partial sums of row i in order with the general addition and leaves the sum at
//                     stash index i, its own g = 0 slot; skipped for S = 1
// Every relation between the generators is legal.  Inside a segment the accumulator meets an entry that equals or opposes
// it as in k_bmm_accumulate; across segments the fold's G1::add follows the same cases: a partial of O, two equal
// partials (a doubling), two opposite ones, a sum of O from partials that are not.
// Device code; included by sequencer.hip only, after kernels/batch_mul_multi.hpp.
#pragma once
#include "../commit_rows_plan.hpp"
#include "batch_mul_multi.hpp"

namespace msm377 {
namespace {

static_assert(CR_ROW_BLOCK == BM_THREADS && CR_PASS_POINTS == BM_CHUNK && CR_SEGMENT_BASES == MSM377_MUL_MAX_BASES, "commit_rows_plan.hpp restates these for the host");

// ---- the hot kernel ----
// k_bmm_accumulate's walk over the generators j0 .. j1 - 1 of segment g = blockIdx.y, line for line and NOT a function
// shared with it or with k_bm_accumulate (kernels/batch_mul_multi.hpp records what sharing the walk did to
// k_bm_accumulate's registers): a change to one walk goes into all three.  Table j is computed from the one pointer of
// the set, so nothing is read from an argument array.  All lanes of a workgroup share g, and lane i of a pass stores at
// g * stride + i (stride: the rows of the pass rounded up to the workgroup size, so S * stride <= BM_CHUNK by the plan):
// a wave's stores are contiguous as in every batch kernel.
// Code object (profiles/commit_rows/device_code.txt): within 256 VGPRs, no register spill, no more than
// k_bmm_accumulate's 100 bytes of scratch per lane.
__global__ void __launch_bounds__(BM_THREADS, 2) k_cr_accumulate(const uint32_t* __restrict__ tables, const uint8_t* __restrict__ scalars, uint64_t n, uint32_t k, uint32_t bases_per_segment,
                                                                 uint64_t out_stride, uint64_t base_stride, uint32_t c, uint32_t scalars_mont, uint64_t stride, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < n;
  const uint32_t g = blockIdx.y, j0 = g * bases_per_segment, j1 = min(k, j0 + bases_per_segment);
  const uint32_t W = (uint32_t)bm_windows((int)c), half = 1u << (c - 1);
  const uint64_t table_words = bm_table_records(c) * BM_REC_WORDS;
  G1XYZZ acc = G1::identity();
#pragma unroll 1
  for (uint32_t j = j0; j < j1; j++) {
    uint32_t s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = 0;  // an idle lane walks the zero scalar: no digit, no load
    if (live) {
      load_words16(reinterpret_cast<const uint32_t*>(scalars + i * out_stride + (uint64_t)j * base_stride), s, 2);
      if (scalars_mont) {  // v -> v 2^-256 mod r, fully reduced: the product of kernels/import.hpp
        const Fq::El v = Fq::mul(Fq::from_words<8>(s), Fq::from_const(EdConsts::IMPORT_MONT256));
        Fq::to_words<8>(v, s);
      }
    }
    const uint32_t* __restrict__ table = tables + (uint64_t)j * table_words;
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w <= W; w++) {
      // Window w sits in the low bits: the scalar moves down by c bits per step, so bm_digit always reads window 0 and no
      // register array is indexed by a run-time value.  Row W: the final carry.
      const int32_t d = w < W ? bm_digit(s, (int)c, 0, carry) : (int32_t)carry;
#pragma unroll
      for (int q = 0; q < 7; q++) s[q] = (s[q] >> c) | (s[q + 1] << (32 - c));  // c <= 16
      s[7] >>= c;
      bool act = d != 0;
      if (__ballot(act) == 0) continue;  // wave-uniform
      const uint32_t mag = act ? (uint32_t)(d < 0 ? -d : d) : 1u;
      G1Affine q;
      act = bm_load_record(table, (uint64_t)w * half + (mag - 1u), q) && act;
      if (act) acc = G1::madd(acc, q, d < 0);
    }
  }
  if (live) bm_store_point(stash, (uint64_t)g * stride + i, bm_tidy(acc));
}

// ---- the fold ----
// Thread i < n: partial 0 + partial 1 + .. + partial S - 1 of row i, in that order, by G1::add (identity, equal and
// opposite operands handled inside); the sum goes back to index i, which no other thread reads.  S - 1 general additions
// per row beside the k (W + 1) mixed ones of the walk.
__global__ void __launch_bounds__(BM_THREADS, 2) k_cr_fold(uint4* __restrict__ stash, uint64_t n, uint32_t segments, uint64_t stride) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t w[4 * BM_POINT_PIECES];
  bm_load_pieces<0, BM_POINT_PIECES>(stash, i, w);
  G1XYZZ acc = G1Dev::from_words(w);
#pragma unroll 1
  for (uint32_t g = 1; g < segments; g++) {
    bm_load_pieces<0, BM_POINT_PIECES>(stash, (uint64_t)g * stride + i, w);
    acc = G1::add(acc, G1Dev::from_words(w));
  }
  bm_store_point(stash, i, bm_tidy(acc));
}

}  // namespace
}  // namespace msm377
