// Row commitments on Edwards-BLS12 (msm377_ed_commit_rows*): out[i] = sum_{j<k} [s_ij]G_j over a resident set of up to
// MSM377_GEN_MAX generators, every output its own 64-byte wire point (Pedersen / BHP-style hashes and vector commitments
// over this curve's generators).  The window tables, their two build kernels, the signed recode, the lazy mixed addition,
// the stash and the normalisation are those of kernels/ed_batch_mul.hpp; the cut of a call is G1's
// (commit_rows_plan.hpp); the set is ONE allocation, table j at record j * bm_table_records(c), which the one table
// builder (sequencer.hip build_mul_tables) fills pass by pass, in place.  New here:
//
//   k_edcr_accumulate  THE HOT KERNEL: grid (row blocks, S).  Thread (i, g) walks the tables of segment g of the plan (at
//                      most 16 generators) with the scalars of row i into one lazy accumulator and leaves the canonical
//                      partial sum at stash index g * stride + i
//   k_edcr_fold        grouped fold, two levels at most: thread (i, h) adds the at most CR_FOLD_GROUP partial sums
//                      first, first + step, .. of group h of row i with the canonical Ed::add and leaves the sum in the
//                      group's FIRST slot.  Level 1 (step 1) folds segments 16 h .. 16 h + 15 into segment 16 h; for
//                      S > 16 level 2 (step 16) folds segments 0, 16, 32, .. into segment 0.  S <= 16: one launch; S = 1: none
// The addition law is complete on the curve: a partial or a group sum that is the identity, two equal ones, two opposite
// ones and a sum of O from terms that are not take the one formula, and every Z stays non-zero (the generators were
// checked on the device before the tables were built).  Addition is associative and the outputs are normalised, so the
// order of the fold does not show in the bytes.
// Device code; included by sequencer.hip only, after kernels/ed_batch_mul.hpp.
#pragma once
#include "../commit_rows_plan.hpp"
#include "ed_batch_mul.hpp"

namespace msm377 {
namespace {

constexpr uint32_t CR_FOLD_GROUP = 16;  // partial sums one fold thread adds
static_assert(MSM377_GEN_MAX / CR_SEGMENT_BASES <= CR_FOLD_GROUP * CR_FOLD_GROUP, "two fold levels reach segment 0 from every segment");

// ---- the hot kernel ----
// k_edbm_accumulate's walk over the generators j0 .. j1 - 1 of segment g = blockIdx.y, line for line and NOT a function
// shared with it (as the G1 trio of kernels/commit_rows.hpp: a change to one walk goes into the other).  Two things
// differ: table j is computed from the one pointer of the set, so nothing is read from an argument array; and the j
// range is the segment's.  The wave-uniform skip of all-zero windows stays: it is what makes short scalars cheap.  The
// accumulator starts as the identity, takes EdLazy::madd_affine(acc, record, sign) only and leaves through Fq::canon:
// the operand pattern of k_edbm_accumulate, which tools/check_lazy_bounds.py already replays -- no new link in the
// bound chain.  All lanes of a workgroup share g, and lane i of a pass stores at g * stride + i (stride: the rows of the
// pass rounded up to the workgroup size, so S * stride <= BM_CHUNK by the plan): a wave's stores are contiguous.
// Code object (profiles/ed_commit_rows/device_code.txt): four waves per SIMD, no scratch, no spill.
__global__ void __launch_bounds__(BM_THREADS, 4) k_edcr_accumulate(const uint32_t* __restrict__ tables, const uint8_t* __restrict__ scalars, uint64_t n, uint32_t k, uint32_t bases_per_segment,
                                                                   uint64_t out_stride, uint64_t base_stride, uint32_t c, uint64_t stride, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < n;
  const uint32_t g = blockIdx.y, j0 = g * bases_per_segment, j1 = min(k, j0 + bases_per_segment);
  const uint32_t W = (uint32_t)bm_windows((int)c), half = 1u << (c - 1);
  const uint64_t table_words = bm_table_records(c) * BM_REC_WORDS;
  EdLazy::Ext acc = EdLazy::identity();
#pragma unroll 1
  for (uint32_t j = j0; j < j1; j++) {
    uint32_t s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = 0;  // an idle lane walks the zero scalar: no digit, no load
    if (live) load_words16(reinterpret_cast<const uint32_t*>(scalars + i * out_stride + (uint64_t)j * base_stride), s, 2);
    const uint32_t* __restrict__ table = tables + (uint64_t)j * table_words;
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w <= W; w++) {
      // As in k_bmm_accumulate: the scalar moves down by c bits per step, bm_digit always reads window 0.  Row W: the carry.
      const int32_t d = w < W ? bm_digit(s, (int)c, 0, carry) : (int32_t)carry;
#pragma unroll
      for (int q = 0; q < 7; q++) s[q] = (s[q] >> c) | (s[q + 1] << (32 - c));  // c <= 16
      s[7] >>= c;
      const bool act = d != 0;
      if (__ballot(act) == 0) continue;  // wave-uniform
      const uint32_t mag = act ? (uint32_t)(d < 0 ? -d : d) : 1u;
      const EdLazy::ABase q = EdDev::load_base(table, (uint32_t)((uint64_t)w * half + (mag - 1u)));
      if (act) acc = EdLazy::madd_affine(acc, q, d < 0);
    }
  }
  if (live) edbm_store_point(stash, (uint64_t)g * stride + i, Fq::canon(acc.x), Fq::canon(acc.y), Fq::canon(acc.t), Fq::canon(acc.z));
}

// ---- the fold ----
__device__ __forceinline__ Ed::Ext edcr_load_point(const uint4* __restrict__ stash, uint64_t idx) {
  uint32_t w[4 * EDBM_POINT_PIECES];
  bm_load_pieces<0, EDBM_POINT_PIECES>(stash, idx, w);
  Ed::Ext p;
  p.x = get9(w);
  p.y = get9(w + 9);
  p.t = get9(w + 18);
  p.z = get9(w + 27);
  return p;
}

// Grid (row blocks, groups).  Thread (i, h), i < n: segments first = h * step * CR_FOLD_GROUP, first + step, .. (at most
// CR_FOLD_GROUP of them, below `segments`) of row i, added in that order by the canonical Ed::add; the sum goes back to
// segment `first`.  Within a launch every slot is read by exactly one thread, and a thread writes only the first slot it
// read: no two threads of a launch touch the same slot.  A group of ONE segment is left as it is.
__global__ void __launch_bounds__(BM_THREADS, 2) k_edcr_fold(uint4* __restrict__ stash, uint64_t n, uint32_t segments, uint32_t step, uint64_t stride) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const uint32_t first = blockIdx.y * step * CR_FOLD_GROUP;
  if (i >= n || first >= segments) return;
  const uint32_t last = min(segments, first + step * CR_FOLD_GROUP);  // exclusive
  if (first + step >= last) return;
  Ed::Ext acc = edcr_load_point(stash, (uint64_t)first * stride + i);
#pragma unroll 1
  for (uint32_t g = first + step; g < last; g += step) acc = Ed::add(acc, edcr_load_point(stash, (uint64_t)g * stride + i));
  edbm_store_point(stash, (uint64_t)first * stride + i, acc.x, acc.y, acc.t, acc.z);
}

}  // namespace
}  // namespace msm377
