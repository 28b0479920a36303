// Multi-base batch multiplication (msm377_g1_batch_mul_multi*): out[i] = sum_{j<k} [s_ij]B_j for k <= 16 fixed bases and
// n rows of scalars, every output its own affine point (Pedersen commitments [m_i]G + [r_i]H, the second half of an
// ElGamal ciphertext, a hiding SRS).  The window tables, the signed recode, the mixed addition and the normalisation are
// those of kernels/batch_mul.hpp; new here:
//
// These two are the build kernels of EVERY G1 window table -- the single-base table (one base), these slots, the generator
// set of the row commitments -- under the one table builder of sequencer.hip (build_mul_tables):
//   k_bmm_row_bases   workgroup b, thread w: [2^(c w)]B_b for every base a build is missing, ONE launch -- the 256
//                     dependent doublings of the last row are paid once per build, not once per base
//   k_bmm_entries     thread (b, w, d) over the concatenated records of the missing tables, cut into passes of at most
//                     BM_CHUNK records wherever the cut falls (two c = 16 tables are 2 records over a chunk)
//   k_bmm_accumulate  THE HOT KERNEL: a thread per output walks table 0 with s_i0, table 1 with s_i1, .. into ONE
//                     accumulator; one normalisation for the sum instead of k of them and k - 1 additions of affine points
// Every relation between the bases is legal (B_1 = +-B_0, B_1 = [m]B_0, bases of small order, a sum of O with no term O):
// the accumulator meets an entry of table j that equals or opposes it exactly as it meets such an entry of its own table
// for a base of small order, and G1::madd follows all of it.
// Device code; included by sequencer.hip only, after kernels/batch_mul.hpp.
#pragma once
#include "batch_mul.hpp"

namespace msm377 {
namespace {

// The tables of a call, one pointer per base position: the slots of BatchMulMultiState are separate allocations.  Passed
// by value, so the kernel reads pointer j from its argument segment (a scalar load at a run-time offset: no register
// array, no scratch).
struct BmmTables {
  const uint32_t* t[MSM377_MUL_MAX_BASES];
};

// ---- table build, every missing slot at once ----
// bases_wire: 96 bytes per missing base; row base w of base b goes to stash index b (W + 1) + w.  Thread w <= W: 256
// dependent doublings for the last row, on one wave, once per build: the longest launch of a build
// (profiles/batch_mul/build_trace.txt).
__global__ void __launch_bounds__(64) k_bmm_row_bases(const uint32_t* __restrict__ bases_wire, uint32_t c, uint4* __restrict__ stash) {
  const uint32_t w = threadIdx.x, W = (uint32_t)bm_windows((int)c), b = blockIdx.x;
  if (w > W) return;
  uint32_t raw[24];
  load_words16(bases_wire + (size_t)b * 24, raw, 6);
  G1Affine p;
  p.x = Fp::to_mont(Fp::from_words<12>(raw));
  p.y = Fp::to_mont(Fp::from_words<12>(raw + 12));
  G1XYZZ acc = G1::from_affine(p);
#pragma unroll 1
  for (uint32_t k = 0; k < c * w; k++) acc = G1::dbl(acc);  // O stays O; Y = 0 (order 2) gives ZZ = 0
  bm_store_point(stash, (uint64_t)b * (W + 1) + w, bm_tidy(acc));
}

// Record g = first + u of the concatenation, u < count <= BM_CHUNK: table b = g / records, entry t = g mod records of it
// (thread t < W 2^(c-1) + 1: entry d = (t mod 2^(c-1)) + 1 of row w = t / 2^(c-1); t = W 2^(c-1) is entry 1 of row W),
// from the row bases of base b; the point goes to stash index u.  One workgroup per CU: G1::dbl and G1::madd side by side
// in one loop want more than the 256 registers that two would leave (182 of them spilled); the kernel runs once per build.
__global__ void __launch_bounds__(BM_THREADS) k_bmm_entries(const uint32_t* __restrict__ row_bases, uint32_t c, uint64_t first, uint64_t count, uint4* __restrict__ stash) {
  const uint64_t u = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (u >= count) return;
  const uint64_t records = bm_table_records(c), g = first + u;
  const uint32_t b = (uint32_t)(g / records), W = (uint32_t)bm_windows((int)c);
  const uint64_t t = g - (uint64_t)b * records;
  const uint32_t w = (uint32_t)(t >> (c - 1)), d = ((uint32_t)t & ((1u << (c - 1)) - 1u)) + 1u;
  G1Affine q;
  const bool finite = bm_load_record(row_bases, (uint64_t)b * (W + 1) + w, q);
  G1XYZZ acc = G1::identity();
  if (finite) {
#pragma unroll 1
    for (int bit = 31 - __clz((int)d); bit >= 0; bit--) {
      acc = G1::dbl(acc);
      if ((d >> bit) & 1u) acc = G1::madd(acc, q);  // identity, equal and opposite points handled inside
    }
  }
  bm_store_point(stash, u, bm_tidy(acc));
}

// ---- the hot kernel ----
// k_bm_accumulate with a rolled loop over the bases around its walk: the budget is that kernel's plus the loop counter,
// the two strides and the scalar's address.  s_ij is the 32 bytes at scalars + i out_stride + j base_stride (both byte
// counts, multiples of 32: row-major, column-major and padded rows are all this).  The accumulator is carried from one
// table into the next, so "acc = +-entry" and "acc = O in mid-walk" happen between bases as they do within one.
// The walk is k_bm_accumulate's, line for line, and NOT one function the two kernels call: with the walk moved into a
// __forceinline__ function k_bm_accumulate came out of the compiler with 206 VGPRs and 63 spilled SGPRs instead of 205 and
// 60 (9 331 instead of 9 381 instructions), so that kernel stays as it was and a change to either walk goes into both.
// Code object (profiles/batch_mul_multi/device_code.txt): within 256 VGPRs, no register spill, k_bm_accumulate's 100
// bytes of scratch per lane.
__global__ void __launch_bounds__(BM_THREADS, 2) k_bmm_accumulate(const BmmTables tables, const uint8_t* __restrict__ scalars, uint64_t n, uint32_t k, uint64_t out_stride,
                                                                  uint64_t base_stride, uint32_t c, uint32_t scalars_mont, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < n;
  const uint32_t W = (uint32_t)bm_windows((int)c), half = 1u << (c - 1);
  G1XYZZ acc = G1::identity();
#pragma unroll 1
  for (uint32_t j = 0; j < k; j++) {
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
    const uint32_t* __restrict__ table = tables.t[j];
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
  if (live) bm_store_point(stash, i, bm_tidy(acc));
}

}  // namespace
}  // namespace msm377
