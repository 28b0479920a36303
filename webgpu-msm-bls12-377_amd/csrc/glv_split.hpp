// The arithmetic of the GLV front end, k -> (k1, k2) with k = k1 + LAMBDA k2, and the signed digits of a half: shared by
// k_decompose_glv (kernels/decompose.hpp, device) and the host (tests/native/glv_split_shim.cpp compiles it with g++ and
// compares it with the model of tests/stage_model.py and with Python's divmod).  Plain integer code, no device intrinsics;
// the kernel keeps its loads, its stores and its atomicOr.
#pragma once
#include <stdint.h>

#include "consts_gen.hpp"

#ifndef MSM_HD  // as in common.hpp and field29.hpp, for translation units that include this header alone
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSM_HD __host__ __device__ __forceinline__
#else
#define MSM_HD inline __attribute__((always_inline))
#endif
#endif

namespace msm377 {

// out[0..NA+NB) = a * b on 32-bit words (schoolbook, carries resolved per row).
template <int NA, int NB_>
MSM_HD void mul_words(const uint32_t* a, const uint32_t* b, uint32_t* out) {
#pragma unroll
  for (int k = 0; k < NA + NB_; k++) out[k] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB_; j++) {
      const uint64_t t = (uint64_t)a[i] * b[j] + out[i + j] + carry;
      out[i + j] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
    out[i + NB_] = carry;
  }
}

// The Barrett quotient of a 256-bit k by LAMBDA (MU = floor(2^384 / LAMBDA)): q = floor(k MU / 2^384), the quotient or
// one less, and rem = k - q LAMBDA on five words, in [0, 2 LAMBDA).
MSM_HD void glv_quotient(const uint32_t* k /* 8 */, uint32_t* q /* 5 */, uint32_t* rem /* 5 */) {
  uint32_t prod[17];
  mul_words<8, 9>(k, GlvConsts::MU, prod);
#pragma unroll
  for (int j = 0; j < 5; j++) q[j] = prod[12 + j];  // floor(k MU / 2^384): the quotient or one less
  uint32_t ql[9];
  mul_words<5, 4>(q, GlvConsts::LAMBDA, ql);
  uint32_t borrow = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint64_t d = (uint64_t)k[j] - ql[j] - borrow;
    rem[j] = (uint32_t)d;
    borrow = (uint32_t)(d >> 32) & 1u;
  }
}

// rem in [0, 2 LAMBDA): one conditional correction, rem -= LAMBDA and q += 1 when rem >= LAMBDA.  Returns whether it was
// taken (for exact multiples of LAMBDA only: tests/test_stage_model_host.py).
MSM_HD bool glv_correct(uint32_t* q /* 5 */, uint32_t* rem /* 5 */) {
  uint32_t sub[5];
  uint32_t borrow = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint64_t d = (uint64_t)rem[j] - (j < 4 ? GlvConsts::LAMBDA[j] : 0u) - borrow;
    sub[j] = (uint32_t)d;
    borrow = (uint32_t)(d >> 32) & 1u;
  }
  if (!borrow) {
#pragma unroll
    for (int j = 0; j < 5; j++) rem[j] = sub[j];
    uint32_t c = 1;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const uint64_t t = (uint64_t)q[j] + c;
      q[j] = (uint32_t)t;
      c = (uint32_t)(t >> 32);
    }
  }
  return !borrow;
}

// The digit chains read four words of each half: a fifth word in use is out of the GLV range (non-zero: bad).
MSM_HD uint32_t glv_fifth_words(const uint32_t* q, const uint32_t* rem) { return q[4] | rem[4]; }

// One step of the digit chain over a 128-bit value v < 2^127: window `win` of eight signed 16-bit digits, the top one
// non-negative.  Returns the digit as stored (biased by 2^15); `carry` goes into the next window, `bad` is raised if the
// value does not fit (the top window reaches 2^15).
MSM_HD uint32_t recode128_step(const uint32_t* v, uint32_t win, uint32_t& carry, uint32_t& bad) {
  const uint32_t limb = (v[win >> 1] >> (16 * (win & 1))) & 0xffffu;
  const uint32_t t = limb + carry;
  carry = (win < 7 && t >= 32768u) ? 1u : 0u;
  if (win == 7 && t >= 32768u) bad = 1u;
  return (t + 32768u) & 0xffffu;
}

}  // namespace msm377
