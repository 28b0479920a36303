// Variable-base batch multiplication (msm377_g1_batch_mul_var*): the scalar of one output as the hot kernel walks it.
// Shared by kernels/batch_mul_var.hpp and the stand-alone test program tests/native/batch_mul_var_host.cpp, and by
// nothing else (the host twin, batch_mul_var_host.hpp, walks the plain bits).  No device code of its own.
//
// The walk is left to right, bm_digit (batch_mul_recode.hpp) carries from the low end: so the 64 signed 4-bit digits
// d_w in -7 .. 8 are computed first and packed as nibbles d_w + 7 (0 .. 15) into the scalar's own eight words, window w
// at bits 4w .. 4w + 3, with the final carry beside them:
//     s = sum_w d_w 16^w + carry 2^256.
// The walk then reads the top nibble and moves the array UP four bits per step (bmv_next), the way k_bm_accumulate moves
// its scalar down: no register array is indexed by a run-time value.
#pragma once
#include "batch_mul_recode.hpp"

namespace msm377 {

constexpr int BMV_WIDTH = 4;                       // c: 4 doublings and one addition per step
constexpr int BMV_WINDOWS = bm_windows(BMV_WIDTH);  // 64
constexpr int BMV_ENTRIES = 1 << (BMV_WIDTH - 1);   // table entries per point: [1..8]P
constexpr int BMV_BIAS = BMV_ENTRIES - 1;           // nibble = digit + 7
static_assert(BMV_WINDOWS * BMV_WIDTH == BM_SCALAR_BITS && BMV_WINDOWS == 64, "eight nibbles per word, eight words");

// s[0..7] (little-endian words of the scalar) -> the packed digits in place; returns the final carry.
MSM_HD uint32_t bmv_pack(uint32_t* s) {
  uint32_t carry = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint32_t word = s[k];
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t one[1] = {word >> (4 * j)};
      const int32_t d = bm_digit(one, BMV_WIDTH, 0, carry);
      packed |= (uint32_t)(d + BMV_BIAS) << (4 * j);
    }
    s[k] = packed;
  }
  return carry;
}

// The digit of the top window still in the array, then the array moves up one window (zeros come in at the bottom;
// they are never read: 64 calls empty it).
MSM_HD int32_t bmv_next(uint32_t* s) {
  const int32_t d = (int32_t)(s[7] >> 28) - BMV_BIAS;
#pragma unroll
  for (int k = 7; k > 0; k--) s[k] = (s[k] << 4) | (s[k - 1] >> 28);
  s[0] <<= 4;
  return d;
}

}  // namespace msm377
