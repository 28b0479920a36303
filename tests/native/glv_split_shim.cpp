// csrc/glv_split.hpp -- the arithmetic of k_decompose_glv: Barrett quotient, its correction, the digit chains of both halves --
// compiled for the host with g++, behind one C function for tests/test_stage_model_host.py.  TEST INFRASTRUCTURE.
#include "glv_split.hpp"

extern "C" {

// Per scalar i < n (8 little-endian words at scalars + 8 i), in the order k_decompose_glv runs it:
//   rem0[5 i ..]     the remainder BEFORE the correction,      corrected[i]  whether the correction was taken,
//   k1[5 i ..], k2[5 i ..]  the halves after it,               digits[16 i ..]  the stored digits of k1, then of k2,
//   bad[i]           what the kernel ORs into its error word as bit 1.
void glv_split_table(const uint32_t* scalars, uint64_t n, uint32_t* rem0, uint32_t* k1, uint32_t* k2, uint16_t* digits, uint8_t* bad, uint8_t* corrected) {
  for (uint64_t i = 0; i < n; i++) {
    uint32_t q[5], rem[5];
    msm377::glv_quotient(scalars + 8 * i, q, rem);
    for (int j = 0; j < 5; j++) rem0[5 * i + j] = rem[j];
    corrected[i] = msm377::glv_correct(q, rem) ? 1 : 0;
    uint32_t b = msm377::glv_fifth_words(q, rem);
    for (int half = 0; half < 2; half++) {
      const uint32_t* v = half ? q : rem;
      uint32_t carry = 0, hb = 0;
      for (uint32_t win = 0; win < 8; win++) digits[16 * i + 8 * half + win] = (uint16_t)msm377::recode128_step(v, win, carry, hb);
      b |= hb;
    }
    for (int j = 0; j < 5; j++) k1[5 * i + j] = rem[j], k2[5 * i + j] = q[j];
    bad[i] = b ? 1 : 0;
  }
}

}
