// Fixed-base batch multiplication (msm377_g1_batch_mul*): the signed window recode of a 256-bit scalar, ONE definition
// shared by the hot kernel (kernels/batch_mul.hpp), the host twin (batch_mul_host.hpp) and the stand-alone test program
// (tests/native/batch_mul_host.cpp).  No device code, no other header of the engine.
//
// A scalar s in [0, 2^256) and a width c give W = ceil(256 / c) digits and a final carry with
//     s = sum_w digit_w 2^(c w) + carry 2^(c W),   |digit_w| <= 2^(c-1),   carry in {0, 1}:
// walking from the low end, v = (the c bits of window w) + carry-in lies in [0, 2^c]; v <= 2^(c-1) is the digit itself,
// anything above it is v - 2^c with a carry into the next window (v = 2^c: digit 0 and a carry).  +2^(c-1) is a digit,
// -2^(c-1) is not, so the table of a window holds d = 1 .. 2^(c-1) and the sign picks the negative.  The top window of
// a width that does not divide 256 holds fewer than c bits; the rule is the same.  The carry out of the top window is
// NOT an error here (the MSM paths refuse such scalars): the table has an entry [2^(c W)]B for it.
#pragma once
#include <stdint.h>

#ifndef MSM_HD  // as in field29.hpp, for translation units that include this header alone
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSM_HD __host__ __device__ __forceinline__
#else
#define MSM_HD inline __attribute__((always_inline))
#endif
#endif

namespace msm377 {

constexpr int BM_SCALAR_BITS = 256;
constexpr int BM_MIN_WIDTH = 2, BM_MAX_WIDTH = 16;  // what bm_digit accepts; the device call supports 8 and 16, the host twin runs 4
constexpr int bm_windows(int c) { return (BM_SCALAR_BITS + c - 1) / c; }

// Digit of window w of the scalar in s[0..7] (little-endian u32 words).  `carry` is the carry into the window on entry
// and the carry out of it on return: call with w = 0, 1, .., W - 1 in order, starting from carry = 0; what is left
// after w = W - 1 is the final carry.
MSM_HD int32_t bm_digit(const uint32_t* s, int c, int w, uint32_t& carry) {
  const int bit = c * w, wi = bit >> 5, off = bit & 31;
  uint32_t v = s[wi] >> off;
  if (off + c > 32 && wi + 1 < 8) v |= s[wi + 1] << (32 - off);
  v &= (1u << c) - 1u;  // (bits past 255 are zero already: the shifts bring in zeros)
  v += carry;
  const uint32_t half = 1u << (c - 1);
  carry = v > half ? 1u : 0u;
  return (int32_t)v - (int32_t)(carry << c);
}

// ---- widths of the device call (msm377_ctx_set_mul_window) and the rule by n ----
//   c = 8    32 + 1 additions per output, 4 096 + 1 table records (0.5 MB: L2-resident)
//   c = 16   16 + 1 additions per output, 2^19 + 1 records (64 MB: gathered at random from the Infinity Cache)
// Measured on one MI355X (profiles/batch_mul/sweep.txt): a warm call is faster on the wide table at every size (2^12: 0.57
// against 0.71 ms, 2^20: 2.76 against 4.62 ms), but its build costs 9.25 ms against 7.00 (6.0 ms of either: the
// 256-doubling chain of the row bases), and it holds 64 MB.  A call of 2^20 outputs saves 1.86 ms of the 2.25 ms of extra
// build: one cold call breaks even at 1.27 million outputs, two calls on one base at 2^19.3, three below 2^19.  A table is
// there to be reused: the rule takes the wide table from 2^19 outputs on, between the second and the third call;
// a caller that reuses a base for many smaller batches forces it with msm377_ctx_set_mul_window(ctx, 16).
constexpr int BM_NARROW_WIDTH = 8, BM_WIDE_WIDTH = 16;
constexpr uint64_t BM_WIDE_MIN_OUTPUTS = 1ull << 19;
inline bool batch_mul_width_supported(int c) { return c == BM_NARROW_WIDTH || c == BM_WIDE_WIDTH; }
inline int batch_mul_rule(uint64_t n) { return n >= BM_WIDE_MIN_OUTPUTS ? BM_WIDE_WIDTH : BM_NARROW_WIDTH; }

// The multi-base call (msm377_g1_batch_mul_multi*, k tables walked into one accumulator): per base the trade is the one
// above -- the row-base chain is paid once per build whatever k, the entries and their normalisation once per table, the
// saving of the wide table once per walk.  Measured for k = 2, 4, 8 (profiles/batch_mul_multi/sweep.txt): a warm call of
// 2^20 outputs saves 1.75 to 1.86 ms PER TABLE on the wide tables (2^19: 0.90 to 0.99 ms) and a build costs 2.4 to 2.6 ms
// more PER TABLE (k = 2: 12.5 against 7.3 ms, k = 8: 26.9 against 7.3).  Both sides scale with k, so the crossover in n is
// the single-base call's for every k -- one cold call breaks even at about 1.4 million outputs, two calls at 2^19.5, three
// at 2^19 -- and so is the rule.  k stays an argument: it is what a rule for tables far past the Infinity Cache would read
// (1.07 GB at k = 16 showed no slowdown).
inline int batch_mul_multi_rule(uint64_t n, uint32_t k) {
  (void)k;
  return batch_mul_rule(n);
}

}  // namespace msm377
