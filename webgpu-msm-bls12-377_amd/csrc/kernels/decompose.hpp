// Stage 1: scalars -> signed window digits (k_decompose, k_decompose_geom, k_decompose_glv; k_decompose_short and
// k_scalars_width for scalars of a declared width).  Replaces
// wgsl/cuzk/convert_point_coords_and_decompose_scalars.template.wgsl:100-141; model cuzk/utils.ts:66-109.
// Device code; included by sequencer.hip only.
#pragma once
#include "../curves.hpp"
#include "../glv_split.hpp"

namespace msm377 {
namespace {

__device__ __forceinline__ void digit_key(uint32_t biased, uint32_t& key, uint32_t& sign) {
  int d = (int)biased - 32768;
  sign = d < 0 ? 1u : 0u;
  key = (uint32_t)(d < 0 ? -d : d);
}
// The same for a slot whose key_max word may carry KEY_UNSIGNED (the top window of a short-scalar call, k_decompose_short).
__device__ __forceinline__ void digit_key(uint32_t stored, bool uns, uint32_t& key, uint32_t& sign) {
  digit_key(stored, key, sign);
  if (uns) key = stored, sign = 0u;
}
// A window whose digits stay small (the top window: a 253-bit scalar leaves it 13 bits) would crowd all its
// elements into a few of the 256 ranges -- regions far beyond what k_local_sort keeps in LDS.  The decomposition
// records the largest key of window 15 and the sort narrows that window's ranges by a power of two (shift s:
// 128 >> s keys per range, s <= 5) so that the keys in use still spread over the 256 regions; every other
// window slot keeps the full width (key_max = NB).
__device__ __forceinline__ uint32_t win_shift(uint32_t key_max_word) {
  if (!(key_max_word & KEY_TRACKED)) return 0;
  const uint32_t max_key = key_max_word & ~(KEY_TRACKED | KEY_UNSIGNED);
  uint32_t s = 0;
  while (s < 5 && max_key < (NB >> (s + 1))) s++;
  return s;
}
__device__ __forceinline__ uint32_t key_range(uint32_t key, uint32_t s) {
  return s == 0 ? (key >= NB ? NRANGE - 1 : key / KRANGE) : key >> (7 - s);
}

// One thread per scalar: 16 signed digits d_w in [-2^15, 2^15), stored biased (d + 2^15).
// Only windows [wb, wb + wc) are written (window sharding); the carry chain always runs over
// all 16.  A final carry (scalar >= 2^255 - 2^239) sets *err, as cuzk/utils.ts:95-98 throws.
//
// even != 0 (whole MSMs, sequencer.hip WindowPlan::recode): the three bits a 253-bit scalar leaves unused are spread over the
// top THREE windows instead of emptying the last one -- windows 0..12 as above, windows 13, 14, 15 take 15 bits each
// (bit offsets 208, 223, 238: common.hpp even_offset) as UNSIGNED digits in [0, 2^15) with a carry chain of their own
// (limb + carry = 2^15 -> digit 0, carry 1).  Every window then fills its 2^15 buckets with rows of n / 2^15 entries;
// with sixteen 16-bit windows the top one holds 13 significant bits: n entries in 4096 rows, each cut into several
// work items whose partial sums a merge kernel adds back (31 us at 2^20), and a sort with narrowed ranges for that
// window (win_shift).  A scalar of 2^253 - 2^238 and more, whose top digit does not fit, raises ERR_NARROW_RANGE and
// the call reruns with the sixteen equal windows; the ERROR condition stays the one of the 16-bit recode.
__global__ void __launch_bounds__(256) k_decompose(const uint32_t* __restrict__ scalars, uint16_t* __restrict__ digits, uint64_t n,
                                                   uint32_t wb, uint32_t wc, int* __restrict__ err, uint32_t* __restrict__ top_key_max, uint32_t even) {
  // top_key_max (may be null): largest key of window 15, the one window that scalars below a 253-bit modulus leave
  // mostly empty; see win_shift.  One LDS atomic per thread at worst, one global atomic per block.
  __shared__ uint32_t wmax;
  if (threadIdx.x == 0) wmax = 0;
  __syncthreads();
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    uint32_t w[8];
    load_words16(scalars + i * 8, w, 2);
    uint32_t carry = 0;
    if (even) {
      uint32_t carry16 = 0;  // the 16-bit recode's carry chain: the error condition
#pragma unroll
      for (uint32_t win = 0; win < 16; win++) {
        const uint32_t limb = (w[win >> 1] >> (16 * (win & 1))) & 0xffffu;
        carry16 = limb + carry16 >= 32768u ? 1u : 0u;
        uint32_t biased;
        if (win < EVEN_FROM) {
          const uint32_t v = limb + carry;
          carry = v >= 32768u ? 1u : 0u;
          biased = (v + 32768u) & 0xffffu;
        } else {
          const uint32_t raw = win == 13 ? (w[6] >> 16) & 0x7fffu : win == 14 ? (w[6] >> 31) | ((w[7] & 0x3fffu) << 1) : (w[7] >> 14) & 0x7fffu;
          const uint32_t v = raw + carry;
          carry = v >> 15;
          biased = (v & 0x7fffu) + 32768u;
        }
        if (win >= wb && win < wb + wc) digits[(size_t)(win - wb) * n + i] = (uint16_t)biased;
      }
      if (carry | (w[7] >> 29)) atomicOr(err, ERR_NARROW_RANGE);
      if (carry16) atomicOr(err, ERR_SCALAR);
    } else {
#pragma unroll
      for (uint32_t win = 0; win < 16; win++) {
        uint32_t limb = (w[win >> 1] >> (16 * (win & 1))) & 0xffffu;
        uint32_t v = limb + carry;
        carry = v >= 32768u ? 1u : 0u;
        if (win >= wb && win < wb + wc) {
          const uint32_t biased = (v + 32768u) & 0xffffu;
          digits[(size_t)(win - wb) * n + i] = (uint16_t)biased;
          if (win == 15 && top_key_max) {
            uint32_t key, sign;
            digit_key(biased, key, sign);
            if ((key | KEY_TRACKED) > wmax) atomicMax(&wmax, key | KEY_TRACKED);
          }
        }
      }
      if (carry) atomicOr(err, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && top_key_max && wmax > *top_key_max) atomicMax(top_key_max, wmax);
}

// ---- narrow windows for small inputs (the reference switches to 4-bit windows below
//      65 536 points, src/submission/submission.ts:97,173-186) ----
// Below ~2^15 points the 16 x 32 768 buckets of the main path are mostly empty and their reduction -- 15 levels, the
// first ones streaming 134 MB of identity records -- is most of the call.  With windows of 2 048 buckets the bucket
// array shrinks 11-fold and the reduction loses four levels; the additions grow from 16 n to 22 n, which a small input
// does not notice.  Everything behind the sort runs the same kernels with L = 11 as their run-time bucket geometry;
// decomposition and sort have their own small kernels (k_decompose_geom, k_small_sort).
// The error condition is the one of the 16-bit recode for every input size (cuzk/utils.ts:95-98 throws when the recode
// ends with a carry; with 16-bit windows that is k >= 2^255 - 2^239), whichever window width runs here.  The reference
// itself switches to 4-bit windows below 65 536 points (submission.ts:97), where the same check fires for every
// k > 0x7777...7 -- a set that differs only in NON-canonical scalars (every k < r passes both): deliberately not
// reproduced, one error condition for all sizes (tests/test_g1_parity_gpu.py::test_narrow_windows_edge_cases).

// The even geometry in general (k_decompose's `even` mode is the instance L = 15, a = 13, W = 16 with its fields at fixed
// places): W windows of 2^L buckets over the 253 bits of a scalar below r -- the first `a` windows are SIGNED digits of
// L + 1 bits (|d| <= 2^L, carry into the next window), the other W - a are UNSIGNED digits of L bits with a carry chain
// of their own (limb + carry = 2^L -> digit 0, carry 1), and a (L + 1) + (W - a) L = 253, so that every window fills
// its 2^L buckets with rows of n / 2^L entries.  The small-input path runs it with L = 11, a = 11, W = 22 (common.hpp
// NARROW_EVEN_*).  (Its first geometry, 22 signed 11-bit windows + an unsigned top one, reached only half of a window's
// 2048 buckets with its signed digits; retired in favour of this one, HISTORY.md.)  Digits are stored biased by `bias`
// (2^L for k_small_sort).  A scalar whose top digit does not fit -- everything from 2^253 on and the few below that
// carry out of the top window -- raises ERR_NARROW_RANGE and the call reruns with sixteen 16-bit windows; the ERROR
// condition stays the 16-bit recode's.
__global__ void __launch_bounds__(256) k_decompose_geom(const uint32_t* __restrict__ scalars, uint16_t* __restrict__ digits, uint64_t n, uint32_t L,
                                                        uint32_t a, uint32_t W, uint32_t bias, int* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  load_words16(scalars + i * 8, w, 2);
  uint32_t carry = 0, bit = 0;
  for (uint32_t win = 0; win < W; win++) {
    const uint32_t c = win < a ? L + 1 : L, word = bit >> 5, off = bit & 31;
    uint32_t v = w[word] >> off;
    if (off + c > 32 && word + 1 < 8) v |= w[word + 1] << (32 - off);
    v = (v & ((1u << c) - 1u)) + carry;
    uint32_t stored;
    if (win < a) {
      carry = v >> L ? 1u : 0u;  // v >= 2^L: the digit is v - 2^(L+1), in [-2^L, 0]
      stored = v + bias - (carry << c);
    } else {
      carry = v >> L;  // v = 2^L: digit 0, carry on
      stored = (v & ((1u << L) - 1u)) + bias;
    }
    digits[(size_t)win * n + i] = (uint16_t)stored;
    bit += c;
  }
  if (carry | (w[7] >> 29)) atomicOr(err, ERR_NARROW_RANGE);  // bit == 253 here
  uint32_t carry16 = 0;
#pragma unroll
  for (uint32_t win = 0; win < 16; win++) carry16 = (((w[win >> 1] >> (16 * (win & 1))) & 0xffffu) + carry16) >= 32768u ? 1u : 0u;
  if (carry16) atomicOr(err, ERR_SCALAR);
}

// ---- short scalars (include/msm377.h msm377_g1_msm_short*) ----
// The caller declares that every scalar is below 2^bits and hands them over as n x SB little-endian bytes, SB = 4, 8, 16
// or 32.  The call then runs W = floor(bits / (L + 1)) + 1 window slots (common.hpp short_windows) instead of the 16 or
// 22 of a 253-bit scalar: the first W - 1 are SIGNED digits of L + 1 bits (v = field + carry; v >= 2^L: digit
// v - 2^(L+1) in [-2^L, 0] and a carry into the next window), the top one is the UNSIGNED rest, bits mod (L + 1) <= L
// bits plus the carry: at most 2^L, so nothing carries out and no scalar below 2^bits needs a second pass.
// A scalar of 2^bits or more raises ERR_SHORT_WIDTH (the call fails with MSM377_ESCALAR); its excess bits are dropped
// before the recode, so that every digit stays a valid sort key whatever the input holds.
//
// One thread per scalar.  Every lane issues 16-byte loads: with SB = 4 (8) four (two) neighbouring lanes read the same
// aligned 16 bytes and pick their word(s) -- the wave still covers one contiguous stretch -- except at the end of an
// array whose last 16 bytes are incomplete, where the lane loads its SB bytes alone.
template <int SB>
__device__ __forceinline__ void load_short_scalar(const uint8_t* __restrict__ scalars, uint64_t i, uint64_t n, uint32_t* w /* SB / 4 words */) {
  if constexpr (SB >= 16) {
    load_words16(reinterpret_cast<const uint32_t*>(scalars + i * SB), w, SB / 16);
  } else {
    constexpr uint64_t PER = 16 / SB;  // scalars per 16 bytes
    const uint64_t g = i / PER;
    if ((g + 1) * PER <= n) {
      uint4 q = reinterpret_cast<const uint4*>(scalars)[g];
      asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));  // all four words: keeps the load 16 bytes wide (else it is narrowed to the word picked below)
      const uint32_t k = (uint32_t)(i % PER);
      if constexpr (SB == 8) {
        w[0] = k ? q.z : q.x;
        w[1] = k ? q.w : q.y;
      } else {
        w[0] = k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w;
      }
    } else if constexpr (SB == 8) {
      const uint2 q = reinterpret_cast<const uint2*>(scalars)[i];
      w[0] = q.x;
      w[1] = q.y;
    } else {
      w[0] = reinterpret_cast<const uint32_t*>(scalars)[i];
    }
  }
}

// Digits are stored biased by `bias` (2^15 on the main path, 2^L for k_small_sort); the top window's by `top_bias`: the
// same on the narrow path, 0 on the main path, whose sort then reads that slot as unsigned (KEY_UNSIGNED in its key_max
// word: +2^15 does not fit a 16-bit digit biased by 2^15).  top_key_max (main path; null otherwise): the largest key of
// the top window, which holds few bits or carries only -- the sort narrows its ranges by it (win_shift).
template <int SB>
__global__ void __launch_bounds__(256) k_decompose_short(const uint8_t* __restrict__ scalars, uint16_t* __restrict__ digits, uint64_t n, uint32_t bits, uint32_t L,
                                                         uint32_t W, uint32_t bias, uint32_t top_bias, int* __restrict__ err, uint32_t* __restrict__ top_key_max) {
  constexpr int NW = SB / 4;
  __shared__ uint32_t wmax;
  if (threadIdx.x == 0) wmax = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    uint32_t w[NW];
    load_short_scalar<SB>(scalars, i, n, w);
    uint32_t excess = 0;  // bits at 2^bits and above
#pragma unroll
    for (int j = 0; j < NW; j++) {
      const uint32_t lo = 32u * j;
      const uint32_t keep = bits <= lo ? 0u : bits >= lo + 32u ? 0xffffffffu : (1u << (bits - lo)) - 1u;
      excess |= w[j] & ~keep;
      w[j] &= keep;
    }
    if (excess) atomicOr(err, ERR_SHORT_WIDTH);
    const uint32_t c = L + 1, mask = (1u << c) - 1u;  // c <= 16
    uint32_t carry = 0;
    for (uint32_t win = 0; win + 1 < W; win++) {
      const uint32_t v = (w[0] & mask) + carry;
      carry = v >> L ? 1u : 0u;
      digits[(size_t)win * n + i] = (uint16_t)(v + bias - (carry << c));
#pragma unroll
      for (int j = 0; j + 1 < NW; j++) w[j] = (w[j] >> c) | (w[j + 1] << (32u - c));  // the scalar moves down a window: no indexed register access
      w[NW - 1] >>= c;
    }
    const uint32_t top = w[0] + carry;  // what is left is below 2^(bits mod c) <= 2^L
    digits[(size_t)(W - 1) * n + i] = (uint16_t)(top + top_bias);
    if (top_key_max && top > wmax) atomicMax(&wmax, top);
  }
  __syncthreads();
  if (threadIdx.x == 0 && top_key_max) atomicMax(top_key_max, wmax | KEY_TRACKED | KEY_UNSIGNED);
}

// Largest bit length in an array of n scalars of `wps` 32-bit words each (1, 2, 4 or 8), 0 if all are zero: the array
// is read as 16-byte groups of words whatever the stride -- word k of the array is word k mod wps of its scalar -- a
// grid-stride loop, a maximum per wave by lane exchange, one per workgroup through LDS, one atomic per workgroup.
__global__ void __launch_bounds__(256) k_scalars_width(const uint32_t* __restrict__ words, uint64_t nwords, uint32_t wps, uint32_t* __restrict__ out) {
  __shared__ uint32_t wave_max[4];
  const uint32_t tid = threadIdx.x;
  const uint64_t groups = nwords / 4;
  const uint4* v = reinterpret_cast<const uint4*>(words);
  uint32_t m = 0;
  auto see = [&](uint64_t k, uint32_t x) {
    if (x) {
      const uint32_t len = ((uint32_t)k & (wps - 1u)) * 32u + 32u - (uint32_t)__builtin_clz(x);
      m = len > m ? len : m;
    }
  };
  for (uint64_t g = (uint64_t)blockIdx.x * 256 + tid; g < groups; g += (uint64_t)gridDim.x * 256) {
    const uint4 q = v[g];
    see(4 * g, q.x);
    see(4 * g + 1, q.y);
    see(4 * g + 2, q.z);
    see(4 * g + 3, q.w);
  }
  if (blockIdx.x == 0 && tid < (uint32_t)(nwords & 3)) see(4 * groups + tid, words[4 * groups + tid]);  // an incomplete last group
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, off, 64);
    m = o > m ? o : m;
  }
  if ((tid & 63) == 0) wave_max[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; k++) m = wave_max[k] > m ? wave_max[k] : m;
    if (m) atomicMax(out, m);
  }
}

// Eight signed 16-bit digits of a 128-bit value v < 2^127 (top digit stays non-negative; the chain is recode128_step of
// glv_split.hpp); windows [wb, wb + wc) are written to slots 0..wc-1.  Returns non-zero if the value does not fit (top
// window reaches 2^15).
__device__ __forceinline__ uint32_t recode128(const uint32_t* v, uint16_t* __restrict__ digits, size_t stride, size_t col, uint32_t wb,
                                              uint32_t wc) {
  uint32_t carry = 0, bad = 0;
#pragma unroll
  for (uint32_t win = 0; win < 8; win++) {
    const uint32_t stored = recode128_step(v, win, carry, bad);
    if (win >= wb && win < wb + wc) digits[(size_t)(win - wb) * stride + col] = (uint16_t)stored;
  }
  return bad;
}

// One thread per scalar: k -> (k1, k2) by a Barrett quotient (MU = floor(2^384 / LAMBDA), at
// most one correction: glv_split.hpp, shared with the host), then the signed digits of k1 into
// column i and of k2 into column n + i of the 8 x 2n digit matrix.  Scalars outside the GLV range
// (k2 >= 2^127, i.e. k >~ 2^254) set bit 1 of *err: the host then reruns the call on the plain
// 16-window path.
__global__ void __launch_bounds__(256) k_decompose_glv(const uint32_t* __restrict__ scalars, uint16_t* __restrict__ digits, uint64_t n,
                                                       uint32_t wb, uint32_t wc, int* __restrict__ err) {
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
  load_words16(scalars + i * 8, k, 2);
  uint32_t q[5], rem[5];
  glv_quotient(k, q, rem);
  glv_correct(q, rem);  // rem in [0, 2 LAMBDA): one conditional correction
  uint32_t bad = glv_fifth_words(q, rem);
  bad |= recode128(rem, digits, (size_t)2 * n, (size_t)i, wb, wc);
  bad |= recode128(q, digits, (size_t)2 * n, (size_t)(n + i), wb, wc);
  if (bad) atomicOr(err, 2);
}

}  // namespace
}  // namespace msm377
