// Front-end import pass (msm377_ctx_set_input_format): the callers' native forms -> the wire format every kernel behind
// it reads.  Nothing in the reference corresponds to this: its harness hands over canonical residues.
//   k_import_points<FORM>           a thread per point: Montgomery coordinates v = x 2^384 (six u64 limbs, as arkworks and
//                                   snarkVM keep them) -> the canonical 96-byte record; with MSM377_POINTS_MONT_FLAG the
//                                   104-byte records carry an infinity flag, and the pass writes the INFINITY MASK (bit
//                                   i mod 32 of word i / 32) and counts the flagged points
//   k_import_scalars<FORM, MASKED>  a thread per scalar: Montgomery scalars v = s 2^256 -> canonical s < r; MASKED writes
//                                   zero for the scalars of flagged points
// A flagged point becomes the generator with a zero scalar: digit 0 is skipped by every path behind the sort, and the
// generator is a subgroup point, so the batched inversion, the Edwards map and the table doublings see nothing special.
// One field product per coordinate: mul(v, 2^22) = v 2^22 / 2^406 = v / 2^384 in the 13-limb field (field29.hpp, R = 2^406;
// the operand is canonical, the result reduced once), and mul(v, 2^5) = v / 2^256 in the 9-limb scalar field (R = 2^261):
// v < 2^256 makes the product v 2^5 < R, so the reduction leaves at most r and one conditional subtraction finishes.
// A coordinate of p or more is no Montgomery residue; its point is handed on UNCHANGED, so that the check calls count
// it as non-canonical by the value the caller wrote, and an MSM treats it like such a value in the wire format.
// The pass is memory-bound (200 / 208 bytes per point, 64 per scalar); canonical field forms throughout.
// Device code; included by sequencer.hip only (after kernels/validate.hpp: G1Check::canonical).
#pragma once
#include "../curves.hpp"

namespace msm377 {
namespace {

constexpr uint32_t IMPORT_THREADS = 256;

// FORM: MSM377_POINTS_MONT (96-byte records, 16-byte loads) or MSM377_POINTS_MONT_FLAG (104-byte records: a record is
// only 8-byte aligned, so it is read with 8-byte loads; a wave's 64 records are 6 656 contiguous bytes either way).
// inf_mask: ceil(n / 32) words, every one of them written; inf_count: incremented by the number of flagged points.
template <uint32_t FORM>
__global__ void __launch_bounds__(IMPORT_THREADS) k_import_points(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
                                                                  uint32_t* __restrict__ inf_mask, uint32_t* __restrict__ inf_count) {
  const uint64_t i = (uint64_t)blockIdx.x * IMPORT_THREADS + threadIdx.x;
  const bool live = i < n;
  bool flagged = false;
  if (live) {
    uint32_t w[24];
    if constexpr (FORM == MSM377_POINTS_MONT_FLAG) {
      const uint2* s = reinterpret_cast<const uint2*>(in + i * 104);
      flagged = (s[12].x & 0xffu) != 0;
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const uint2 v = s[k];
        w[2 * k] = v.x;
        w[2 * k + 1] = v.y;
      }
    } else {
      load_words16(reinterpret_cast<const uint32_t*>(in + i * 96), w, 6);
    }
    if (flagged) {
#pragma unroll
      for (int k = 0; k < 24; k++) w[k] = G1Consts::GEN_WIRE[k];
    } else if (G1Check::canonical(w)) {
      const Fp::El c = Fp::from_const(G1Consts::IMPORT_MONT384);
      const Fp::El x = Fp::mul(Fp::from_words<12>(w), c), y = Fp::mul(Fp::from_words<12>(w + 12), c);
      Fp::to_words<12>(x, w);
      Fp::to_words<12>(y, w + 12);
    }
    uint4* dst = reinterpret_cast<uint4*>(out + i * 24);
#pragma unroll
    for (int k = 0; k < 6; k++) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  }
  if constexpr (FORM == MSM377_POINTS_MONT_FLAG) {
    // a wave's 64 points are two mask words; whole waves reach this line (no early return above)
    const unsigned long long b = __ballot(flagged);
    if ((threadIdx.x & 63) == 0) {
      const uint64_t first = i >> 5, words = (n + 31) >> 5;
      if (first < words) inf_mask[first] = (uint32_t)b;
      if (first + 1 < words) inf_mask[first + 1] = (uint32_t)(b >> 32);
      if (b) atomicAdd(inf_count, (uint32_t)__popcll(b));
    }
  }
}

// FORM: MSM377_SCALARS_MONT (32-byte scalars) or MSM377_SCALARS_WIRE (a masked copy of scalars of `words` u32 each:
// 8, or 1 / 2 / 4 for the compact scalars of the short-scalar calls).  MASKED: bit i of inf_mask set -> scalar i = 0.
template <uint32_t FORM, bool MASKED>
__global__ void __launch_bounds__(IMPORT_THREADS) k_import_scalars(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n, uint32_t words,
                                                                   const uint32_t* __restrict__ inf_mask) {
  const uint64_t i = (uint64_t)blockIdx.x * IMPORT_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool zero = MASKED && ((inf_mask[i >> 5] >> (i & 31)) & 1u);
  if constexpr (FORM == MSM377_SCALARS_MONT) {
    uint32_t w[8];
    load_words16(in + i * 8, w, 2);
    const Fq::El s = Fq::mul(Fq::from_words<8>(w), Fq::from_const(EdConsts::IMPORT_MONT256));
    Fq::to_words<8>(s, w);
    uint4* dst = reinterpret_cast<uint4*>(out + i * 8);
    dst[0] = zero ? make_uint4(0, 0, 0, 0) : make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = zero ? make_uint4(0, 0, 0, 0) : make_uint4(w[4], w[5], w[6], w[7]);
  } else {
    for (uint32_t k = 0; k < words; k++) out[i * words + k] = zero ? 0u : in[i * words + k];
  }
}

}  // namespace
}  // namespace msm377
