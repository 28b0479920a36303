// Host implementation of fixed-base batch multiplication (msm377_g1_batch_mul_host): out[i] = [s_i]B on one thread with
// the host tail's field and point code (fp64_host.hpp).  The second, independent implementation the device call
// (kernels/batch_mul.hpp) is compared with: 64-bit words instead of 29-bit limbs, general XYZZ additions over a table that
// is never normalised, one fixed small width, the batched inversion on the calling thread.  Shared with the device: the
// recode (batch_mul_recode.hpp) and nothing else.  No device code, no context; compiles with plain g++.
#pragma once
#include <string.h>

#include <vector>

#include "batch_mul_recode.hpp"
#include "common.hpp"
#include "fp64_host.hpp"
#include "import_host.hpp"

namespace msm377 {

constexpr int BM_HOST_WIDTH = 4;  // 64 windows of 8 entries + the carry's entry: a table of 513 points per call

// The output-writing tail of both host twins (this one and batch_mul_var_host.hpp): Montgomery's trick over the XYZZ
// results on the calling thread, then the records of out_form (MSM377_POINTS_WIRE or MSM377_POINTS_MONT_FLAG) and the
// optional flag bytes.  An identity contributes 1 to the products.
inline void batch_mul_write_outputs_host(const std::vector<G1H::XYZZ>& acc, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  const uint64_t n = acc.size();
  std::vector<Fp64::El> prefix(n);
  Fp64::El run = Fp64::one();
  for (uint64_t i = 0; i < n; i++) {
    prefix[i] = run;
    if (!G1H::is_identity(acc[i])) run = Fp64::mul(run, acc[i].zzz);
  }
  Fp64::El inv = Fp64::inv(run);
  for (uint64_t i = n; i-- > 0;) {
    const G1H::XYZZ& a = acc[i];
    const bool ident = G1H::is_identity(a);
    Fp64::El x = Fp64::zero(), y = Fp64::one();
    if (!ident) {
      const Fp64::El zi = Fp64::mul(inv, prefix[i]);  // 1 / ZZZ_i
      inv = Fp64::mul(inv, a.zzz);
      const Fp64::El t = Fp64::mul(zi, a.zz);
      x = Fp64::mul(a.x, Fp64::sqr(t));
      y = Fp64::mul(a.y, zi);
    }
    if (out_form == MSM377_POINTS_WIRE) {
      Fp64::to_wire(x, out_points + i * 96);
      Fp64::to_wire(y, out_points + i * 96 + 48);
    } else {  // the host's Montgomery radix 2^384 IS the callers'
      uint8_t* rec = out_points + i * 104;
      memcpy(rec, x.v, 48);
      memcpy(rec + 48, y.v, 48);
      memset(rec + 96, 0, 8);
      rec[96] = ident ? 1 : 0;
    }
    if (out_inf) out_inf[i] = ident ? 1 : 0;
  }
}

// The terms of one base: acc[i] = [s_i]B as XYZZ points, s_i the 32 bytes at scalars + i * stride.  base_xy: 96 canonical
// wire bytes (the callers check).  batch_mul_host below and batch_mul_multi_host.hpp (one call per base) run this.
inline std::vector<G1H::XYZZ> batch_mul_terms_host(const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint64_t stride, uint32_t scalar_form) {
  G1H::Affine b;
  memcpy(b.x.v, base_xy, 48);  // little-endian host
  memcpy(b.y.v, base_xy + 48, 48);
  b.x = Fp64::mul(b.x, Fp64::from_const(G1Consts64::R2));
  b.y = Fp64::mul(b.y, Fp64::from_const(G1Consts64::R2));

  constexpr int C = BM_HOST_WIDTH, W = bm_windows(C), H = 1 << (C - 1);
  std::vector<G1H::XYZZ> table((size_t)W * H + 1);
  G1H::XYZZ row = G1H::from_affine(b);
  for (int w = 0; w <= W; w++) {  // row w: [d 2^(C w)]B by additions along the row; row W: the carry's entry alone
    table[(size_t)w * H] = row;
    for (int d = 1; d < H && w < W; d++) table[(size_t)w * H + d] = G1H::add(table[(size_t)w * H + d - 1], row);
    for (int k = 0; k < C; k++) row = G1H::dbl(row);
  }

  std::vector<G1H::XYZZ> acc(n);
  for (uint64_t i = 0; i < n; i++) {
    uint8_t wire[32];
    import_scalars_host(scalars + i * stride, 1, scalar_form, wire);
    uint32_t s[8];
    memcpy(s, wire, 32);
    G1H::XYZZ a = G1H::identity();
    uint32_t carry = 0;
    for (int w = 0; w <= W; w++) {
      const int32_t d = w < W ? bm_digit(s, C, w, carry) : (int32_t)carry;
      if (d == 0) continue;
      const G1H::XYZZ& e = table[(size_t)w * H + (d < 0 ? -d : d) - 1];
      a = G1H::add(a, d < 0 ? G1H::neg(e) : e);  // identity, equal and opposite operands handled inside
    }
    acc[i] = a;
  }
  return acc;
}

// scalar_form: MSM377_SCALARS_WIRE (32-byte integers, any value below 2^256, NOT reduced mod r: B may lie outside the
// prime-order subgroup) or MSM377_SCALARS_MONT (v 2^-256 mod r, fully reduced, as the MSM calls read them).
// out_form: MSM377_POINTS_WIRE (96-byte records, the identity as x = 0, y = 1) or MSM377_POINTS_MONT_FLAG (104-byte
// records: what msm377_g1_result_to_native makes of the wire record, the flag set for a true identity only).
// out_inf (may be null): n bytes, 1 for the identity.  MSM377_EINVAL leaves the outputs untouched.
inline int batch_mul_host(const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t scalar_form, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  if (out_form != MSM377_POINTS_WIRE && out_form != MSM377_POINTS_MONT_FLAG) return MSM377_EINVAL;
  if (scalar_form > MSM377_SCALARS_MONT) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!base_xy || !scalars || !out_points) return MSM377_EINVAL;
  uint64_t lim[2][6];
  memcpy(lim, base_xy, 96);  // little-endian host
  if (Fp64::geq_p(lim[0]) || Fp64::geq_p(lim[1])) return MSM377_EINVAL;
  const std::vector<G1H::XYZZ> acc = batch_mul_terms_host(base_xy, scalars, n, 32, scalar_form);
  batch_mul_write_outputs_host(acc, out_form, out_points, out_inf);
  return MSM377_OK;
}

}  // namespace msm377
