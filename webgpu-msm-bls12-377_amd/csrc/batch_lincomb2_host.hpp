// Host implementation of the pairwise linear combination (msm377_g1_batch_lincomb2_host): out[i] = [a_i]P_i + [b_i]Q_i on
// one thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of the device call
// (kernels/batch_lincomb2.hpp): each term by plain bit-by-bit double-and-add from the top bit, then ONE general XYZZ
// addition -- no joint walk, no window, no recode, no table, 64-bit words instead of 29-bit limbs.  Shared with the other
// host twins: the output-writing tail (batch_mul_write_outputs_host).  Shared with the device: nothing.  No device code,
// no context; compiles with plain g++.
#pragma once
#include <string.h>

#include <vector>

#include "batch_mul_host.hpp"
#include "common.hpp"
#include "fp64_host.hpp"
#include "import_host.hpp"

namespace msm377 {

// [s]P for one record of point_form and one scalar of scalar_form; a flagged record's coordinate bytes are never interpreted.
inline G1H::XYZZ batch_lincomb2_term_host(const uint8_t* point, uint32_t point_form, const uint8_t* scalar, uint32_t scalar_form) {
  uint8_t wire[96], s[32];
  uint32_t mask = 0;
  import_points_host(point, 1, point_form, wire, &mask);
  import_scalars_host(scalar, 1, scalar_form, s);
  G1H::XYZZ t = G1H::identity();
  if (mask) return t;
  G1H::Affine p;
  memcpy(p.x.v, wire, 48);  // little-endian host
  memcpy(p.y.v, wire + 48, 48);
  p.x = Fp64::mul(p.x, Fp64::from_const(G1Consts64::R2));
  p.y = Fp64::mul(p.y, Fp64::from_const(G1Consts64::R2));
  const G1H::XYZZ q = G1H::from_affine(p);
  for (int bit = 255; bit >= 0; bit--) {
    t = G1H::dbl(t);
    if ((s[bit >> 3] >> (bit & 7)) & 1) t = G1H::add(t, q);  // identity, equal and opposite operands handled inside
  }
  return t;
}

// point_form (both arrays), scalar_form (both scalars), out_form, out_inf: as batch_mul_var_host.  a_stride, b_stride:
// each 32, or 0 (the one scalar at `a` / `b` for all n).  MSM377_EINVAL leaves the outputs untouched.
inline int batch_lincomb2_host(const uint8_t* p, const uint8_t* q, uint32_t point_form, const uint8_t* a, const uint8_t* b, uint32_t scalar_form, uint64_t n, uint32_t a_stride,
                               uint32_t b_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  if (out_form != MSM377_POINTS_WIRE && out_form != MSM377_POINTS_MONT_FLAG) return MSM377_EINVAL;
  if (point_form > MSM377_POINTS_MONT_FLAG || scalar_form > MSM377_SCALARS_MONT) return MSM377_EINVAL;
  if ((a_stride != 0 && a_stride != 32) || (b_stride != 0 && b_stride != 32)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!p || !q || !a || !b || !out_points) return MSM377_EINVAL;
  const size_t in_stride = point_form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  std::vector<G1H::XYZZ> acc(n);
  for (uint64_t i = 0; i < n; i++) {
    const G1H::XYZZ ta = batch_lincomb2_term_host(p + i * in_stride, point_form, a + i * (size_t)a_stride, scalar_form);
    const G1H::XYZZ tb = batch_lincomb2_term_host(q + i * in_stride, point_form, b + i * (size_t)b_stride, scalar_form);
    acc[i] = G1H::add(ta, tb);  // [a]P = +-[b]Q, either one O: handled inside
  }
  batch_mul_write_outputs_host(acc, out_form, out_points, out_inf);
  return MSM377_OK;
}

}  // namespace msm377
