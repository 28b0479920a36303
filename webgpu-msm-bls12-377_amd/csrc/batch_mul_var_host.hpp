// Host implementation of variable-base batch multiplication (msm377_g1_batch_mul_var_host): out[i] = [s_i]P_i on one
// thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of the device call
// (kernels/batch_mul_var.hpp): plain bit-by-bit double-and-add from the top bit with general XYZZ additions -- no window,
// no recode, no table, 64-bit words instead of 29-bit limbs.  Shared with the fixed-base twin: the output-writing tail
// (batch_mul_write_outputs_host).  Shared with the device: nothing.  No device code, no context; compiles with plain g++.
#pragma once
#include <string.h>

#include <vector>

#include "batch_mul_host.hpp"
#include "common.hpp"
#include "fp64_host.hpp"
#include "import_host.hpp"

namespace msm377 {

// point_form: MSM377_POINTS_WIRE, _MONT (96-byte records) or _MONT_FLAG (104-byte records; a flagged record is the
// identity and its coordinate bytes are never interpreted).  Coordinates of p or more are trusted not to occur.
// scalar_form, out_form, out_inf: as batch_mul_host.  scalar_stride: 32, or 0 (the one scalar at `scalars` for all n).
// MSM377_EINVAL leaves the outputs untouched.
inline int batch_mul_var_host(const uint8_t* points, uint32_t point_form, const uint8_t* scalars, uint32_t scalar_form, uint64_t n, uint32_t scalar_stride, uint32_t out_form,
                              uint8_t* out_points, uint8_t* out_inf) {
  if (out_form != MSM377_POINTS_WIRE && out_form != MSM377_POINTS_MONT_FLAG) return MSM377_EINVAL;
  if (point_form > MSM377_POINTS_MONT_FLAG || scalar_form > MSM377_SCALARS_MONT) return MSM377_EINVAL;
  if (scalar_stride != 0 && scalar_stride != 32) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!points || !scalars || !out_points) return MSM377_EINVAL;
  const size_t in_stride = point_form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  std::vector<G1H::XYZZ> acc(n);
  for (uint64_t i = 0; i < n; i++) {
    uint8_t wire[96], s[32];
    uint32_t mask = 0;
    import_points_host(points + i * in_stride, 1, point_form, wire, &mask);
    import_scalars_host(scalars + i * (size_t)scalar_stride, 1, scalar_form, s);
    G1H::XYZZ a = G1H::identity();
    if (!mask) {
      G1H::Affine p;
      memcpy(p.x.v, wire, 48);  // little-endian host
      memcpy(p.y.v, wire + 48, 48);
      p.x = Fp64::mul(p.x, Fp64::from_const(G1Consts64::R2));
      p.y = Fp64::mul(p.y, Fp64::from_const(G1Consts64::R2));
      const G1H::XYZZ q = G1H::from_affine(p);
      for (int bit = 255; bit >= 0; bit--) {
        a = G1H::dbl(a);
        if ((s[bit >> 3] >> (bit & 7)) & 1) a = G1H::add(a, q);  // identity, equal and opposite operands handled inside
      }
    }
    acc[i] = a;
  }
  batch_mul_write_outputs_host(acc, out_form, out_points, out_inf);
  return MSM377_OK;
}

}  // namespace msm377
