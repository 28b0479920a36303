// Host implementation of the Edwards-BLS12 variable-base batch multiplication (msm377_ed_batch_mul_var_host):
// out[i] = [s_i]P_i on one thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of the device
// call (kernels/ed_batch_mul_var.hpp): plain double-and-add over the bits of every scalar on the canonical formulas, one
// inversion per output -- no table, no signed recode, no lazy forms, 64-bit words instead of 29-bit limbs.  Shared with
// the device call: the text of a refusal and nothing else (the device call checks its points with k_check_curve<EdCheck>).
// No device code, no context; compiles with plain g++.
#pragma once
#include <string.h>

#include <string>

#include "common.hpp"
#include "ed_batch_mul_host.hpp"
#include "fp64_host.hpp"
#include "validate_host.hpp"

namespace msm377 {

inline bool ed_batch_mul_var_stride_ok(uint32_t scalar_stride) { return scalar_stride == 0 || scalar_stride == 32; }

// The lowest index whose point has a coordinate that is not below q (reason MSM377_CHECK_CANONICAL) or is not on the
// curve (MSM377_CHECK_CURVE); UINT64_MAX if every point is a curve point.  The addition law is complete on the curve and
// nowhere else.
inline uint64_t ed_batch_mul_var_first_bad(const uint8_t* points, uint64_t n, uint32_t* reason) {
  for (uint64_t i = 0; i < n; i++) {
    EdHostCheck::Pt p;
    const bool canonical = EdHostCheck::load(points + i * 64, p);
    if (canonical && EdHostCheck::on_curve(p)) continue;
    *reason = canonical ? MSM377_CHECK_CURVE : MSM377_CHECK_CANONICAL;
    return i;
  }
  return UINT64_MAX;
}

// The text msm377_last_error carries behind MSM377_EPOINT, from the device's finding or the host's.
inline std::string ed_batch_mul_var_refusal(uint64_t index, uint32_t reason) {
  return "point " + std::to_string(index) + (reason == MSM377_CHECK_CANONICAL ? " has a coordinate that is not below q" : " is not on the curve") +
         ": the multiplication takes curve points only";
}

// points: n x 64 bytes x || y; s_i: the 32 bytes at scalars + i * scalar_stride (scalar_stride 0: one scalar for all), read
// as an integer and not reduced.  Outputs: 64-byte wire records, the identity as (0, 1); out_points may be points.
// MSM377_EINVAL and MSM377_EPOINT leave the outputs untouched.
inline int ed_batch_mul_var_host(const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points) {
  if (!ed_batch_mul_var_stride_ok(scalar_stride)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!points || !scalars || !out_points) return MSM377_EINVAL;
  uint32_t reason = 0;
  if (ed_batch_mul_var_first_bad(points, n, &reason) != UINT64_MAX) return MSM377_EPOINT;
  for (uint64_t i = 0; i < n; i++) {
    EdHostCheck::Pt p;
    EdHostCheck::load(points + i * 64, p);
    edh_to_wire(ed_mul_bits_host(EdH::make_base(p.x, p.y), scalars + i * (size_t)scalar_stride), out_points + i * 64);
  }
  return MSM377_OK;
}

}  // namespace msm377
