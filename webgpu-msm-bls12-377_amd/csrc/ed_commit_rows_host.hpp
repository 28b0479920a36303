// Host implementation of the Edwards-BLS12 row commitments (msm377_ed_commit_rows_host): out[i] = sum_{j<k} [s_ij]G_j on
// one thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of the device call
// (kernels/ed_commit_rows.hpp): every term by plain double-and-add over the bits of its scalar on the canonical formulas
// (ed_batch_mul_host.hpp ed_mul_bits_host), the terms added in the order of the generators by the general addition, one
// inversion per output -- no window table, no signed recode, no segments, no partial sums, no lazy forms, 64-bit words
// instead of 29-bit limbs.  Shared with the device call: the text of a refusal and nothing else (the device call checks
// its generators with k_check_curve<EdCheck>).  No device code, no context; compiles with plain g++.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "ed_batch_mul_host.hpp"
#include "ed_batch_mul_var_host.hpp"
#include "fp64_host.hpp"
#include "validate_host.hpp"

namespace msm377 {

// k in 1 .. MSM377_GEN_MAX; both strides non-zero multiples of 32.
inline bool ed_commit_rows_shape_ok(uint32_t k, uint64_t out_stride, uint64_t base_stride) {
  return k >= 1 && k <= MSM377_GEN_MAX && out_stride != 0 && base_stride != 0 && out_stride % 32 == 0 && base_stride % 32 == 0;
}

// The text msm377_last_error carries behind MSM377_EPOINT of msm377_ed_set_generators.
inline std::string ed_commit_rows_refusal(uint64_t index, uint32_t reason) {
  return "point " + std::to_string(index) + " of the generators" + (reason == MSM377_CHECK_CANONICAL ? " has a coordinate that is not below q" : " is not on the curve") +
         ": a set takes curve points only";
}

// gens_xy: k x 64 bytes x || y; s_ij: the 32 bytes at scalars + i * out_stride + j * base_stride, read as an integer and
// not reduced.  Outputs: 64-byte wire records, the identity as (0, 1).  MSM377_EINVAL and MSM377_EPOINT (a generator with
// a coordinate of q or more, or off the curve: ed_batch_mul_var_first_bad names the lowest) leave the outputs untouched.
inline int ed_commit_rows_host(const uint8_t* gens_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  if (!ed_commit_rows_shape_ok(k, out_stride, base_stride)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!gens_xy || !scalars || !out_points) return MSM377_EINVAL;
  uint32_t reason = 0;
  if (ed_batch_mul_var_first_bad(gens_xy, k, &reason) != UINT64_MAX) return MSM377_EPOINT;
  std::vector<EdH::Base> gen(k);
  for (uint32_t j = 0; j < k; j++) {
    EdHostCheck::Pt p;
    EdHostCheck::load(gens_xy + (size_t)j * 64, p);
    gen[j] = EdH::make_base(p.x, p.y);
  }
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* row = scalars + i * out_stride;
    EdH::Ext acc = ed_mul_bits_host(gen[0], row);
    for (uint32_t j = 1; j < k; j++) acc = EdH::add(acc, ed_mul_bits_host(gen[j], row + (uint64_t)j * base_stride));
    edh_to_wire(acc, out_points + i * 64);
  }
  return MSM377_OK;
}

}  // namespace msm377
