// Host implementation of the row commitments (msm377_g1_commit_rows_host): out[i] = sum_j [s_ij]G_j on one thread with
// the host tail's field and point code (fp64_host.hpp).  The yardstick of the device call (kernels/commit_rows.hpp): the
// terms of each generator by the single-base twin (batch_mul_terms_host: its own narrow table per generator, general XYZZ
// additions), then one general addition per generator and output, in the order of the generators -- no segments, no
// partial sums, 64-bit words instead of 29-bit limbs.  Shared with the device: the recode (batch_mul_recode.hpp), through
// the single-base twin, and nothing else; the canonical check of the generators is the multi-base twin's.  No device
// code, no context; compiles with plain g++.
#pragma once
#include <string.h>

#include <vector>

#include "batch_mul_host.hpp"
#include "batch_mul_multi_host.hpp"
#include "common.hpp"
#include "fp64_host.hpp"

namespace msm377 {

// k in 1 .. MSM377_GEN_MAX; both strides non-zero multiples of 32.
inline bool commit_rows_shape_ok(uint32_t k, uint64_t out_stride, uint64_t base_stride) {
  return k >= 1 && k <= MSM377_GEN_MAX && out_stride != 0 && base_stride != 0 && out_stride % 32 == 0 && base_stride % 32 == 0;
}

// s_ij: the 32 bytes at scalars + i * out_stride + j * base_stride.  scalar_form, out_form, out_inf: as batch_mul_host.
// MSM377_EINVAL leaves the outputs untouched.
inline int commit_rows_host(const uint8_t* gens_xy, uint32_t k, const uint8_t* scalars, uint32_t scalar_form, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                            uint8_t* out_points, uint8_t* out_inf) {
  if (out_form != MSM377_POINTS_WIRE && out_form != MSM377_POINTS_MONT_FLAG) return MSM377_EINVAL;
  if (scalar_form > MSM377_SCALARS_MONT) return MSM377_EINVAL;
  if (!commit_rows_shape_ok(k, out_stride, base_stride)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!gens_xy || !scalars || !out_points) return MSM377_EINVAL;
  if (!batch_mul_multi_bases_canonical(gens_xy, k)) return MSM377_EINVAL;
  std::vector<G1H::XYZZ> acc = batch_mul_terms_host(gens_xy, scalars, n, out_stride, scalar_form);
  for (uint32_t j = 1; j < k; j++) {
    const std::vector<G1H::XYZZ> term = batch_mul_terms_host(gens_xy + (size_t)j * 96, scalars + (size_t)j * base_stride, n, out_stride, scalar_form);
    for (uint64_t i = 0; i < n; i++) acc[i] = G1H::add(acc[i], term[i]);  // equal and opposite terms, either one O: handled inside
  }
  batch_mul_write_outputs_host(acc, out_form, out_points, out_inf);
  return MSM377_OK;
}

}  // namespace msm377
