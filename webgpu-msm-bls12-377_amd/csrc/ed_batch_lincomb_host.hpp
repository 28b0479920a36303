// Host implementation of the Edwards-BLS12 k-term linear combination (msm377_ed_batch_lincomb_host):
// out[i] = sum_{j<k} [s_ij]P_ij on one thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of
// the device call (kernels/ed_batch_lincomb.hpp): each term by plain double-and-add over the bits of its scalar on the
// canonical formulas, the terms added in order with the general addition, one inversion per output -- no table, no signed
// recode, no shared doublings, no lazy forms.  Shared with the device call: the shape rule, the order of a refusal and its
// text, and nothing else (the device call checks its points with k_check_curve<EdCheck>).  No device code, no context;
// compiles with plain g++.
#pragma once
#include <string.h>

#include <string>

#include "common.hpp"
#include "ed_batch_mul_host.hpp"
#include "ed_batch_mul_var_host.hpp"
#include "fp64_host.hpp"
#include "validate_host.hpp"

namespace msm377 {

// k terms, 1 <= k <= MSM377_LINCOMB_MAX_TERMS, in host memory; point_stride 64 or 0, scalar_stride 32 or 0 in every one.
inline bool ed_batch_lincomb_shape_ok(const msm377_lincomb_term* terms, uint32_t k) {
  if (!terms || k < 1 || k > MSM377_LINCOMB_MAX_TERMS) return false;
  for (uint32_t j = 0; j < k; j++)
    if ((terms[j].point_stride != 0 && terms[j].point_stride != 64) || !ed_batch_mul_var_stride_ok(terms[j].scalar_stride)) return false;
  return true;
}

// No pointer of a term is null, and the outputs do not lie over the ONE point of a stride-0 term.
inline bool ed_batch_lincomb_pointers_ok(const msm377_lincomb_term* terms, uint32_t k, const void* out_points) {
  if (!out_points) return false;
  for (uint32_t j = 0; j < k; j++)
    if (!terms[j].points || !terms[j].scalars || (terms[j].point_stride == 0 && terms[j].points == out_points)) return false;
  return true;
}

// Which of the terms' findings is reported: bad[j] is the lowest failing index of term j, UINT64_MAX for none.  The lowest
// index wins; among equal indices the lowest term.  Returns k if there is no finding.
inline uint32_t ed_batch_lincomb_first_term(const uint64_t* bad, uint32_t k) {
  uint32_t t = k;
  for (uint32_t j = 0; j < k; j++)
    if (bad[j] != UINT64_MAX && (t == k || bad[j] < bad[t])) t = j;
  return t;
}

// The finding of all k arrays (a stride-0 term is ONE point, index 0): false if every point is a curve point; else *term,
// *index in that term's array and *reason (MSM377_CHECK_CANONICAL / MSM377_CHECK_CURVE).
inline bool ed_batch_lincomb_first_bad(const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint32_t* term, uint64_t* index, uint32_t* reason) {
  uint64_t bad[MSM377_LINCOMB_MAX_TERMS];
  uint32_t why[MSM377_LINCOMB_MAX_TERMS] = {};
  for (uint32_t j = 0; j < k; j++) bad[j] = ed_batch_mul_var_first_bad((const uint8_t*)terms[j].points, terms[j].point_stride ? n : 1, &why[j]);
  const uint32_t t = ed_batch_lincomb_first_term(bad, k);
  if (t == k) return false;
  *term = t;
  *index = bad[t];
  *reason = why[t];
  return true;
}

// The text msm377_last_error carries behind MSM377_EPOINT, from the device's finding or the host's.
inline std::string ed_batch_lincomb_refusal(uint32_t term, uint64_t index, uint32_t reason) {
  return "point " + std::to_string(index) + " of term " + std::to_string(term) +
         (reason == MSM377_CHECK_CANONICAL ? " has a coordinate that is not below q" : " is not on the curve") + ": the linear combination takes curve points only";
}

// P_ij: the 64 bytes x || y at terms[j].points + i * point_stride; s_ij: the 32 bytes at terms[j].scalars + i *
// scalar_stride, read as an integer and not reduced.  Outputs: 64-byte wire records, the identity as (0, 1).  out_points
// may be the points of any term of stride 64, and the fold in place works: all terms of output i are read before output i
// is written, and no later output reads record i.  MSM377_EINVAL and MSM377_EPOINT leave the outputs untouched.
inline int ed_batch_lincomb_host(const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint8_t* out_points) {
  if (!ed_batch_lincomb_shape_ok(terms, k)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!ed_batch_lincomb_pointers_ok(terms, k, out_points)) return MSM377_EINVAL;
  uint32_t term = 0, reason = 0;
  uint64_t index = 0;
  if (ed_batch_lincomb_first_bad(terms, k, n, &term, &index, &reason)) return MSM377_EPOINT;
  for (uint64_t i = 0; i < n; i++) {
    EdH::Ext sum;
    for (uint32_t j = 0; j < k; j++) {
      EdHostCheck::Pt p;
      EdHostCheck::load((const uint8_t*)terms[j].points + i * (size_t)terms[j].point_stride, p);
      const EdH::Ext tj = ed_mul_bits_host(EdH::make_base(p.x, p.y), (const uint8_t*)terms[j].scalars + i * (size_t)terms[j].scalar_stride);
      sum = j ? EdH::add(sum, tj) : tj;
    }
    edh_to_wire(sum, out_points + i * 64);
  }
  return MSM377_OK;
}

}  // namespace msm377
