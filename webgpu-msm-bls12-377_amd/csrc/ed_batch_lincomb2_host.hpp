// Host implementation of the Edwards-BLS12 pairwise linear combination (msm377_ed_batch_lincomb2_host):
// out[i] = [a_i]P_i + [b_i]Q_i on one thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of
// the device call (kernels/ed_batch_lincomb2.hpp): each term by plain double-and-add over the bits of its scalar on the
// canonical formulas, then ONE general addition and one inversion per output -- no table, no signed recode, no shared
// doublings, no lazy forms.  Shared with the device call: the stride rule, the order of a refusal and its text, and
// nothing else (the device call checks its points with k_check_curve<EdCheck>).  No device code, no context; compiles
// with plain g++.
#pragma once
#include <string.h>

#include <string>

#include "common.hpp"
#include "ed_batch_mul_host.hpp"
#include "ed_batch_mul_var_host.hpp"
#include "fp64_host.hpp"
#include "validate_host.hpp"

namespace msm377 {

// a_stride, b_stride: 32 or 0; p_stride, q_stride: 64 or 0.  0: ONE scalar / ONE point for all n pairs.
inline bool ed_batch_lincomb2_strides_ok(uint32_t p_stride, uint32_t q_stride, uint32_t a_stride, uint32_t b_stride) {
  return (p_stride == 0 || p_stride == 64) && (q_stride == 0 || q_stride == 64) && ed_batch_mul_var_stride_ok(a_stride) && ed_batch_mul_var_stride_ok(b_stride);
}

// Which of two findings is reported: the lower index; p where they are equal.  UINT64_MAX: no finding in that array.
inline bool ed_batch_lincomb2_q_first(uint64_t bad_p, uint64_t bad_q) { return bad_q < bad_p; }

// The finding of both arrays (a stride-0 array is ONE point, index 0): false if every point is a curve point; else
// *array (0: p, 1: q), *index in that array and *reason (MSM377_CHECK_CANONICAL / MSM377_CHECK_CURVE).
inline bool ed_batch_lincomb2_first_bad(const uint8_t* p, const uint8_t* q, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t* array, uint64_t* index, uint32_t* reason) {
  uint32_t why_p = 0, why_q = 0;
  const uint64_t bad_p = ed_batch_mul_var_first_bad(p, p_stride ? n : 1, &why_p), bad_q = ed_batch_mul_var_first_bad(q, q_stride ? n : 1, &why_q);
  if (bad_p == UINT64_MAX && bad_q == UINT64_MAX) return false;
  const bool in_q = ed_batch_lincomb2_q_first(bad_p, bad_q);
  *array = in_q ? 1u : 0u;
  *index = in_q ? bad_q : bad_p;
  *reason = in_q ? why_q : why_p;
  return true;
}

// The text msm377_last_error carries behind MSM377_EPOINT, from the device's finding or the host's.
inline std::string ed_batch_lincomb2_refusal(uint32_t array, uint64_t index, uint32_t reason) {
  return "point " + std::to_string(index) + " of " + (array ? "q" : "p") + (reason == MSM377_CHECK_CANONICAL ? " has a coordinate that is not below q" : " is not on the curve") +
         ": the linear combination takes curve points only";
}

// P_i: the 64 bytes x || y at p + i * p_stride, Q_i likewise; a_i: the 32 bytes at a + i * a_stride, b_i likewise, read as
// integers and not reduced.  Outputs: 64-byte wire records, the identity as (0, 1).  out_points may be p or q where that
// array's stride is 64, and the fold in place (q = p + 64 h, out = p, n = h) works: pair i is read before output i is
// written, and no later pair reads record i.  out_points equal to a stride-0 array is MSM377_EINVAL.  MSM377_EINVAL and
// MSM377_EPOINT leave the outputs untouched.
inline int ed_batch_lincomb2_host(const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                                  uint32_t b_stride, uint8_t* out_points) {
  if (!ed_batch_lincomb2_strides_ok(p_stride, q_stride, a_stride, b_stride)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!p || !q || !a || !b || !out_points) return MSM377_EINVAL;
  if ((p_stride == 0 && out_points == p) || (q_stride == 0 && out_points == q)) return MSM377_EINVAL;
  uint32_t array = 0, reason = 0;
  uint64_t index = 0;
  if (ed_batch_lincomb2_first_bad(p, q, n, p_stride, q_stride, &array, &index, &reason)) return MSM377_EPOINT;
  for (uint64_t i = 0; i < n; i++) {
    EdHostCheck::Pt pp, qq;
    EdHostCheck::load(p + i * (size_t)p_stride, pp);
    EdHostCheck::load(q + i * (size_t)q_stride, qq);
    const EdH::Ext ta = ed_mul_bits_host(EdH::make_base(pp.x, pp.y), a + i * (size_t)a_stride);
    const EdH::Ext tb = ed_mul_bits_host(EdH::make_base(qq.x, qq.y), b + i * (size_t)b_stride);
    edh_to_wire(EdH::add(ta, tb), out_points + i * 64);
  }
  return MSM377_OK;
}

}  // namespace msm377
