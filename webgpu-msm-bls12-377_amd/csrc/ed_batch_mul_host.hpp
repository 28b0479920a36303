// Host implementation of the Edwards-BLS12 batch multiplication (msm377_ed_batch_mul_multi_host): out[i] = sum_j [s_ij]B_j
// on one thread with the host tail's field and point code (fp64_host.hpp).  The yardstick of the device call
// (kernels/ed_batch_mul.hpp): plain double-and-add over the bits of every scalar, a general addition per further term, one
// inversion per output -- no window table, no signed recode, 64-bit words instead of 29-bit limbs.  Shared with the
// device: the argument checks below and nothing else.  No device code, no context; compiles with plain g++.
#pragma once
#include <string.h>

#include "common.hpp"
#include "fp64_host.hpp"
#include "validate_host.hpp"

namespace msm377 {

// k in 1 .. MSM377_MUL_MAX_BASES; both strides non-zero multiples of 32.
inline bool ed_batch_mul_shape_ok(uint32_t k, uint64_t out_stride, uint64_t base_stride) {
  return k >= 1 && k <= MSM377_MUL_MAX_BASES && out_stride != 0 && base_stride != 0 && out_stride % 32 == 0 && base_stride % 32 == 0;
}

// 64 wire bytes per base: both coordinates below q and the point on the curve.  The addition law is complete on the curve
// and nowhere else: what the batched inversion of the device call relies on (every Z non-zero).
inline bool ed_batch_mul_bases_ok(const uint8_t* bases_xy, uint32_t k) {
  for (uint32_t j = 0; j < k; j++) {
    EdHostCheck::Pt p;
    if (!EdHostCheck::load(bases_xy + (size_t)j * 64, p) || !EdHostCheck::on_curve(p)) return false;
  }
  return true;
}

// [s]B, s the 256-bit integer in the 32 little-endian bytes at `scalar`: not reduced, every value legal.
inline EdH::Ext ed_mul_bits_host(const EdH::Base& b, const uint8_t* scalar) {
  EdH::Ext acc = EdH::identity();
  int top = 255;
  while (top >= 0 && !((scalar[top >> 3] >> (top & 7)) & 1)) top--;
  for (int bit = top; bit >= 0; bit--) {
    acc = EdH::dbl(acc);
    if ((scalar[bit >> 3] >> (bit & 7)) & 1) acc = EdH::madd(acc, b);
  }
  return acc;
}

// s_ij: the 32 bytes at scalars + i * out_stride + j * base_stride.  Outputs: 64-byte wire records x || y, the identity
// as (0, 1).  MSM377_EINVAL leaves the outputs untouched.
inline int ed_batch_mul_multi_host(const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  if (!ed_batch_mul_shape_ok(k, out_stride, base_stride)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  if (!bases_xy || !scalars || !out_points) return MSM377_EINVAL;
  if (!ed_batch_mul_bases_ok(bases_xy, k)) return MSM377_EINVAL;
  EdH::Base base[MSM377_MUL_MAX_BASES];
  for (uint32_t j = 0; j < k; j++) {
    EdHostCheck::Pt p;
    EdHostCheck::load(bases_xy + (size_t)j * 64, p);
    base[j] = EdH::make_base(p.x, p.y);
  }
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* row = scalars + i * out_stride;
    EdH::Ext acc = ed_mul_bits_host(base[0], row);
    for (uint32_t j = 1; j < k; j++) acc = EdH::add(acc, ed_mul_bits_host(base[j], row + (uint64_t)j * base_stride));
    edh_to_wire(acc, out_points + i * 64);
  }
  return MSM377_OK;
}

}  // namespace msm377
