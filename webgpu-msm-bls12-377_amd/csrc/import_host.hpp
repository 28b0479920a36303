// Host implementation of the native input forms (msm377_g1_import_points_host, msm377_import_scalars_host,
// msm377_g1_result_to_native): the conversions of kernels/import.hpp on one thread with the host tail's fields
// (fp64_host.hpp), whose Montgomery radices -- 2^384 and 2^256 -- ARE the callers': an import is one Montgomery reduction,
// the way back one product with R^2.  The second, independent implementation the device pass is compared with: 64-bit
// words instead of 29-bit limbs, no constant of the form 2^k.  No device code.
#pragma once
#include <string.h>

#include "common.hpp"
#include "fp64_host.hpp"

namespace msm377 {

// One point: 96 coordinate bytes in Montgomery form -> the wire record.  A coordinate of p or more is no residue: the
// record is handed on unchanged (the check calls then count it as non-canonical), as the device pass does.
inline void import_point_host(const uint8_t* rec, uint8_t* out) {
  uint64_t lim[2][6];
  memcpy(lim, rec, 96);  // little-endian host
  if (Fp64::geq_p(lim[0]) || Fp64::geq_p(lim[1])) {
    memmove(out, rec, 96);
    return;
  }
  Fp64::El x, y;
  memcpy(x.v, lim[0], 48);
  memcpy(y.v, lim[1], 48);
  Fp64::to_wire(x, out);
  Fp64::to_wire(y, out + 48);
}

// out_inf_mask (may be null): ceil(n / 32) words, bit i mod 32 of word i / 32 set for a flagged point; all zero for the
// forms without flags.  A flagged point's record is the generator's, whatever its coordinate bytes hold.
inline void import_points_host(const uint8_t* in, uint64_t n, uint32_t form, uint8_t* out_wire, uint32_t* out_inf_mask) {
  if (out_inf_mask) memset(out_inf_mask, 0, (size_t)((n + 31) / 32) * 4);
  const size_t stride = form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* rec = in + i * stride;
    uint8_t* out = out_wire + i * 96;
    if (form == MSM377_POINTS_WIRE) {
      memmove(out, rec, 96);
    } else if (form == MSM377_POINTS_MONT_FLAG && rec[96] != 0) {
      memcpy(out, G1Consts::GEN_WIRE, 96);
      if (out_inf_mask) out_inf_mask[i >> 5] |= 1u << (i & 31);
    } else {
      import_point_host(rec, out);
    }
  }
}

// Every 32-byte value v is accepted and means v / 2^256 mod r, fully reduced: the reduction of v < 2^256 leaves at most
// r, which the product's own conditional subtraction takes to [0, r).
inline void import_scalars_host(const uint8_t* in, uint64_t n, uint32_t form, uint8_t* out_wire) {
  for (uint64_t i = 0; i < n; i++) {
    if (form == MSM377_SCALARS_WIRE) {
      memmove(out_wire + i * 32, in + i * 32, 32);
      continue;
    }
    Fq64::El v;
    memcpy(v.v, in + i * 32, 32);
    Fq64::to_wire(v, out_wire + i * 32);
  }
}

// A wire result -> the callers' affine record: Montgomery x, y, flag byte, seven zero bytes.  The wire identity (0, 1)
// sets the flag (its coordinates are written all the same).  false: a coordinate is not below p.
inline bool result_to_native_host(const uint8_t xy[96], uint8_t out[104]) {
  uint64_t lim[2][6];
  memcpy(lim, xy, 96);
  if (Fp64::geq_p(lim[0]) || Fp64::geq_p(lim[1])) return false;
  Fp64::El x, y;
  memcpy(x.v, lim[0], 48);
  memcpy(y.v, lim[1], 48);
  uint64_t one[6] = {1, 0, 0, 0, 0, 0};
  const bool identity = Fp64::is_zero(x) && memcmp(lim[1], one, 48) == 0;
  x = Fp64::mul(x, Fp64::from_const(G1Consts64::R2));
  y = Fp64::mul(y, Fp64::from_const(G1Consts64::R2));
  memset(out, 0, 104);
  memcpy(out, x.v, 48);
  memcpy(out + 48, y.v, 48);
  out[96] = identity ? 1 : 0;
  return true;
}

}  // namespace msm377
