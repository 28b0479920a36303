// Host implementation of the input checks (msm377_*_check_points_host): the same cascade as kernels/validate.hpp --
// canonical, on the curve, [order]P = O -- on one thread with the host tail's fields and point code (fp64_host.hpp).
// The second, independent implementation the GPU report is compared with: 64-bit words instead of 29-bit limbs, the
// curve equation in Montgomery form, and plain double-and-add over the BITS of the order instead of the kernels'
// signed-digit chain.  No device code.
#pragma once
#include "common.hpp"
#include "fp64_host.hpp"

namespace msm377 {

// flags -> 1, 3 or 7 (a subgroup verdict needs a curve point, the curve equation a canonical one); 0: invalid.
inline uint32_t check_flags_normal(uint32_t flags) {
  if (flags == 0 || (flags & ~MSM377_CHECK_ALL)) return 0;
  if (flags & MSM377_CHECK_SUBGROUP) return MSM377_CHECK_ALL;
  if (flags & MSM377_CHECK_CURVE) return MSM377_CHECK_CANONICAL | MSM377_CHECK_CURVE;
  return MSM377_CHECK_CANONICAL;
}
inline void check_report_empty(msm377_check_report* r, uint64_t n) {
  memset(r, 0, sizeof *r);
  r->checked = n;
  r->first_bad = UINT64_MAX;
}

struct G1HostCheck {
  static constexpr int POINT_BYTES = 96;
  using F = Fp64;
  struct Pt {
    G1H::Affine a;
  };
  static bool load(const uint8_t* rec, Pt& p) {  // false: a coordinate is not below p
    uint64_t lim[2][6];
    memcpy(lim, rec, 96);  // little-endian host
    if (Fp64::geq_p(lim[0]) || Fp64::geq_p(lim[1])) return false;
    Fp64::El x, y;
    memcpy(x.v, lim[0], 48);
    memcpy(y.v, lim[1], 48);
    p.a.x = Fp64::mul(x, Fp64::from_const(G1Consts64::R2));
    p.a.y = Fp64::mul(y, Fp64::from_const(G1Consts64::R2));
    return true;
  }
  static bool on_curve(const Pt& p) {  // y^2 = x^3 + 1
    const Fp64::El x3 = Fp64::mul(Fp64::sqr(p.a.x), p.a.x);
    return Fp64::eq(Fp64::sqr(p.a.y), Fp64::add(x3, Fp64::one()));
  }
  static bool in_subgroup(const Pt& p) {
    G1H::XYZZ acc = G1H::identity();
    for (int b = CheckConsts::G1_ORDER_BITS - 1; b >= 0; b--) {
      acc = G1H::dbl(acc);  // identity and Y = 0 handled inside
      if ((CheckConsts::G1_ORDER64[b >> 6] >> (b & 63)) & 1) acc = G1H::madd(acc, p.a);  // identity, equal, opposite handled inside
    }
    return G1H::is_identity(acc);
  }
};

struct EdHostCheck {
  static constexpr int POINT_BYTES = 64;
  struct Pt {
    Fq64::El x, y;
  };
  static bool load(const uint8_t* rec, Pt& p) {
    uint64_t lim[2][4];
    memcpy(lim, rec, 64);
    if (Fq64::geq_p(lim[0]) || Fq64::geq_p(lim[1])) return false;
    Fq64::El x, y;
    memcpy(x.v, lim[0], 32);
    memcpy(y.v, lim[1], 32);
    p.x = Fq64::mul(x, Fq64::from_const(EdConsts64::R2));
    p.y = Fq64::mul(y, Fq64::from_const(EdConsts64::R2));
    return true;
  }
  static bool on_curve(const Pt& p) {  // -x^2 + y^2 = 1 + d x^2 y^2
    const Fq64::El xx = Fq64::sqr(p.x), yy = Fq64::sqr(p.y);
    const Fq64::El rhs = Fq64::add(Fq64::one(), Fq64::mul(Fq64::mul(xx, yy), Fq64::from_const(EdConsts64::ED_D)));
    return Fq64::eq(Fq64::sub(yy, xx), rhs);
  }
  static bool in_subgroup(const Pt& p) {  // the law is complete on the curve: no cases
    const EdH::Base q = EdH::make_base(p.x, p.y);
    EdH::Ext acc = EdH::identity();
    for (int b = CheckConsts::ED_ORDER_BITS - 1; b >= 0; b--) {
      acc = EdH::dbl(acc);
      if ((CheckConsts::ED_ORDER64[b >> 6] >> (b & 63)) & 1) acc = EdH::madd(acc, q);
    }
    return Fq64::is_zero(acc.x) && Fq64::eq(acc.y, acc.z);
  }
};

// flags: normalised (1, 3 or 7).  A point is counted once, in the first class it fails.
template <class CK>
inline void check_points_host(const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* r) {
  check_report_empty(r, n);
  for (uint64_t i = 0; i < n; i++) {
    typename CK::Pt p;
    uint32_t reason = 0;
    if (!CK::load(points + i * CK::POINT_BYTES, p)) {
      reason = MSM377_CHECK_CANONICAL;
      r->noncanonical++;
    } else if ((flags & MSM377_CHECK_CURVE) && !CK::on_curve(p)) {
      reason = MSM377_CHECK_CURVE;
      r->off_curve++;
    } else if ((flags & MSM377_CHECK_SUBGROUP) && !CK::in_subgroup(p)) {
      reason = MSM377_CHECK_SUBGROUP;
      r->outside_subgroup++;
    }
    if (reason && r->first_bad == UINT64_MAX) {
      r->first_bad = i;
      r->first_bad_reason = reason;
    }
  }
}

}  // namespace msm377
