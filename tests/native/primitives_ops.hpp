// TEST INFRASTRUCTURE: one op-code dispatch over the product's field and curve primitives, on RAW limbs (no to_mont, no
// from_words: the caller chooses every limb).  The same text is compiled twice -- by g++ into the host shim
// (field29_shim.cpp) and by hipcc into the gfx950 test library (primitives_device.hip) -- so that the tests can ask for
// device == host bit for bit.  The op numbers are mirrored in tests/lazy_model.py.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "ed_ext.hpp"
#include "fp_inverse.hpp"
#include "fq_inverse.hpp"
#include "g1_xyzz.hpp"
#include "te377.hpp"

namespace primtest {
using namespace msm377;

enum FieldOp {
  F_MUL_LZ = 0,
  F_SQR_LZ,
  F_MUL_ADD_MUL_LZ,
  F_MUL,
  F_SQR,
  F_MUL_SUB_MUL,
  F_ADD,
  F_SUB,
  F_NEG,
  F_REDUCE_ONCE,
  F_NORM,
  F_CSUB_MOD,
  F_CSUB_MOD2,
  F_CSUB_MOD4,
  F_CANON,
  F_ADD_KP2_SUB,
  F_ADD_KP6_SUB,
  F_ADD_KP4W3_SUB_SUB2,
  F_KP2_SUB,
  F_ADD_LZ,
  F_INVERSE_MONT,  // FpInverse / FqInverse::inverse_mont: a data-dependent walk, one branch sequence per case
  F_NUM_OPS
};
enum TeOp { T_MADD = 0, T_MADD_AFFINE, T_ADD, T_FINISH, T_FROM_BASE, T_FROM_BASE_AFFINE, T_IS_ZERO, T_NUM_OPS };
enum G1Op { G_MADD_LZ = 0, G_ADD_LZ, G_CANON_PT, G_DBL, G_DBL_AFFINE, G_NUM_OPS };
enum EdOp { E_MADD = 0, E_ADD, E_DBL, E_DBL_NT, E_MAKE_BASE, E_CNEG, E_NUM_OPS };  // the strict EdT<Fq, EdK29> (ed_ext.hpp)

template <class F>
MSM_HD typename F::El ld(const uint32_t* w) {
  typename F::El r;
#pragma unroll
  for (int j = 0; j < F::N; j++) r.l[j] = w[j];
  return r;
}
template <class F>
MSM_HD void st(uint32_t* w, const typename F::El& a) {
#pragma unroll
  for (int j = 0; j < F::N; j++) w[j] = a.l[j];
}

// out = op(a, b, c, d); operands an op does not take are ignored.  N limbs each.
template <class F>
MSM_HD void field_op(int op, const uint32_t* pa, const uint32_t* pb, const uint32_t* pc, const uint32_t* pd, uint32_t* out) {
  using K = typename F::Consts;
  using El = typename F::El;
  const El a = ld<F>(pa), b = ld<F>(pb), c = ld<F>(pc), d = ld<F>(pd);
  El r = F::zero();
  switch (op) {
    case F_MUL_LZ: r = F::mul_lz(a, b); break;
    case F_SQR_LZ: r = F::sqr_lz(a); break;
    case F_MUL_ADD_MUL_LZ: r = F::mul_add_mul_lz(a, b, c, d); break;
    case F_MUL: r = F::mul(a, b); break;
    case F_SQR: r = F::sqr(a); break;
    case F_MUL_SUB_MUL: r = F::mul_sub_mul(a, b, c, d); break;
    case F_ADD: r = F::add(a, b); break;
    case F_SUB: r = F::sub(a, b); break;
    case F_NEG: r = F::neg(a); break;
    case F_REDUCE_ONCE: r = F::reduce_once(a); break;
    case F_NORM: r = F::norm(a); break;
    case F_CSUB_MOD: r = F::csub(a, K::MOD); break;
    case F_CSUB_MOD2: r = F::csub(a, K::MOD2); break;
    case F_CSUB_MOD4: r = F::csub(a, K::MOD4); break;
    case F_CANON: r = F::canon(a); break;
    case F_ADD_KP2_SUB: r = F::add_kp_sub(a, K::KP2, b); break;
    case F_ADD_KP6_SUB: r = F::add_kp_sub(a, K::KP6, b); break;
    case F_ADD_KP4W3_SUB_SUB2: r = F::add_kp_sub_sub2(a, K::KP4W3, b, c); break;
    case F_KP2_SUB: r = F::kp_sub(K::KP2, a); break;
    case F_ADD_LZ: r = F::add_lz(a, b); break;
    case F_INVERSE_MONT:
      if constexpr (std::is_same<F, Fp>::value) r = FpInverse::inverse_mont(a);
      else r = FqInverse::inverse_mont(a);
      break;
    default: break;
  }
  st<F>(out, r);
}

// p: 4 N limbs (X, Y, T, Z -- for T_FINISH the four products A, B, C, D).  q: 4 N limbs, a PBase (ymx, ypx, kt, z2), an
// ABase (ymx, ypx, kt, unused) or a second Ext.  out: 4 N limbs.  Returns bit 0 = is_bad(out), or for T_IS_ZERO
// bit 0 = is_zero_mod_p(p.x), bit 1 = is_bad(p).
template <class TE>
MSM_HD uint32_t te_op(int op, const uint32_t* pp, const uint32_t* pq, uint32_t neg, uint32_t* out) {
  using F = typename TE::F;
  constexpr int N = F::N;
  typename TE::Ext p, o = TE::identity();
  p.x = ld<F>(pp), p.y = ld<F>(pp + N), p.t = ld<F>(pp + 2 * N), p.z = ld<F>(pp + 3 * N);
  typename TE::PBase pb;
  pb.ymx = ld<F>(pq), pb.ypx = ld<F>(pq + N), pb.kt = ld<F>(pq + 2 * N), pb.z2 = ld<F>(pq + 3 * N);
  typename TE::ABase ab;
  ab.ymx = pb.ymx, ab.ypx = pb.ypx, ab.kt = pb.kt;
  typename TE::Ext q;
  q.x = pb.ymx, q.y = pb.ypx, q.t = pb.kt, q.z = pb.z2;
  uint32_t flags = 0;
  switch (op) {
    case T_MADD: o = TE::madd(p, pb, neg != 0); break;
    case T_MADD_AFFINE: o = TE::madd_affine(p, ab, neg != 0); break;
    case T_ADD: o = TE::add(p, q); break;
    case T_FINISH: o = TE::finish(p.x, p.y, p.t, p.z); break;
    case T_FROM_BASE:
      if constexpr (std::is_same<TE, Te377>::value) o = TE::from_base(pb, neg != 0);
      break;
    case T_FROM_BASE_AFFINE:
      if constexpr (std::is_same<TE, Te377>::value) o = TE::from_base_affine(ab, neg != 0);
      break;
    case T_IS_ZERO:
      o = p;
      flags = (TE::is_zero_mod_p(p.x) ? 1u : 0u) | (TE::is_bad(p) ? 2u : 0u);
      break;
    default: break;
  }
  if (op != T_IS_ZERO) flags = TE::is_bad(o) ? 1u : 0u;
  st<F>(out, o.x), st<F>(out + N, o.y), st<F>(out + 2 * N, o.t), st<F>(out + 3 * N, o.z);
  return flags;
}

// a: XYZZ, 52 limbs.  q: an affine point (x, y: 26 limbs used) or a second XYZZ (52).  out: 52 limbs.
MSM_HD void g1_op(int op, const uint32_t* pa, const uint32_t* pq, uint32_t neg, uint32_t* out) {
  G1XYZZ a, b, o = G1::identity();
  a.x = ld<Fp>(pa), a.y = ld<Fp>(pa + 13), a.zz = ld<Fp>(pa + 26), a.zzz = ld<Fp>(pa + 39);
  b.x = ld<Fp>(pq), b.y = ld<Fp>(pq + 13), b.zz = ld<Fp>(pq + 26), b.zzz = ld<Fp>(pq + 39);
  G1Affine q;
  q.x = b.x, q.y = b.y;
  switch (op) {
    case G_MADD_LZ: o = G1::madd_lz(a, q, neg != 0); break;
    case G_ADD_LZ: o = G1::add_lz(a, b); break;
    case G_CANON_PT: o = G1::canon_pt(a); break;
    case G_DBL: o = G1::dbl(a); break;
    case G_DBL_AFFINE: o = G1::dbl_affine(q); break;
    default: break;
  }
  st<Fp>(out, o.x), st<Fp>(out + 13, o.y), st<Fp>(out + 26, o.zz), st<Fp>(out + 39, o.zzz);
}

// The strict (canonical in, canonical out) Edwards-BLS12 formulas the batch kernels build their tables with.  p: an Ext
// (X, Y, T, Z), 36 limbs.  q: a Base (ymx, ypx, kt: 27 limbs used) or a second Ext.  out: 36 limbs -- an Ext, or for
// E_MAKE_BASE (from p.x, p.y) and E_CNEG (of q) a Base in the first 27 and zeros behind it.
MSM_HD void ed_op(int op, const uint32_t* pp, const uint32_t* pq, uint32_t neg, uint32_t* out) {
  Ed::Ext p, q, o;
  p.x = ld<Fq>(pp), p.y = ld<Fq>(pp + 9), p.t = ld<Fq>(pp + 18), p.z = ld<Fq>(pp + 27);
  q.x = ld<Fq>(pq), q.y = ld<Fq>(pq + 9), q.t = ld<Fq>(pq + 18), q.z = ld<Fq>(pq + 27);
  Ed::Base b, ob;
  b.ymx = q.x, b.ypx = q.y, b.kt = q.t;
  o.x = o.y = o.t = o.z = Fq::zero();
  bool base_out = false;
  switch (op) {
    case E_MADD: o = Ed::madd(p, b); break;
    case E_ADD: o = Ed::add(p, q); break;
    case E_DBL: o = Ed::dbl(p); break;
    case E_DBL_NT: o = Ed::dbl_nt(p); break;
    case E_MAKE_BASE: ob = Ed::make_base(p.x, p.y), base_out = true; break;
    case E_CNEG: ob = Ed::cneg(b, neg != 0), base_out = true; break;
    default: break;
  }
  if (base_out) o.x = ob.ymx, o.y = ob.ypx, o.t = ob.kt;
  st<Fq>(out, o.x), st<Fq>(out + 9, o.y), st<Fq>(out + 18, o.t), st<Fq>(out + 27, o.z);
}

}  // namespace primtest
