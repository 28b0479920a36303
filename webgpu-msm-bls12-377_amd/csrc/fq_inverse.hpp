// One inversion in the 9-limb field Fq (the base field of Edwards-BLS12) without a 253-squaring chain: fp_inverse.hpp's
// walk -- Kaliski's "almost Montgomery inverse", a binary extended Euclid on 256-bit integers -- and four field products
// that take a^-1 2^k back to the Montgomery form.  For the ONE lane that inverts a pass's product in k_edbm_across
// (kernels/ed_batch_mul.hpp).  fp_inverse.hpp is 13-limb code over 384-bit words and stays as it is: the G1 kernels do not
// change with this file.  The control flow depends on the data: for a single lane, never for a wave of 64 operands.
// Host-visible (MSM_HD) so that tests/native/ed_batch_mul_host.cpp runs the very same code on the CPU.
#pragma once
#include "field29.hpp"

namespace msm377 {

struct FqInverse {
  static constexpr int NW = 8;  // 256 bits: q < 2^253, and every intermediate stays below 2q
  struct W {
    uint32_t w[NW];
  };
  static MSM_HD bool is_zero(const W& a) {
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) acc |= a.w[j];
    return acc == 0;
  }
  static MSM_HD bool greater(const W& a, const W& b) {  // a > b: the borrow out of b - a
    uint64_t bw = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) bw = ((uint64_t)b.w[j] - a.w[j] - bw) >> 63;
    return bw != 0;
  }
  static MSM_HD void sub(W& a, const W& b) {  // a -= b (a >= b)
    uint64_t bw = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      const uint64_t d = (uint64_t)a.w[j] - b.w[j] - bw;
      a.w[j] = (uint32_t)d;
      bw = d >> 63;
    }
  }
  static MSM_HD void add(W& a, const W& b) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      c += (uint64_t)a.w[j] + b.w[j];
      a.w[j] = (uint32_t)c;
      c >>= 32;
    }
  }
  static MSM_HD void shr1(W& a) {
#pragma unroll
    for (int j = 0; j < NW - 1; j++) a.w[j] = (a.w[j] >> 1) | (a.w[j + 1] << 31);
    a.w[NW - 1] >>= 1;
  }
  static MSM_HD void shl1(W& a) {
#pragma unroll
    for (int j = NW - 1; j > 0; j--) a.w[j] = (a.w[j] << 1) | (a.w[j - 1] >> 31);
    a.w[0] <<= 1;
  }

  // a: a Montgomery residue x R (R = 2^261; any form the canonical products accept), x != 0 mod q.  Returns x^-1 R,
  // canonical.  Phase 1 as in fp_inverse.hpp: with u = q, v = a, r = 0, s = 1 the invariants are a r = -u 2^k,
  // a s = v 2^k (mod q) and u s + v r = q; it ends with u = 1, v = 0, q - r = a^-1 2^k, 253 <= k <= 506.
  static MSM_HD Fq::El inverse_mont(const Fq::El& a_in) {
    using K = EdConsts;
    W u, v, r, s, p;
    Fq::to_words<NW>(Fq::from_const(K::MOD), p.w);
    Fq::to_words<NW>(Fq::mul(a_in, Fq::one()), v.w);  // a again (a R / R), reduced below q
    u = p;
#pragma unroll
    for (int j = 0; j < NW; j++) r.w[j] = s.w[j] = 0;
    s.w[0] = 1;
    int k = 0;
    while (!is_zero(v) && k < 2 * 256) {
      if (!(u.w[0] & 1u)) {
        shr1(u);
        shl1(s);
      } else if (!(v.w[0] & 1u)) {
        shr1(v);
        shl1(r);
      } else if (greater(u, v)) {
        sub(u, v);
        shr1(u);
        add(r, s);
        shl1(s);
      } else {
        sub(v, u);
        shr1(v);
        add(s, r);
        shl1(r);
      }
      k++;
    }
    if (!greater(p, r)) sub(r, p);  // r >= q
    W x = p;
    sub(x, r);  // a^-1 2^k mod q, in [1, q]
    // x R^2 2^-k: two products with R^2 (each multiplies by R), two with powers of two 2^j1, 2^j2 (each multiplies by
    // 2^(j - 261)), j1 + j2 = 522 - k in [16, 269], both at most 252 (2^252 < q).
    Fq::El e = Fq::from_words<NW>(x.w);
    e = Fq::mul(Fq::mul(e, Fq::from_const(K::R2)), Fq::from_const(K::R2));
    int j1 = 522 - k, j2 = 0;
    if (j1 > 252) {
      j2 = j1 - 252;
      j1 = 252;
    }
    if (j1 < 0) j1 = 0;  // (k <= 506: unreachable; keeps the shifts below defined)
    Fq::El c1 = Fq::zero(), c2 = Fq::zero();
#pragma unroll
    for (int j = 0; j < Fq::N; j++) {
      if (j == j1 / LB) c1.l[j] = 1u << (j1 % LB);
      if (j == j2 / LB) c2.l[j] = 1u << (j2 % LB);
    }
    return Fq::mul(Fq::mul(e, c1), c2);
  }
};

}  // namespace msm377
