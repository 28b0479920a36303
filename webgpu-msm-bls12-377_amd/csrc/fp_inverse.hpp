// One inversion in the 13-limb base field without a 377-squaring chain: Kaliski's "almost Montgomery inverse" (binary
// extended Euclid: shifts, additions and comparisons on 384-bit integers), then four field products that take
// a^-1 2^k back to the Montgomery form.  For the ONE lane that inverts a chunk's product in k_bm_across
// (kernels/batch_mul.hpp): a Fermat inversion there is ~570 dependent field products on a single lane, ~2 ms against 0.35 measured
// (profiles/batch_mul/sweep_fermat.txt against sweep.txt) -- the whole GPU waits for it; this walk is at most 754 steps of ~100
// plain 32-bit instructions.  The control flow depends on the data: for a single lane, never for a wave of 64 operands.
// Host-visible (MSM_HD) so that tests/native/batch_mul_host.cpp runs the very same code on the CPU.
#pragma once
#include "field29.hpp"

namespace msm377 {

struct FpInverse {
  static constexpr int NW = 12;  // 384 bits: p < 2^377, and every intermediate stays below 2p
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

  // a: a Montgomery residue x R (any form the canonical products accept), x != 0 mod p.  Returns x^-1 R, canonical.
  // Kaliski, phase 1: with u = p, v = a, r = 0, s = 1 the invariants are a r = -u 2^k, a s = v 2^k (mod p) and
  // u s + v r = p, so r, s <= p until the last step and r < 2p after it; it ends with u = 1, v = 0, p - r = a^-1 2^k,
  // 377 <= k <= 754.
  static MSM_HD Fp::El inverse_mont(const Fp::El& a_in) {
    using K = G1Consts;
    W u, v, r, s, p;
    Fp::to_words<NW>(Fp::from_const(K::MOD), p.w);
    Fp::to_words<NW>(Fp::mul(a_in, Fp::one()), v.w);  // a again (a R / R), reduced below p
    u = p;
#pragma unroll
    for (int j = 0; j < NW; j++) r.w[j] = s.w[j] = 0;
    s.w[0] = 1;
    int k = 0;
    while (!is_zero(v) && k < 2 * 384) {
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
    if (!greater(p, r)) sub(r, p);  // r >= p
    W x = p;
    sub(x, r);  // a^-1 2^k mod p, in [1, p]
    // x R^2 2^-k: two products with R^2 (each multiplies by R), two with powers of two 2^j1, 2^j2 (each multiplies by
    // 2^(j - 406)), j1 + j2 = 812 - k in [58, 435], both at most 376 (2^376 < p).
    Fp::El e = Fp::from_words<NW>(x.w);
    e = Fp::mul(Fp::mul(e, Fp::from_const(K::R2)), Fp::from_const(K::R2));
    int j1 = 812 - k, j2 = 0;
    if (j1 > 376) {
      j2 = j1 - 376;
      j1 = 376;
    }
    if (j1 < 0) j1 = 0;  // (k <= 754: unreachable; keeps the shifts below defined)
    Fp::El c1 = Fp::zero(), c2 = Fp::zero();
#pragma unroll
    for (int j = 0; j < Fp::N; j++) {
      if (j == j1 / LB) c1.l[j] = 1u << (j1 % LB);
      if (j == j2 / LB) c2.l[j] = 1u << (j2 % LB);
    }
    return Fp::mul(Fp::mul(e, c1), c2);
  }
};

}  // namespace msm377
