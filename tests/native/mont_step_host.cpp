// TEST INFRASTRUCTURE: the three lazy Montgomery products of csrc/field29.hpp (mul_lz, mul_add_mul_lz, sqr_lz) against
// the form they had before their reduction step went from five bookkeeping instructions to three: plain columns from 0,
// q = (0 - t0) & LMASK, carry = (t0 + q) >> 29.  That form is kept here VERBATIM as the reference (RefProducts): the
// new step must give the same limbs, every one, for every operand the contracts allow.
// Built two ways by tests/test_mont_step_host.py: as a shared library for ctypes (operands from numpy), and with
// -DMONT_STEP_MAIN as a stand-alone program that draws its own operands, for a run under -fsanitize=undefined,address.
#include <stdint.h>
#include <stdio.h>

#include "field29.hpp"

using namespace msm377;

template <class C>
struct RefProducts {
  static constexpr int N = C::NL;
  static constexpr int RS = C::RS;
  using El = Limbs<N>;

  // Lazy product: see above.  Output N-form with value < p + 2^354 (top limb <= MOD[N-1] + 64).
  static MSM_HD El mul_lz(const El& a, const El& b) {
    uint64_t t[N];
#pragma unroll
    for (int j = 0; j < N; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < RS; i++) {
      if (i < N) {
#pragma unroll
        for (int j = 0; j < N; j++) t[j] += (uint64_t)a.l[i] * b.l[j];
      }
      uint32_t q = (0u - (uint32_t)t[0]) & LMASK;
      uint64_t carry = (t[0] + q) >> LB;  // low 29 bits cancel exactly
#pragma unroll
      for (int j = 1; j < N; j++) t[j] += (uint64_t)q * C::MOD[j];
      t[1] += carry;
#pragma unroll
      for (int j = 0; j < N - 1; j++) t[j] = t[j + 1];
      t[N - 1] = 0;
    }
    El r;
#pragma unroll
    for (int j = 0; j < N - 1; j++) {
      r.l[j] = (uint32_t)t[j] & LMASK;
      t[j + 1] += t[j] >> LB;
    }
    r.l[N - 1] = (uint32_t)t[N - 1];
    return r;
  }

  // a*b + e*d in ONE reduction (Y3 = R (Q - X3) + (-Y1) PPP of every point addition): the quotient
  // digits serve both products.  Same output contract as mul_lz; the column bound covers both sums.
  static MSM_HD El mul_add_mul_lz(const El& a, const El& b, const El& e, const El& d) {
    uint64_t t[N];
#pragma unroll
    for (int j = 0; j < N; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < RS; i++) {
      if (i < N) {
#pragma unroll
        for (int j = 0; j < N; j++) t[j] += (uint64_t)a.l[i] * b.l[j];
#pragma unroll
        for (int j = 0; j < N; j++) t[j] += (uint64_t)e.l[i] * d.l[j];
      }
      uint32_t q = (0u - (uint32_t)t[0]) & LMASK;
      uint64_t carry = (t[0] + q) >> LB;
#pragma unroll
      for (int j = 1; j < N; j++) t[j] += (uint64_t)q * C::MOD[j];
      t[1] += carry;
#pragma unroll
      for (int j = 0; j < N - 1; j++) t[j] = t[j + 1];
      t[N - 1] = 0;
    }
    El r;
#pragma unroll
    for (int j = 0; j < N - 1; j++) {
      r.l[j] = (uint32_t)t[j] & LMASK;
      t[j + 1] += t[j] >> LB;
    }
    r.l[N - 1] = (uint32_t)t[N - 1];
    return r;
  }

  // Lazy square of an N-form value: off-diagonal terms once with a doubled operand (2 a_i < 2^30 for
  // i <= N-2; the top limb is never the doubled one).
  static MSM_HD El sqr_lz(const El& a) {
    uint64_t t[RS + N];
#pragma unroll
    for (int j = 0; j < RS + N; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
      t[2 * i] += (uint64_t)a.l[i] * a.l[i];
      const uint32_t a2 = a.l[i] << 1;
#pragma unroll
      for (int j = i + 1; j < N; j++) t[i + j] += (uint64_t)a2 * a.l[j];
    }
#pragma unroll
    for (int i = 0; i < RS; i++) {
      uint32_t q = (0u - (uint32_t)t[i]) & LMASK;
      uint64_t carry = (t[i] + q) >> LB;
#pragma unroll
      for (int j = 1; j < N; j++) t[i + j] += (uint64_t)q * C::MOD[j];
      t[i + 1] += carry;
    }
    El r;
#pragma unroll
    for (int j = 0; j < N - 1; j++) {
      r.l[j] = (uint32_t)t[RS + j] & LMASK;
      t[RS + j + 1] += t[RS + j] >> LB;
    }
    r.l[N - 1] = (uint32_t)t[RS + N - 1];
    return r;
  }
};

template <class C>
static int compare_one(int op, const uint32_t* a, const uint32_t* b, const uint32_t* e, const uint32_t* d, uint32_t* out) {
  using F = Field<C>;
  using Ref = RefProducts<C>;
  typename F::El x, y, z, w, got, exp;
  for (int j = 0; j < F::N; j++) {
    x.l[j] = a[j];
    y.l[j] = b[j];
    z.l[j] = e[j];
    w.l[j] = d[j];
  }
  if (op == 0) {
    got = F::mul_lz(x, y);
    exp = Ref::mul_lz(x, y);
  } else if (op == 1) {
    got = F::sqr_lz(x);
    exp = Ref::sqr_lz(x);
  } else {
    got = F::mul_add_mul_lz(x, y, z, w);
    exp = Ref::mul_add_mul_lz(x, y, z, w);
  }
  int diff = 0;
  for (int j = 0; j < F::N; j++) {
    diff |= got.l[j] != exp.l[j];
    if (out) out[j] = got.l[j];
  }
  return diff;
}

extern "C" {
// n cases, operands case-major (13 limbs for field 0 = Fp, 9 for field 1 = Fq); op 0 mul_lz(a, b), 1 sqr_lz(a),
// 2 mul_add_mul_lz(a, b, e, d).  Returns the number of cases whose limbs differ from the reference form (first_bad: the
// first of them); out (may be null) receives the new form's limbs.
uint32_t mont_step_compare(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* e, const uint32_t* d, uint32_t n, uint32_t* out,
                           uint32_t* first_bad) {
  uint32_t bad = 0;
  const int nl = field == 0 ? 13 : 9;
  for (uint32_t i = 0; i < n; i++) {
    const size_t at = (size_t)nl * i;
    const int diff = field == 0 ? compare_one<G1Consts>(op, a + at, b + at, e + at, d + at, out ? out + at : nullptr)
                                : compare_one<EdConsts>(op, a + at, b + at, e + at, d + at, out ? out + at : nullptr);
    if (diff && !bad++) *first_bad = i;
  }
  return bad;
}
}

#if defined(MONT_STEP_MAIN)
// Stand-alone run: operands in the shapes of field29.hpp's "Montgomery products" comment, from a fixed generator, and
// the corners of those shapes.  Exit status 1 on any difference.
static uint64_t rng_state = 0x377377377ull;
static uint32_t rnd_below(uint64_t bound_incl) {  // uniform enough for a test: [0, bound_incl]
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state % (bound_incl + 1));
}
struct Shape {
  uint32_t limb, top;  // inclusive maxima of limbs 0..N-2 and of the top limb
};
template <class C>
static int run_field(int field, const Shape* shapes, const int (*pairs)[2], int npairs, int cases) {
  constexpr int N = C::NL;
  int bad = 0;
  uint32_t v[4][N];
  for (int p = 0; p < npairs; p++) {
    for (int it = 0; it < cases; it++) {
      for (int k = 0; k < 4; k++) {
        const Shape& s = shapes[pairs[p][k & 1]];
        // it 0: the corner of the box; it 1: zero; it 2: column 0 a multiple of 2^29; then random
        for (int j = 0; j < N; j++) v[k][j] = it == 0 ? (j == N - 1 ? s.top : s.limb) : it == 1 ? 0u : rnd_below(j == N - 1 ? s.top : s.limb);
        if (it == 2) v[k][0] = (k & 1) ? 2u : (1u << 28);
      }
      for (int op = 0; op < 3; op++) {
        if (op == 1 && shapes[pairs[p][0]].limb > LMASK) continue;  // sqr_lz takes N-form values only
        if (op == 2 && p != 0) continue;                            // mul_add_mul_lz: two N x N sums fit, canonical here
        bad += compare_one<C>(op, v[0], v[1], v[2], v[3], nullptr);
      }
    }
  }
  printf("field %d: %d differences\n", field, bad);
  return bad;
}
int main() {
  // 0 canonical, 1 wide N-form (top < 2^31.6), 2 narrow N-form (top < 2^29.1), 3 lazy (limbs < 3 * 2^29, top < 2^31)
  const Shape fp[4] = {{LMASK, G1Consts::MOD[12] - 1}, {LMASK, 3254976540u}, {LMASK, 575403995u}, {3u * (1u << 29) - 1u, (1u << 31) - 1u}};
  const int fp_pairs[4][2] = {{0, 0}, {1, 1}, {3, 2}, {2, 3}};
  const Shape fq[1] = {{LMASK, EdConsts::MOD[8] - 1}};
  const int fq_pairs[1][2] = {{0, 0}};
  int bad = run_field<G1Consts>(0, fp, fp_pairs, 4, 20000);
  bad += run_field<EdConsts>(1, fq, fq_pairs, 1, 20000);
  return bad ? 1 : 0;
}
#endif
