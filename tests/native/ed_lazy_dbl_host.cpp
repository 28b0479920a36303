// Stand-alone driver of the lazy Edwards doubling (csrc/te377.hpp TeLazy::dbl / dbl_nt), the walk's recode
// (csrc/batch_mul_var_recode.hpp) and the host twin csrc/ed_batch_mul_var_host.hpp for
// tests/test_ed_batch_mul_var_host.py: compiled with g++ (and, once more, with the address / undefined-behaviour sanitizers)
// against the headers, no library, no device.
//   ed_lazy_dbl_host dbl <in>          in: 64-byte wire points.  For each: TeLazy<Fq, EdConsts>::dbl and dbl_nt against the
//                                      canonical Ed::dbl after Fq::canon, coordinate by coordinate, on the point as it is
//                                      loaded, on a projective image whose four coordinates sit at the upper end of the
//                                      stored form (q <= v < q + q / 16), and on the walk's chain -- (dbl_nt^3, dbl,
//                                      madd_affine) 64 times with both signs -- against Ed::dbl_nt / Ed::dbl / Ed::madd
//                                      step by step.  Prints the number of points.
//   ed_lazy_dbl_host bound             coordinates that are no curve point's (the formulas are polynomial identities): the
//                                      largest stored values q + q / 16 - 1 - r, small r, in every coordinate
//   ed_lazy_dbl_host recode <in>       in: 32-byte scalars; bmv_pack / bmv_next: s == sum_w d_w 16^w + carry 2^256, d_w in
//                                      -7 .. 8, carry in {0, 1}
//   ed_lazy_dbl_host run <in> <out>    in:  u64 n, u32 scalar_stride, u32 zero, then n x 64 point bytes and the scalar bytes
//                                           (n x 32, or 32 for stride 0; an allocation of exactly that size)
//                                      out: i32 return code, then (code 0) n records; after any other code the program
//                                           checks that the poisoned output is untouched
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_mul_var_recode.hpp"
#include "ed_batch_mul_var_host.hpp"
#include "ed_ext.hpp"
#include "te377.hpp"

using namespace msm377;

static uint64_t splitmix(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static bool same(const Fq::El& lazy, const Fq::El& canonical) { return Fq::eq(Fq::canon(lazy), canonical); }

static bool same_point(const EdLazy::Ext& a, const Ed::Ext& b, bool with_t) {
  return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z) && (!with_t || same(a.t, b.t));
}

static Ed::Ext canonical_of(const EdLazy::Ext& a) {
  Ed::Ext c;
  c.x = Fq::canon(a.x);
  c.y = Fq::canon(a.y);
  c.t = Fq::canon(a.t);
  c.z = Fq::canon(a.z);
  return c;
}

// One doubling of each kind from the same stored point.
static bool dbl_ok(const EdLazy::Ext& p) {
  const Ed::Ext c = canonical_of(p);
  return same_point(EdLazy::dbl(p), Ed::dbl(c), true) && same_point(EdLazy::dbl_nt(p), Ed::dbl_nt(c), false);
}

// v (canonical, below q / 16) + q: the same residue at the upper end of the stored form.
static Fq::El plus_q(const Fq::El& v) { return Fq::norm(Fq::add_lz(v, Fq::from_const(EdConsts::MOD))); }

// Is the canonical v below q / 16?  q has 253 bits: v < 2^248 suffices (2^248 < q / 16 < 2^249).
static bool small(const Fq::El& v) { return (v.l[8] >> (248 - 232)) == 0; }  // limb 8 holds bits 232 and up

// (lambda x, lambda y, lambda x y, lambda) of an affine p with every coordinate below q / 16, then q added to each.
// The point of order 2 is (0 : -lambda : 0 : lambda): Y and Z cannot both be small, Y stays canonical there.
static bool upper_image(const Ed::Ext& p, uint64_t& seed, EdLazy::Ext& out) {
  const bool y_too = !Fq::is_zero(Fq::add(p.y, p.z));
  for (int tries = 0; tries < 4000000; tries++) {
    uint32_t w[8];
    for (int k = 0; k < 4; k++) {
      const uint64_t z = splitmix(seed);
      w[2 * k] = (uint32_t)z;
      w[2 * k + 1] = (uint32_t)(z >> 32);
    }
    w[7] &= 0x00ffffffu;  // lambda below 2^248
    const Fq::El z = Fq::from_words<8>(w);  // lambda itself, in Montgomery form: small by construction (p is affine, Z = 1)
    if (Fq::is_zero(z)) continue;
    const Fq::El x = Fq::mul(p.x, z);
    if (!small(x)) continue;
    const Fq::El y = Fq::mul(p.y, z);
    if (y_too && !small(y)) continue;
    const Fq::El t = Fq::mul(p.t, z);
    if (!small(t)) continue;
    out.x = plus_q(x);
    out.y = y_too ? plus_q(y) : y;
    out.t = plus_q(t);
    out.z = plus_q(z);
    return true;
  }
  return false;
}

// The walk of k_edbmv_accumulate on one point with a fixed digit pattern, lazy against canonical, step by step.
static bool chain_ok(const Ed::Ext& p, const EdLazy::Ext& start) {
  const Ed::Base qc = Ed::make_base(p.x, p.y);  // p is affine here (z = 1)
  EdLazy::ABase ql;
  ql.ymx = qc.ymx;
  ql.ypx = qc.ypx;
  ql.kt = qc.kt;
  EdLazy::Ext a = start;
  Ed::Ext c = canonical_of(start);
  for (int w = 0; w < 64; w++) {
    for (int k = 0; k < 3; k++) {
      a = EdLazy::dbl_nt(a);
      c = Ed::dbl_nt(c);
      if (!same_point(a, c, false)) return false;
    }
    a = EdLazy::dbl(a);
    c = Ed::dbl(c);
    if (!same_point(a, c, true)) return false;
    if (w % 5 == 4) continue;  // a zero digit: dbl straight after dbl
    const bool neg = (w & 1) != 0;
    a = EdLazy::madd_affine(a, ql, neg);
    c = Ed::madd(c, Ed::cneg(qc, neg));
    if (!same_point(a, c, true)) return false;
  }
  return true;
}

static bool digits_ok(const uint32_t s[8]) {
  uint32_t packed[8];
  memcpy(packed, s, 32);
  const uint32_t carry = bmv_pack(packed);
  if (carry > 1) return false;
  int64_t acc[10] = {};
  for (int w = BMV_WINDOWS - 1; w >= 0; w--) {  // bmv_next hands the digits out from the top
    const int32_t d = bmv_next(packed);
    if (d < -7 || d > 8) return false;
    acc[(4 * w) >> 5] += (int64_t)d * ((int64_t)1 << ((4 * w) & 31));
  }
  for (int k = 0; k < 8; k++)
    if (packed[k] != 0) return false;  // 64 calls empty the array
  acc[8] += carry;
  int64_t run = 0;
  for (int i = 0; i < 10; i++) {
    const int64_t v = acc[i] + run;
    run = v >> 32;
    if ((uint32_t)(v & 0xffffffffll) != (i < 8 ? s[i] : 0u)) return false;
  }
  return run == 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "dbl")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t raw[16];
    int count = 0;
    uint64_t seed = 0xED2DB1;
    while (fread(raw, 4, 16, f) == 16) {
      Ed::Ext p;
      p.x = Fq::to_mont(Fq::from_words<8>(raw));
      p.y = Fq::to_mont(Fq::from_words<8>(raw + 8));
      p.t = Fq::mul(p.x, p.y);
      p.z = Fq::one();
      EdLazy::Ext l;
      l.x = p.x;
      l.y = p.y;
      l.t = p.t;
      l.z = p.z;
      EdLazy::Ext up;
      bool ok = dbl_ok(l) && chain_ok(p, l) && chain_ok(p, EdLazy::identity());
      ok = ok && upper_image(p, seed, up) && dbl_ok(up) && chain_ok(p, up);
      if (!ok) {
        fprintf(stderr, "dbl: point %d\n", count);
        fclose(f);
        return 1;
      }
      count++;
    }
    fclose(f);
    printf("%d\n", count);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "bound")) {
    // top = q + floor(q / 16) in 32-bit words (below 2^254); every coordinate is top - r for an r of 1, of 64 bits or of
    // up to 248 bits, cut into limbs as it stands: a stored value, not reduced
    uint32_t qw[8], top[8];
    Fq::to_words<8>(Fq::from_const(EdConsts::MOD), qw);
    uint64_t carry = 0;
    for (int k = 0; k < 8; k++) {
      const uint64_t sum = (uint64_t)qw[k] + ((qw[k] >> 4) | (k < 7 ? qw[k + 1] << 28 : 0u)) + carry;
      top[k] = (uint32_t)sum;
      carry = sum >> 32;
    }
    if (carry) return 2;
    int count = 0;
    uint64_t seed = 0xB0D;
    for (int i = 0; i < 256; i++) {
      Fq::El v[4];
      for (int k = 0; k < 4; k++) {
        uint32_t r[8] = {1, 0, 0, 0, 0, 0, 0, 0}, w[8];
        const uint64_t z = splitmix(seed);
        if (i & (1 << k)) r[0] = (uint32_t)z | 1u, r[1] = (uint32_t)(z >> 32);
        if (i >= 128) r[7] = (uint32_t)(z >> 40);
        int64_t borrow = 0;
        for (int j = 0; j < 8; j++) {
          const int64_t d = (int64_t)top[j] - r[j] + borrow;
          w[j] = (uint32_t)(d & 0xffffffffll);
          borrow = d >> 32;
        }
        if (borrow) return 2;
        v[k] = Fq::from_words<8>(w);
      }
      EdLazy::Ext p;
      p.x = v[0];
      p.y = v[1];
      p.t = v[2];
      p.z = v[3];
      if (!dbl_ok(p)) {
        fprintf(stderr, "bound: case %d\n", i);
        return 1;
      }
      count++;
    }
    printf("%d\n", count);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "recode")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t s[8];
    int count = 0;
    while (fread(s, 4, 8, f) == 8) {
      if (!digits_ok(s)) {
        fprintf(stderr, "recode: scalar %d\n", count);
        fclose(f);
        return 1;
      }
      count++;
    }
    fclose(f);
    printf("%d\n", count);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    uint32_t head[2];
    bool ok = fread(&n, 8, 1, f) == 1 && fread(head, 4, 2, f) == 2 && n <= (1u << 20);
    std::vector<uint8_t> points(ok ? (size_t)n * 64 : 0);
    ok = ok && fread(points.data(), 64, (size_t)n, f) == n;
    const size_t scalar_bytes = ok ? (head[0] == 0 ? (n ? 32 : 0) : (size_t)n * 32) : 0;
    uint8_t* scalars = ok ? (uint8_t*)malloc(scalar_bytes ? scalar_bytes : 1) : nullptr;  // exact size: no slack behind the last scalar
    ok = ok && scalars && fread(scalars, 1, scalar_bytes, f) == scalar_bytes;
    fclose(f);
    if (!ok) {
      free(scalars);
      return 2;
    }
    std::vector<uint8_t> out((size_t)n * 64 + 1, 0xEE);
    const int32_t rc = ed_batch_mul_var_host(points.data(), scalars, n, head[0], out.data());
    free(scalars);
    if (rc != 0) {
      for (uint8_t b : out)
        if (b != 0xEE) return 3;
    }
    if (out[(size_t)n * 64] != 0xEE) return 3;
    FILE* g = fopen(argv[3], "wb");
    if (!g) return 2;
    fwrite(&rc, 4, 1, g);
    if (rc == 0) fwrite(out.data(), 64, (size_t)n, g);
    fclose(g);
    return 0;
  }
  fprintf(stderr, "usage: ed_lazy_dbl_host dbl <in> | bound | recode <in> | run <in> <out>\n");
  return 2;
}
