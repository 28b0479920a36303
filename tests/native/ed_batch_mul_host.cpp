// Stand-alone driver of csrc/ed_batch_mul_host.hpp, csrc/fq_inverse.hpp and csrc/batch_mul_recode.hpp for
// tests/test_ed_batch_mul_host.py: compiled with g++ and the address / undefined-behaviour sanitizers against the headers,
// no library, no device.
//   ed_batch_mul_host limits            MSM377_MUL_MAX_BASES
//   ed_batch_mul_host recode <in>       in: 32-byte scalars; for the widths 8 and 16 (and every width bm_digit accepts)
//                                       s == sum_w digit_w 2^(c w) + carry 2^(c W), |digit_w| <= 2^(c-1), carry in {0, 1}
//   ed_batch_mul_host inverse           FqInverse::inverse_mont (the device's 9-limb walk, compiled for the host) against
//                                       Fq64::inv: 1, q - 1, 2, values with long zero runs, seeded values
//   ed_batch_mul_host run <in> <out>    in:  u32 k, u32 zero, u64 n, u64 out_stride, u64 base_stride, u64 scalar bytes, then
//                                            k x 64 base bytes and the scalar bytes (an allocation of exactly that size)
//                                       out: i32 return code, then (code 0) n records; after any other code the program
//                                            checks that the poisoned output is untouched
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_mul_recode.hpp"
#include "ed_batch_mul_host.hpp"
#include "fq_inverse.hpp"

using namespace msm377;

static bool recode_ok(const uint32_t s[8], int c) {
  const int W = bm_windows(c);
  int64_t acc[11] = {};  // 32-bit word positions; a position takes a few terms below 2^48
  uint32_t carry = 0;
  for (int w = 0; w <= W; w++) {
    const int32_t d = w < W ? bm_digit(s, c, w, carry) : (int32_t)carry;
    if (w < W && (d > (1 << (c - 1)) || d < -(1 << (c - 1)) + 1)) return false;
    if (carry > 1) return false;
    const int bit = c * w;
    acc[bit >> 5] += (int64_t)d * ((int64_t)1 << (bit & 31));
  }
  int64_t run = 0;
  for (int i = 0; i < 11; i++) {
    const int64_t v = acc[i] + run;
    const uint32_t word = (uint32_t)(v & 0xffffffffll);
    run = v >> 32;
    if (word != (i < 8 ? s[i] : 0u)) return false;
  }
  return run == 0;
}

static uint64_t splitmix(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a: canonical residue as 8 little-endian u32 words
static bool inverse_ok(const uint32_t a[8]) {
  const Fq::El m = Fq::to_mont(Fq::from_words<8>(a));
  const Fq::El inv = FqInverse::inverse_mont(m);
  for (int j = 0; j < 9; j++)
    if (inv.l[j] > LMASK) return false;
  const Fq64::El want = Fq64::inv(Fq64::from_limbs29_mont(m.l));
  if (!Fq64::eq(Fq64::from_limbs29_mont(inv.l), want)) return false;
  return Fq::eq(Fq::mul(inv, m), Fq::one());  // and canonical: the product is the canonical form of 1
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d\n", MSM377_MUL_MAX_BASES);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "recode")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t s[8];
    int count = 0;
    while (fread(s, 4, 8, f) == 8) {
      for (int c = BM_MIN_WIDTH; c <= BM_MAX_WIDTH; c++)
        if (!recode_ok(s, c)) {
          fprintf(stderr, "recode: scalar %d, width %d\n", count, c);
          fclose(f);
          return 1;
        }
      count++;
    }
    fclose(f);
    printf("%d\n", count);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "inverse")) {
    uint32_t q[8];
    Fq::to_words<8>(Fq::from_const(EdConsts::MOD), q);
    std::vector<std::vector<uint32_t>> values;
    values.push_back({1, 0, 0, 0, 0, 0, 0, 0});
    values.push_back({2, 0, 0, 0, 0, 0, 0, 0});
    values.push_back({q[0] - 1, q[1], q[2], q[3], q[4], q[5], q[6], q[7]});  // q - 1 (q is odd)
    for (int b = 1; b < 252; b += 7) {  // long zero runs: 2^b, 2^b + 1, 2^251 + 2^b
      std::vector<uint32_t> v(8, 0), u(8, 0), t(8, 0);
      v[b >> 5] = 1u << (b & 31);
      u = v;
      u[0] |= 1;
      t = v;
      t[7] |= 1u << 27;
      values.push_back(v);
      values.push_back(u);
      values.push_back(t);
    }
    uint64_t x = 0xED1417;
    for (int i = 0; i < 200; i++) {
      std::vector<uint32_t> v(8);
      for (int k = 0; k < 4; k++) {
        const uint64_t z = splitmix(x);
        v[2 * k] = (uint32_t)z;
        v[2 * k + 1] = (uint32_t)(z >> 32);
      }
      v[7] &= 0x0fffffffu;  // below 2^252 < q
      if (i % 4 == 1) v[1] = v[2] = v[3] = v[4] = 0;
      if (i % 4 == 2) v[3] = v[4] = v[5] = v[6] = v[7] = 0;
      values.push_back(v);
    }
    int count = 0;
    for (const auto& v : values) {
      bool zero = true;
      for (uint32_t w : v) zero = zero && w == 0;
      if (zero) continue;
      if (!inverse_ok(v.data())) {
        fprintf(stderr, "inverse: value %d\n", count);
        return 1;
      }
      count++;
    }
    printf("%d\n", count);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t head[2];
    uint64_t dims[4];  // n, out_stride, base_stride, scalar bytes
    bool ok = fread(head, 4, 2, f) == 2 && fread(dims, 8, 4, f) == 4 && dims[0] <= (1u << 20) && dims[3] <= (1u << 28) && head[0] <= 64;
    std::vector<uint8_t> bases(ok ? (size_t)head[0] * 64 : 0);
    ok = ok && fread(bases.data(), 64, head[0], f) == head[0];
    uint8_t* scalars = ok ? (uint8_t*)malloc(dims[3] ? dims[3] : 1) : nullptr;  // exact size: no slack behind the last scalar
    ok = ok && scalars && fread(scalars, 1, dims[3], f) == dims[3];
    fclose(f);
    if (!ok) {
      free(scalars);
      return 2;
    }
    const uint64_t n = dims[0];
    std::vector<uint8_t> out((size_t)n * 64 + 1, 0xEE);
    const int32_t rc = ed_batch_mul_multi_host(bases.data(), head[0], scalars, n, dims[1], dims[2], out.data());
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
  fprintf(stderr, "usage: ed_batch_mul_host limits | recode <in> | inverse | run <in> <out>\n");
  return 2;
}
