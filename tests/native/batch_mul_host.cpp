// Stand-alone driver of csrc/batch_mul_recode.hpp and csrc/batch_mul_host.hpp for tests/test_batch_mul_host.py: compiled
// with g++ and the address / undefined-behaviour sanitizers against the headers, no library, no device.
//   batch_mul_host recode <c> <hex scalar> ...   one line per scalar: the W = ceil(256 / c) digits, then the final carry
//   batch_mul_host widths                        the host twin's width, then the device call's widths and its rule's threshold
//   batch_mul_host inverse <hex residue> ...      csrc/fp_inverse.hpp (the device's chunk inversion) on the CPU: one line per
//                                                value a < p, the canonical a^-1 as hex (through the Montgomery form and back)
//   batch_mul_host run <in> <out>                in:  u32 scalar_form, u32 out_form, u64 n, 96 base bytes, n x 32 scalar bytes
//                                                out: i32 return code, then (code 0) n records and n flag bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_mul_host.hpp"
#include "fp_inverse.hpp"

using namespace msm377;

// hex (either case, no prefix, at most 8 * words digits) -> little-endian u32 words; false: anything else
static bool parse_hex(const char* hex, uint32_t* w, size_t words) {
  memset(w, 0, 4 * words);
  const size_t len = strlen(hex);
  if (len == 0 || len > 8 * words) return false;
  for (size_t k = 0; k < len; k++) {
    const char ch = hex[len - 1 - k];
    uint32_t v;
    if (ch >= '0' && ch <= '9') v = (uint32_t)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') v = (uint32_t)(ch - 'a' + 10);
    else if (ch >= 'A' && ch <= 'F') v = (uint32_t)(ch - 'A' + 10);
    else return false;
    w[k / 8] |= v << (4 * (k % 8));
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "widths")) {
    printf("%d %d %d %llu\n", BM_HOST_WIDTH, BM_NARROW_WIDTH, BM_WIDE_WIDTH, (unsigned long long)BM_WIDE_MIN_OUTPUTS);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "recode")) {
    const int c = atoi(argv[2]);
    if (c < BM_MIN_WIDTH || c > BM_MAX_WIDTH) return 2;
    for (int a = 3; a < argc; a++) {
      uint32_t s[8];
      if (!parse_hex(argv[a], s, 8)) return 2;
      uint32_t carry = 0;
      for (int w = 0; w < bm_windows(c); w++) printf("%d ", (int)bm_digit(s, c, w, carry));
      printf("%u\n", carry);
    }
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "inverse")) {
    for (int a = 2; a < argc; a++) {
      uint32_t w[12];
      if (!parse_hex(argv[a], w, 12)) return 2;
      const Fp::El inv = Fp::from_mont(FpInverse::inverse_mont(Fp::to_mont(Fp::from_words<12>(w))));
      Fp::to_words<12>(inv, w);
      for (int j = 11; j >= 0; j--) printf("%08x", w[j]);
      printf("\n");
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t head[2];
    uint64_t n = 0;
    uint8_t base[96];
    bool ok = fread(head, 4, 2, f) == 2 && fread(&n, 8, 1, f) == 1 && fread(base, 1, 96, f) == 96 && n <= (1u << 20);
    std::vector<uint8_t> scalars(ok ? (size_t)n * 32 + 1 : 1);
    ok = ok && fread(scalars.data(), 32, (size_t)n, f) == (size_t)n;
    fclose(f);
    if (!ok) return 2;
    const size_t stride = head[1] == MSM377_POINTS_MONT_FLAG ? 104 : 96;
    std::vector<uint8_t> out((size_t)n * stride + 1, 0xEE), inf((size_t)n + 1, 0xEE);
    const int32_t rc = batch_mul_host(base, scalars.data(), n, head[0], head[1], out.data(), inf.data());
    FILE* g = fopen(argv[3], "wb");
    if (!g) return 2;
    fwrite(&rc, 4, 1, g);
    if (rc == 0) {
      fwrite(out.data(), stride, (size_t)n, g);
      fwrite(inf.data(), 1, (size_t)n, g);
    }
    fclose(g);
    return 0;
  }
  fprintf(stderr, "usage: batch_mul_host recode <c> <hex>... | widths | inverse <hex>... | run <in> <out>\n");
  return 2;
}
