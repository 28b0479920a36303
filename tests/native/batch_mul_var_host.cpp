// Stand-alone driver of csrc/batch_mul_var_recode.hpp and csrc/batch_mul_var_host.hpp for tests/test_batch_mul_var_host.py:
// compiled with g++ and the address / undefined-behaviour sanitizers against the headers, no library, no device.
//   batch_mul_var_host pack <hex scalar> ...   one line per scalar: the 64 digits as bmv_pack / bmv_next hand them out
//                                              (window 63 first), the carry, then "|", bm_digit's 64 digits of width 4
//                                              (window 0 first) and its final carry
//   batch_mul_var_host run <in> <out>          in:  u32 point_form, u32 scalar_form, u32 out_form, u32 scalar_stride, u64 n,
//                                                   n point records, then n (stride 32) or one (stride 0) 32-byte scalars
//                                              out: i32 return code, then (code 0) n records and n flag bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_mul_var_host.hpp"
#include "batch_mul_var_recode.hpp"

using namespace msm377;

// hex (either case, no prefix, at most 64 digits) -> eight little-endian u32 words; false: anything else
static bool parse_hex(const char* hex, uint32_t* w) {
  memset(w, 0, 32);
  const size_t len = strlen(hex);
  if (len == 0 || len > 64) return false;
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
  if (argc >= 2 && !strcmp(argv[1], "pack")) {
    for (int a = 2; a < argc; a++) {
      uint32_t s[8], packed[8];
      if (!parse_hex(argv[a], s)) return 2;
      memcpy(packed, s, 32);
      const uint32_t carry = bmv_pack(packed);
      for (int w = 0; w < BMV_WINDOWS; w++) printf("%d ", (int)bmv_next(packed));
      printf("%u | ", carry);
      uint32_t c = 0;
      for (int w = 0; w < BMV_WINDOWS; w++) printf("%d ", (int)bm_digit(s, BMV_WIDTH, w, c));
      printf("%u\n", c);
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t head[4];
    uint64_t n = 0;
    bool ok = fread(head, 4, 4, f) == 4 && fread(&n, 8, 1, f) == 1 && n <= (1u << 20);
    const size_t in_stride = head[0] == MSM377_POINTS_MONT_FLAG ? 104 : 96, ns = head[3] == 0 && n ? 1 : (size_t)n;
    std::vector<uint8_t> points(ok ? (size_t)n * in_stride + 1 : 1), scalars(ok ? ns * 32 + 1 : 1);
    ok = ok && fread(points.data(), in_stride, (size_t)n, f) == (size_t)n && fread(scalars.data(), 32, ns, f) == ns;
    fclose(f);
    if (!ok) return 2;
    const size_t stride = head[2] == MSM377_POINTS_MONT_FLAG ? 104 : 96;
    std::vector<uint8_t> out((size_t)n * stride + 1, 0xEE), inf((size_t)n + 1, 0xEE);
    const int32_t rc = batch_mul_var_host(points.data(), head[0], scalars.data(), head[1], n, head[3], head[2], out.data(), inf.data());
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
  fprintf(stderr, "usage: batch_mul_var_host pack <hex>... | run <in> <out>\n");
  return 2;
}
