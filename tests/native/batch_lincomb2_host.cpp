// Stand-alone driver of csrc/batch_lincomb2_host.hpp for tests/test_batch_lincomb2_host.py: compiled with g++ and the
// address / undefined-behaviour sanitizers against the headers, no library, no device.
//   batch_lincomb2_host run <in> <out>   in:  u32 point_form, u32 scalar_form, u32 out_form, u32 a_stride, u32 b_stride,
//                                             u32 0, u64 n, n records of p, n records of q, then n (stride 32) or one
//                                             (stride 0) 32-byte scalars a, the same for b
//                                        out: i32 return code, then (code 0) n records and n flag bytes
// Every buffer is exactly as long as the call may read or write: the sanitizer sees a byte too many.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "batch_lincomb2_host.hpp"

using namespace msm377;

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t head[6];
    uint64_t n = 0;
    bool ok = fread(head, 4, 6, f) == 6 && fread(&n, 8, 1, f) == 1 && n <= (1u << 20);
    const size_t in_stride = head[0] == MSM377_POINTS_MONT_FLAG ? 104 : 96;
    const size_t na = head[3] == 0 && n ? 1 : (size_t)n, nb = head[4] == 0 && n ? 1 : (size_t)n;
    std::vector<uint8_t> p(ok ? (size_t)n * in_stride : 0), q(p.size()), a(ok ? na * 32 : 0), b(ok ? nb * 32 : 0);
    ok = ok && fread(p.data(), in_stride, (size_t)n, f) == (size_t)n && fread(q.data(), in_stride, (size_t)n, f) == (size_t)n && fread(a.data(), 32, na, f) == na &&
         fread(b.data(), 32, nb, f) == nb;
    fclose(f);
    if (!ok) return 2;
    const size_t stride = head[2] == MSM377_POINTS_MONT_FLAG ? 104 : 96;
    std::vector<uint8_t> out((size_t)n * stride, 0xEE), inf((size_t)n, 0xEE);
    const int32_t rc = batch_lincomb2_host(p.data(), q.data(), head[0], a.data(), b.data(), head[1], n, head[3], head[4], head[2], out.data(), inf.data());
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
  fprintf(stderr, "usage: batch_lincomb2_host run <in> <out>\n");
  return 2;
}
