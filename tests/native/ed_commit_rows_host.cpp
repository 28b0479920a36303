// Stand-alone driver of csrc/ed_commit_rows_host.hpp for tests/test_ed_commit_rows_host.py: compiled with g++ and the
// address / undefined-behaviour sanitizers against the headers, no library, no device.
//   ed_commit_rows_host limits            MSM377_GEN_MAX MSM377_GEN_WIDE_MAX
//   ed_commit_rows_host run <in> <out>    in:  u32 k, u32 generators in the file, u64 n, u64 out_stride, u64 base_stride,
//                                              u64 scalar bytes, then the generators (64 bytes each) and the scalar bytes
//                                              (an allocation of exactly that size: a read past the layout's last scalar
//                                              is the sanitizer's to report)
//                                         out: i32 return code, then (code 0) n records; after any other code the program
//                                              checks that the poisoned output is untouched
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ed_commit_rows_host.hpp"

using namespace msm377;

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %d\n", MSM377_GEN_MAX, MSM377_GEN_WIDE_MAX);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t head[2];
    uint64_t dims[4];  // n, out_stride, base_stride, scalar bytes
    bool ok = fread(head, 4, 2, f) == 2 && fread(dims, 8, 4, f) == 4 && dims[0] <= (1u << 20) && dims[3] <= (1u << 28) && head[1] <= 8192;
    uint8_t* gens = ok ? (uint8_t*)malloc(head[1] ? (size_t)head[1] * 64 : 1) : nullptr;  // exact sizes: no slack behind the last generator or scalar
    ok = ok && gens && fread(gens, 64, head[1], f) == head[1];
    uint8_t* scalars = ok ? (uint8_t*)malloc(dims[3] ? dims[3] : 1) : nullptr;
    ok = ok && scalars && fread(scalars, 1, dims[3], f) == dims[3];
    fclose(f);
    if (!ok) return 2;
    const uint64_t n = dims[0];
    std::vector<uint8_t> out((size_t)n * 64 + 1, 0xEE);
    const int32_t rc = ed_commit_rows_host(gens, head[0], scalars, n, dims[1], dims[2], out.data());
    free(scalars);
    free(gens);
    if (rc != 0) {
      for (uint8_t b : out)
        if (b != 0xEE) return 3;
    } else if (out[(size_t)n * 64] != 0xEE) {
      return 3;
    }
    FILE* g = fopen(argv[3], "wb");
    if (!g) return 2;
    fwrite(&rc, 4, 1, g);
    if (rc == 0) fwrite(out.data(), 64, (size_t)n, g);
    fclose(g);
    return 0;
  }
  fprintf(stderr, "usage: ed_commit_rows_host limits | run <in> <out>\n");
  return 2;
}
