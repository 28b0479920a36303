// Stand-alone driver of csrc/commit_rows_host.hpp and csrc/commit_rows_plan.hpp for tests/test_commit_rows_host.py:
// compiled with g++ and the address / undefined-behaviour sanitizers against the headers, no library, no device.
//   commit_rows_host limits            MSM377_GEN_MAX MSM377_GEN_WIDE_MAX
//   commit_rows_host plan <k>          segments, generators per segment, rows per pass of commit_rows_plan(k)
//   commit_rows_host run <in> <out>    in:  u32 scalar_form, u32 out_form, u32 k, u32 generators in the file, u64 n,
//                                           u64 out_stride, u64 base_stride, u64 scalar bytes, then the generators (96
//                                           bytes each) and the scalar bytes (an allocation of exactly that size: a read
//                                           past the layout's last scalar is the sanitizer's to report)
//                                      out: i32 return code, then (code 0) n records and n flag bytes; after any other
//                                           code the program checks that the poisoned outputs are untouched
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "commit_rows_host.hpp"
#include "commit_rows_plan.hpp"

using namespace msm377;

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %d\n", MSM377_GEN_MAX, MSM377_GEN_WIDE_MAX);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "plan")) {
    const CommitRowsPlan p = commit_rows_plan((uint32_t)strtoul(argv[2], nullptr, 10));
    printf("%u %u %llu\n", p.segments, p.bases_per_segment, (unsigned long long)p.rows_per_pass);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "run")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t head[4];
    uint64_t dims[4];  // n, out_stride, base_stride, scalar bytes
    bool ok = fread(head, 4, 4, f) == 4 && fread(dims, 8, 4, f) == 4 && dims[0] <= (1u << 20) && dims[3] <= (1u << 28) && head[3] <= 8192;
    std::vector<uint8_t> gens(ok ? (size_t)head[3] * 96 : 0);  // (k may exceed the generators given: a refusal reads none)
    ok = ok && fread(gens.data(), 96, head[3], f) == head[3];
    uint8_t* scalars = ok ? (uint8_t*)malloc(dims[3] ? dims[3] : 1) : nullptr;  // exact size: no slack behind the last scalar
    ok = ok && scalars && fread(scalars, 1, dims[3], f) == dims[3];
    fclose(f);
    if (!ok) return 2;
    const uint64_t n = dims[0];
    const size_t stride = head[1] == MSM377_POINTS_MONT_FLAG ? 104 : 96;
    std::vector<uint8_t> out((size_t)n * stride + 1, 0xEE), inf((size_t)n + 1, 0xEE);
    const int32_t rc = commit_rows_host(gens.data(), head[2], scalars, head[0], n, dims[1], dims[2], head[1], out.data(), inf.data());
    free(scalars);
    if (rc != 0) {
      for (uint8_t b : out)
        if (b != 0xEE) return 3;
      for (uint8_t b : inf)
        if (b != 0xEE) return 3;
    }
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
  fprintf(stderr, "usage: commit_rows_host limits | plan <k> | run <in> <out>\n");
  return 2;
}
