// Stand-alone driver of the host twin csrc/ed_batch_lincomb2_host.hpp for tests/test_ed_batch_lincomb2_host.py: compiled
// with g++ (and, once more, with the address / undefined-behaviour sanitizers) against the headers, no library, no device.
//   ed_batch_lincomb2_host run <in> <out>
//     in:  u64 n, u32 p_stride, q_stride, a_stride, b_stride, u32 place, u32 zero, then the bytes of p, q, a and b -- n
//          elements each, or ONE for stride 0; every array in an allocation of exactly its size, so that a read behind the
//          one element of a stride-0 array is a finding
//          place: 0 the outputs in a buffer of their own, poisoned with 0xEE
//                 1 the outputs over p, 2 over q (that array's stride must be 64)
//                 3 the fold in place: p and q are ONE buffer of 2n records, q = p + n records, the outputs over p
//     out: i32 return code, then (code 0) n records; after any other code the program checks that the poisoned output is
//          untouched (place 0)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ed_batch_lincomb2_host.hpp"

using namespace msm377;

static uint8_t* exact(FILE* f, size_t bytes, bool& ok) {
  uint8_t* buf = (uint8_t*)malloc(bytes ? bytes : 1);
  ok = ok && buf && fread(buf, 1, bytes, f) == bytes;
  return buf;
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: ed_batch_lincomb2_host run <in> <out>\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 2;
  uint64_t n = 0;
  uint32_t head[6];
  bool ok = fread(&n, 8, 1, f) == 1 && fread(head, 4, 6, f) == 6 && n <= (1u << 20);
  const uint32_t p_stride = head[0], q_stride = head[1], a_stride = head[2], b_stride = head[3], place = head[4];
  const auto bytes = [&](uint32_t stride, size_t size) { return !ok || !n ? (size_t)0 : stride ? (size_t)n * size : size; };
  uint8_t *p = nullptr, *q = nullptr;
  if (place == 3) {
    ok = ok && p_stride == 64 && q_stride == 64;
    p = exact(f, ok ? (size_t)n * 128 : 0, ok);
    q = p + (size_t)n * 64;
  } else {
    p = exact(f, bytes(p_stride, 64), ok);
    q = exact(f, bytes(q_stride, 64), ok);
  }
  uint8_t* a = exact(f, bytes(a_stride, 32), ok);
  uint8_t* b = exact(f, bytes(b_stride, 32), ok);
  fclose(f);
  ok = ok && place <= 3 && (place != 1 || p_stride == 64) && (place != 2 || q_stride == 64);
  int status = 2;
  if (ok) {
    std::vector<uint8_t> own((size_t)n * 64 + 1, 0xEE);
    uint8_t* out = place == 0 ? own.data() : place == 2 ? q : p;
    const int32_t rc = ed_batch_lincomb2_host(p, q, a, b, n, p_stride, q_stride, a_stride, b_stride, out);
    status = 0;
    if (rc != 0 && place == 0)
      for (uint8_t v : own)
        if (v != 0xEE) status = 3;
    if (own[(size_t)n * 64] != 0xEE) status = 3;
    FILE* g = status ? nullptr : fopen(argv[3], "wb");
    if (!status && !g) status = 2;
    if (g) {
      fwrite(&rc, 4, 1, g);
      if (rc == 0) fwrite(out, 64, (size_t)n, g);
      fclose(g);
    }
  }
  free(p);
  if (place != 3) free(q);
  free(a);
  free(b);
  return status;
}
