// Stand-alone driver of the host twin csrc/ed_batch_lincomb_host.hpp for tests/test_ed_batch_lincomb_host.py: compiled with
// g++ (and, once more, with the address / undefined-behaviour sanitizers) against the headers, no library, no device.
//   ed_batch_lincomb_host run <in> <out>
//     in:  u64 n, u32 k, u32 place, then k x (u32 point_stride, u32 scalar_stride), then per term its points and its
//          scalars -- n elements each, or ONE for stride 0; every array in an allocation of exactly its size, so that a read
//          behind the one element of a stride-0 array is a finding
//          place: 0 the outputs in a buffer of their own, poisoned with 0xEE
//                 1 + t the outputs over the points of term t (its point_stride must be 64)
//                 100 the fold in place: the points of terms 0 and 1 are ONE buffer of 2n records, term 1 = term 0 + n
//                     records, the outputs over term 0
//     out: i32 return code, then (code 0) n records; after any other code the program checks that the poisoned output is
//          untouched (place 0)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ed_batch_lincomb_host.hpp"

using namespace msm377;

static uint8_t* exact(FILE* f, size_t bytes, bool& ok) {
  uint8_t* buf = (uint8_t*)malloc(bytes ? bytes : 1);
  ok = ok && buf && fread(buf, 1, bytes, f) == bytes;
  return buf;
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: ed_batch_lincomb_host run <in> <out>\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 2;
  uint64_t n = 0;
  uint32_t head[2] = {}, strides[2 * MSM377_LINCOMB_MAX_TERMS] = {};
  bool ok = fread(&n, 8, 1, f) == 1 && fread(head, 4, 2, f) == 2 && n <= (1u << 20);
  const uint32_t k = head[0], place = head[1];
  ok = ok && k <= MSM377_LINCOMB_MAX_TERMS && fread(strides, 4, 2 * (size_t)k, f) == 2 * (size_t)k;  // (k = 0: the call refuses it)
  const bool fold = place == 100;
  ok = ok && (place <= k || fold) && (!fold || (k >= 2 && strides[0] == 64 && strides[2] == 64)) && (place == 0 || fold || strides[2 * (place - 1)] == 64);
  const auto bytes = [&](uint32_t stride, size_t size) { return !ok || !n ? (size_t)0 : stride ? (size_t)n * size : size; };
  msm377_lincomb_term terms[MSM377_LINCOMB_MAX_TERMS] = {};
  uint8_t *points[MSM377_LINCOMB_MAX_TERMS] = {}, *scalars[MSM377_LINCOMB_MAX_TERMS] = {};
  for (uint32_t t = 0; ok && t < k; t++) {
    if (fold && t == 1) {
      points[1] = points[0] + (size_t)n * 64;  // (read with term 0, below)
      ok = fread(points[1], 1, (size_t)n * 64, f) == (size_t)n * 64;
    } else if (fold && t == 0) {
      points[0] = (uint8_t*)malloc(n ? (size_t)n * 128 : 1);
      ok = points[0] && fread(points[0], 1, (size_t)n * 64, f) == (size_t)n * 64;
    } else {
      points[t] = exact(f, bytes(strides[2 * t], 64), ok);
    }
    scalars[t] = exact(f, bytes(strides[2 * t + 1], 32), ok);
    terms[t] = msm377_lincomb_term{points[t], scalars[t], strides[2 * t], strides[2 * t + 1]};
  }
  fclose(f);
  int status = 2;
  if (ok) {
    std::vector<uint8_t> own((size_t)n * 64 + 1, 0xEE);
    uint8_t* out = place == 0 ? own.data() : fold ? points[0] : points[place - 1];
    const int32_t rc = ed_batch_lincomb_host(terms, k, n, out);
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
  for (uint32_t t = 0; t < k && t < MSM377_LINCOMB_MAX_TERMS; t++) {
    if (!(fold && t == 1)) free(points[t]);
    free(scalars[t]);
  }
  return status;
}
