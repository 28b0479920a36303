// How a bucket row is cut into accumulation work items: shared by the kernels of kernels/accumulate.hpp (device) and the
// host (tests/native/row_split_shim.cpp compiles it with g++ and compares it with the model of tests/stage_model.py).
// Plain integer code, no device intrinsics.
#pragma once
#include <stdint.h>

#ifndef MSM_HD  // as in common.hpp and field29.hpp, for translation units that include this header alone
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSM_HD __host__ __device__ __forceinline__
#else
#define MSM_HD inline __attribute__((always_inline))
#endif
#endif

namespace msm377 {

// A row of `len` entries becomes `nseg` work items of `seglen` entries (the last one `lastlen`): equal parts of at
// most SEG entries, so a row just over a multiple of SEG does not leave one full-length chain beside a stub.
struct RowSplit {
  uint32_t nseg, seglen, lastlen;
};
MSM_HD RowSplit row_split(uint32_t len, uint32_t SEG) {
  RowSplit r;
  if (len <= SEG) {
    r.nseg = 1;
    r.seglen = r.lastlen = len;
    return r;
  }
  const uint32_t parts = (len + SEG - 1) / SEG;
  r.seglen = (len + parts - 1) / parts;
  r.nseg = (len + r.seglen - 1) / r.seglen;  // <= parts
  r.lastlen = len - (r.nseg - 1) * r.seglen;  // 1..seglen
  return r;
}

}  // namespace msm377
