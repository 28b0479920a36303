// How a row-commitment call (msm377_g1_commit_rows*, kernels/commit_rows.hpp) over k generators is cut: the ONE definition
// the host code, the device launch and msm377_commit_rows_plan read.
//   segments S          = ceil(k / 16): a row's walk is split across S threads, each over at most 16 tables -- the depth
//                         k_bmm_accumulate runs at
//   bases per segment   = ceil(k / S): the segments are even to within one base and none is empty (k > 16 (S - 1), so the
//                         S bases_per_segment - k bases the last segment is short of are fewer than bases_per_segment)
//   rows per pass       = floor(2^20 / S) rounded down to a multiple of the workgroup size: the S partial sums of every row
//                         of a pass lie side by side in the 2^20-point stash of the batch calls (4 096 rows at k = 4 096,
//                         2^20 at k <= 16)
// Plain C++: compiles with g++ and hipcc alike.
#pragma once
#include <stdint.h>

#include "../../include/msm377.h"

namespace msm377 {

constexpr uint32_t CR_SEGMENT_BASES = 16;    // MSM377_MUL_MAX_BASES: the longest walk of one thread
constexpr uint64_t CR_PASS_POINTS = 1ull << 20;  // BM_CHUNK: the points one stash holds
constexpr uint32_t CR_ROW_BLOCK = 256;       // BM_THREADS (kernels/commit_rows.hpp asserts both)

struct CommitRowsPlan {
  uint32_t segments = 0, bases_per_segment = 0;
  uint64_t rows_per_pass = 0;
};

// k outside 1 .. MSM377_GEN_MAX: 0 segments.
inline CommitRowsPlan commit_rows_plan(uint32_t k) {
  CommitRowsPlan p;
  if (k < 1 || k > MSM377_GEN_MAX) return p;
  p.segments = (k + CR_SEGMENT_BASES - 1) / CR_SEGMENT_BASES;
  p.bases_per_segment = (k + p.segments - 1) / p.segments;
  p.rows_per_pass = CR_PASS_POINTS / p.segments / CR_ROW_BLOCK * CR_ROW_BLOCK;
  return p;
}

}  // namespace msm377
