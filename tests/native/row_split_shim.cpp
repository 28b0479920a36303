// csrc/row_split.hpp -- the function every accumulation kernel cuts its rows with -- compiled for the host with g++, behind
// one C function for tests/test_stage_model_host.py.  TEST INFRASTRUCTURE.
#include "row_split.hpp"

extern "C" {

// out[3 i .. 3 i + 3) = nseg, seglen, lastlen of a row of len_first + i entries, i < count.
void row_split_table(uint32_t seg, uint32_t len_first, uint32_t count, uint32_t* out) {
  for (uint32_t i = 0; i < count; i++) {
    const msm377::RowSplit r = msm377::row_split(len_first + i, seg);
    out[3 * i] = r.nseg, out[3 * i + 1] = r.seglen, out[3 * i + 2] = r.lastlen;
  }
}

}
