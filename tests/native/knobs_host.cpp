// Stand-alone driver of csrc/knobs.hpp for tests/test_knobs_host.py: compiled with g++ and the address /
// undefined-behaviour sanitizers against the header, no library, no device.  Prints Knobs::from_env() of the environment
// it is started in, one "field value" line per field.
#include <inttypes.h>
#include <stdio.h>

#include "knobs.hpp"

int main() {
  const msm377::Knobs k = msm377::Knobs::from_env();
#define SHOW(field) printf(#field " %" PRId64 "\n", (int64_t)k.field)
  SHOW(glv_mode);
  SHOW(g1_form);
  SHOW(conv_wave_prio);
  SHOW(aff_prewake_us);
  SHOW(upload_chunks);
  SHOW(upload_split_pct);
  printf("upload_chunk_min %" PRIu64 "\n", k.upload_chunk_min);
  SHOW(tail_threads);
  SHOW(tail_wait_ms);
  SHOW(tail_spin_us);
  SHOW(tail_trace);
  SHOW(tail_numa);
  SHOW(te_affine_msm);
  printf("narrow_max_points %" PRIu64 "\n", k.narrow_max_points);
  SHOW(precomp_bits);
  printf("affine_min_points %" PRIu64 "\n", k.affine_min_points);
  SHOW(seg_plain);
  SHOW(seg_glv);
  SHOW(zc_out);
  SHOW(narrow_seg);
  printf("narrow_quad_items %" PRIu64 "\n", k.narrow_quad_items);
  SHOW(coop_threads);
  SHOW(narrow_tail_from);
  SHOW(tail_lds);
  SHOW(reduce_columns);
  SHOW(even_windows);
  SHOW(sort_elem);
  SHOW(twin_batches);
  SHOW(base_checks);
  SHOW(tail_from);
  return 0;
}
