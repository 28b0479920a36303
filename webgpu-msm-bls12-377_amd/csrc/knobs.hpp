// Every tunable of a context that the environment (MSM377_*) or a setter of include/msm377.h writes, as one value: a
// context is created with one (msm377_ctx_create: Knobs::from_env()), its twin runs with a copy of its owner's.  Modes
// of use (timing, stage capture, input forms, the forced batch_mul window) are not tunables and live in msm377_ctx.
// Host-only, no HIP header: tests/native/knobs_host.cpp compiles it with g++.
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.hpp"
#include "tail_pool.hpp"
#include "validate_host.hpp"

namespace msm377 {

struct Knobs {
  // GLV front end of the Weierstrass path: 0 = off (default), 1 = on.  phi(P) = [lambda] P holds only for points of
  // the prime-order subgroup, so it is an opt-in: the caller vouches for the inputs (every protocol use does).
  // Interleaved A/B on one MI355X (tools/ab_knobs.py), Weierstrass plain vs GLV ms per MSM: 2^18 1.39 / 1.24,
  // 2^19 2.08 / 2.00, 2^20 3.56 / 3.51, 2^22 12.56 / 12.39 (halved bucket reduction and host tail).
  int glv_mode = 0;        // MSM377_GLV, msm377_ctx_set_glv
  int g1_form = 1;         // G1 full-MSM entry points: 1 = twisted Edwards form (te377.hpp, default), 0 = Weierstrass XYZZ (MSM377_G1_FORM)
  // MSM377_CONV_WAVE_PRIO: the conversion kernels (k_affine_up / k_affine_down) raise their waves' issue priority
  // (s_setprio 3) over the front-end kernels that run beside them on the main stream.
  uint32_t conv_wave_prio = 1;
  // MSM377_AFF_PREWAKE_US: the helper threads that invert the conversion's block products are woken when the way up is
  // queued and poll for their share (at most this long) instead of being woken from their condition variable when the
  // products arrive -- the wake-up (20-60 us) sat in the middle of the front end's critical path.  0 = off.
  int64_t aff_prewake_us = 600;
  uint32_t upload_chunks = 4;              // chunks of the host-buffer upload (MSM377_UPLOAD_CHUNKS, 2..7): 2: 5.07, 3: 4.89, 4-6: 4.70, 8: 4.95 ms at 2^20 (round 2)
  uint32_t upload_split_pct = 30;          // share of the points in the first chunk (MSM377_UPLOAD_SPLIT, 5..90)
  uint64_t upload_chunk_min = 1ull << 18;  // msm377_g1_msm: inputs of at least this many points upload and run as two chunks (MSM377_UPLOAD_CHUNK_MIN)
  int tail_threads = 6;               // MSM377_TAIL_THREADS: threads of the host tail (1..8, tail_horner_mt)
  int tail_wait_ms = 2000;            // MSM377_TAIL_WAIT_MS (>= 1): how long a call waits for a helper thread's answer (TailPool::wait_limit_ns)
  // MSM377_TAIL_SPIN_US: how long at most the tail workers poll for their job after a call has armed them (TailPool;
  // 0 = they sleep until the job is posted).  Tail stage at 2^20, interleaved (tools/ab_knobs.py): one thread 0.140 ms,
  // six sleeping workers 0.124, six polling ones 0.089.  (Round 2 first measured no difference: the per-thread
  // exceptional-case flags shared a cache line then and the threads fought over it -- TeChecked is padded now.)
  int64_t tail_spin_us = 1000;
  bool tail_trace = false;  // MSM377_TAIL_TRACE=1
  bool tail_numa = true;    // MSM377_TAIL_NUMA=0: leave the tail workers where the scheduler puts them (TailPool::numa_local)
  bool te_affine_msm = true;          // MSM377_TE_AFFINE_MSM=0: msm377_g1_msm_device keeps projective records (A/B knob)
  // Inputs of at most this many points run the narrow-window path (22 windows of 2048 buckets instead of
  // 16 x 32768; MSM377_NARROW_MAX, msm377_ctx_set_narrow_max, 0 = never).  Interleaved A/B, 16-bit / narrow ms per MSM (tools/ab_knobs.py):
  // 2^10 0.64 / 0.46, 2^13 0.67 / 0.53, 2^14 0.68 / 0.51, 2^15 0.73 / 0.60, 2^16 0.74 / 0.71 (first version, 23 windows); at the end of
  // round 2: 2^16 0.605 / 0.56 (its bucket reduction 0.28 / 0.10 ms, its accumulation kernel 0.14 / 0.18), hence 2^16.
  uint64_t narrow_max_points = 1ull << 16;
  int precomp_bits = MSM377_WINDOW_BITS;  // window width msm377_g1_set_bases_precomputed builds its next table for: 16 or 20 (msm377_ctx_set_precompute_window, MSM377_PRECOMP_BITS)
  // Below this the batched conversion does not pay: it costs ~9 more products per point than the projective record and
  // saves 16, but its two kernels and the host round trip sit in front of the accumulation, which they cannot hide
  // under the (short) sort of a small input.  Interleaved A/B, projective / affine ms per MSM (tools/ab_knobs.py):
  // 2^15 0.69 / 0.88, 2^16 0.75 / 0.89, 2^17 0.88 / 0.97, 2^18 1.19 / 1.26, 2^19 1.76 / 1.78, 2^20 2.89 / 2.79.  MSM377_AFFINE_MIN.
  uint64_t affine_min_points = 1ull << 20;
  uint32_t seg_plain = 0, seg_glv = 0;  // MSM377_SEG_PLAIN / MSM377_SEG_GLV: force the work-item length (SEG_MIN..SEG_MAX), 0 = auto_seg()
  int zc_out = 1;  // zero-copy output of the full-MSM path (k_gather_partials, wait_zero_copy_out); MSM377_ZERO_COPY_OUT=0: D2H copies + event
  uint32_t narrow_seg = 0;  // MSM377_NARROW_SEG (>= NARROW_SEG: the buffers are sized for that); 0 = by input size (launch_record)
  uint64_t narrow_quad_items = 100000;  // MSM377_NARROW_QUAD_ITEMS: most work items k_accumulate_quad is used for (0: a thread per work item, like the main path)
  // First reduction level run with one addition per lane quad: the first level whose 4 lanes x additions x windows fit
  // coop_threads -- level 7 for 16 windows (measured: 18-24 -> 13-18 us per level from there on, slower before), 6 for 8, 4
  // for the 2 windows a rank of an 8-GPU window-sharded run owns.
  // MSM377_COOP_THREADS: a tree level runs one lane quad per addition once that takes at most this many threads.  65536 / 131072 /
  // 262144 make no difference on the main path (2^20: 2.74 ms each); on the narrow path 131072 moves its levels 0-2 to quads.
  uint32_t coop_threads = 131072;
  // MSM377_NARROW_TAIL_FROM: tail_from of the narrow-window path (2048 buckets per window).  Reduce stage at 2^12 with
  // 7 / 5 / 4 / 3 / 2: 0.106 / 0.099 / 0.096 / 0.101 / 0.122 ms (profiles/r02_final/ab_narrow_tree.txt).
  uint32_t narrow_tail_from = 4;
  bool tail_lds = true;         // MSM377_TAIL_LDS=0: the single-launch reduction tail works in global memory (k_reduce_tail)
  // MSM377_REDUCE_COLUMNS=0: the levels below tail_from run one launch per level (k_tree_step / k_tree_step_quad) instead of
  // as column launches of up to four levels each (k_tree_columns); same records either way, kept for A/B runs and the tests.
  bool reduce_columns = true;
  bool even_windows = true;     // MSM377_EVEN_WINDOWS=0: sixteen 16-bit windows on the 16-window paths (kernels/decompose.hpp k_decompose); the narrow path keeps its geometry
  // MSM377_SORT_ELEM: bytes per sort_temp element of the main path's sort.  8 (default): SortElem.  4: the packed SortElem4
  // wherever the call allows it (common.hpp sort_elem_bytes), for A/B runs and the tests, which run both forms.  Interleaved
  // A/B at 2^20, 15 pairs (profiles/sort_elem4/ab_sort_elem.txt): sort stage 0.264 -> 0.249 ms, k_accumulate starts 12-17 us
  // sooner, whole MSM 2.477 -> 2.469 ms (medians) with run-to-run spreads of 0.06 and 0.09: inside the noise, so 8 stays the default.
  uint32_t sort_elem = 8;
  bool twin_batches = true;     // MSM377_TWIN_BATCH=0: batches run on this context alone (sequencer.hip twin_prepare; always false in a twin)
  // MSM377_BASE_CHECKS / msm377_ctx_set_base_checks: MSM377_CHECK_* flags (normalised) the set-bases calls check a base set
  // with before they convert it; 0 = none.
  uint32_t base_checks = 0;
  // First level of the single-launch tail of the reduction (k_reduce_tail); MSM377_TAIL_FROM, 15 = one launch per level throughout.
  uint32_t tail_from = 7;  // measured (tools/ab_knobs.py, 2^20): 15: 2.874 ms, 7: 2.842, 6: 2.885, 5: 2.916, 4: 3.062

  static inline Knobs from_env();
};

// The rules of the table below: how the text of a variable becomes the value of field F.
namespace knob_rule {
template <auto F>
using field_t = std::remove_reference_t<decltype(std::declval<Knobs&>().*F)>;
template <auto F>
void flag(Knobs& k, const char* e) { k.*F = atoi(e) != 0; }
template <auto F>
void raw_int(Knobs& k, const char* e) { k.*F = (field_t<F>)atoi(e); }
template <auto F, int LO, int HI>
void int_in(Knobs& k, const char* e) { k.*F = (field_t<F>)std::min(std::max(atoi(e), LO), HI); }
template <auto F>
void u64(Knobs& k, const char* e) { k.*F = strtoull(e, nullptr, 10); }
template <auto F>
void i64(Knobs& k, const char* e) { k.*F = atoll(e); }
inline void wide_or_16(Knobs& k, const char* e) { k.precomp_bits = atoi(e) == (int)WIDE_BITS ? (int)WIDE_BITS : MSM377_WINDOW_BITS; }
inline void four_or_8(Knobs& k, const char* e) { k.sort_elem = atoi(e) == 4 ? 4u : 8u; }
inline void check_mask(Knobs& k, const char* e) { k.base_checks = check_flags_normal((uint32_t)strtoul(e, nullptr, 0)); }  // (an invalid mask reads as 0)
}  // namespace knob_rule

inline Knobs Knobs::from_env() {
  using namespace knob_rule;
  static constexpr struct {
    const char* name;
    void (*rule)(Knobs&, const char*);
  } TABLE[] = {
      {"MSM377_GLV", raw_int<&Knobs::glv_mode>},
      {"MSM377_G1_FORM", flag<&Knobs::g1_form>},
      {"MSM377_CONV_WAVE_PRIO", flag<&Knobs::conv_wave_prio>},
      {"MSM377_AFF_PREWAKE_US", i64<&Knobs::aff_prewake_us>},
      {"MSM377_UPLOAD_CHUNKS", int_in<&Knobs::upload_chunks, 2, 7>},
      {"MSM377_UPLOAD_SPLIT", int_in<&Knobs::upload_split_pct, 5, 90>},
      {"MSM377_UPLOAD_CHUNK_MIN", u64<&Knobs::upload_chunk_min>},
      {"MSM377_TAIL_THREADS", int_in<&Knobs::tail_threads, 1, TailPool::WORKERS + 1>},
      {"MSM377_TAIL_WAIT_MS", int_in<&Knobs::tail_wait_ms, 1, INT_MAX>},
      {"MSM377_TAIL_SPIN_US", i64<&Knobs::tail_spin_us>},
      {"MSM377_TAIL_TRACE", flag<&Knobs::tail_trace>},
      {"MSM377_TAIL_NUMA", flag<&Knobs::tail_numa>},
      {"MSM377_TE_AFFINE_MSM", flag<&Knobs::te_affine_msm>},
      {"MSM377_NARROW_MAX", u64<&Knobs::narrow_max_points>},
      {"MSM377_PRECOMP_BITS", wide_or_16},
      {"MSM377_AFFINE_MIN", u64<&Knobs::affine_min_points>},
      {"MSM377_SEG_PLAIN", int_in<&Knobs::seg_plain, (int)SEG_MIN, (int)SEG_MAX>},
      {"MSM377_SEG_GLV", int_in<&Knobs::seg_glv, (int)SEG_MIN, (int)SEG_MAX>},
      {"MSM377_ZERO_COPY_OUT", raw_int<&Knobs::zc_out>},
      {"MSM377_NARROW_SEG", int_in<&Knobs::narrow_seg, (int)NARROW_SEG, (int)SEG_BINS - 1>},
      {"MSM377_NARROW_QUAD_ITEMS", u64<&Knobs::narrow_quad_items>},
      {"MSM377_COOP_THREADS", raw_int<&Knobs::coop_threads>},
      {"MSM377_NARROW_TAIL_FROM", int_in<&Knobs::narrow_tail_from, 1, (int)TREE_LEVELS>},
      {"MSM377_TAIL_LDS", flag<&Knobs::tail_lds>},
      {"MSM377_REDUCE_COLUMNS", flag<&Knobs::reduce_columns>},
      {"MSM377_EVEN_WINDOWS", flag<&Knobs::even_windows>},
      {"MSM377_SORT_ELEM", four_or_8},
      {"MSM377_TWIN_BATCH", flag<&Knobs::twin_batches>},
      {"MSM377_BASE_CHECKS", check_mask},
      {"MSM377_TAIL_FROM", int_in<&Knobs::tail_from, 1, (int)TREE_LEVELS>},
  };
  Knobs k;
  for (const auto& row : TABLE)
    if (const char* e = getenv(row.name)) row.rule(k, e);
  return k;
}

}  // namespace msm377
