// The engine context behind the opaque msm377_ctx of include/msm377.h: streams, events, device workspace (layout: DESIGN.md
// section 3), pinned host buffers, tuning state.  Shared by sequencer.hip, host_tail.hip and capi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

#include "common.hpp"
#include "fp64_host.hpp"
#include "tail_pool.hpp"

using msm377::SortElem;
using msm377::WorkItem;
using msm377::TailPool;
using msm377::Fp64;
using msm377::MAX_WINDOW_SLOTS;
using msm377::NARROW_SEG;

// The resident base table of the fixed-base entry points.  Valid only from the successful end of a msm377_g1_set_bases*
// call until a call writes d_bases, d_raw_points or the table: every writer clear()s it first and a successful build
// sets it as its last step.  The twin of a context borrows the whole value for the length of a batch call.
struct ResidentBases {
  uint64_t n = 0;              // resident base count (0: none)
  int form = 0;                // TableForm (sequencer.hip) of the records
  uint32_t* bases = nullptr;   // the base records: the owner's d_bases
  // The precomputed-window table: `windows` x cap affine records, [2^(c w)] P_i at record w * n + i.  The allocation
  // outlives clear(); free_table (sequencer.hip) gives it back.
  uint32_t* table = nullptr;
  uint64_t cap = 0;
  uint32_t windows = 0;        // 16 (c = 16), or WIDE_WINDOWS (c = 20: six 20-bit + seven 19-bit windows)
  // Identity points of a set that came in with infinity flags (MSM377_POINTS_MONT_FLAG): their records hold the generator,
  // and every fixed-base call zeroes their scalars through the mask (kernels/import.hpp).  flagged == 0: nothing to do.
  uint32_t flagged = 0;
  const uint32_t* inf_mask = nullptr;  // the owner's d_inf_mask: bit i mod 32 of word i / 32
  bool valid() const { return n != 0; }
  void clear() { n = 0; flagged = 0; }
  void set(uint32_t* records, uint64_t count, int table_form, uint32_t flagged_points = 0, const uint32_t* mask = nullptr) {
    bases = records; n = count; form = table_form; flagged = flagged_points; inf_mask = mask;
  }
};

// Fixed-base batch multiplication (msm377_g1_batch_mul*, kernels/batch_mul.hpp): the window table of ONE base, keyed by
// the base's 96 wire bytes and the window width, and the fixed-size scratch a chunk of outputs passes through.  Like the
// resident base table the window table is valid only from the successful end of a build: a build clears `valid` first
// and sets it as its last step.  Nothing here is shared with the MSM paths or the check calls.
struct BatchMulState {
  int window = 0;          // msm377_ctx_set_mul_window: 0 = the rule by n, else the forced width
  int last_window = 0;     // width the last call ran (msm377_ctx_get_last_mul_window)
  uint64_t builds = 0;     // table builds so far (msm377_ctx_get_mul_table_builds)
  bool valid = false;
  uint8_t base[96] = {};   // key: the base ...
  int width = 0;           // ... and the width of the table in `table`
  uint32_t* table = nullptr;        // records of the current table
  uint64_t table_cap = 0;           // records allocated
  uint32_t* stash = nullptr;        // BM_PIECES x BM_CHUNK 16-byte pieces
  uint32_t* trees = nullptr;        // one product tree per workgroup of a chunk
  uint32_t* block_prod = nullptr;   // 13 limbs per workgroup: its product, then (block_inv) the inverse
  uint32_t* block_inv = nullptr;
  uint32_t* row_bases = nullptr;    // (W + 1) table records: [2^(c w)]B
  uint32_t* base_wire = nullptr;    // the base's 96 bytes on the device
  // Variable-base calls (msm377_g1_batch_mul_var*, kernels/batch_mul_var.hpp): the per-point tables of ONE pass, [1..8]P_i
  // as 128-byte records (128 MB), rebuilt by every pass and never valid between calls.  They share the scratch above.
  uint32_t* var_table = nullptr;
};

// Work buffers of the 20-bit-window sort (kernels/wide.hpp) for up to `cap` points.
struct WideBuffers {
  uint32_t* digits = nullptr;  // 13 x n u32 biased 20-bit digits, the flat list the sort reads
  SortElem* temp = nullptr;    // output of the second partition pass (the first one writes d_sort_temp)
  uint32_t* counts = nullptr;  // the sort's counters and offsets (kernels/wide.hpp WC_*)
  uint64_t cap = 0;
  bool ensure(uint64_t n);     // sequencer.hip; false: out of device memory (nothing allocated)
  void release() {
    for (void* p : {(void*)digits, (void*)temp, (void*)counts}) (void)hipFree(p);  // (no-op on nullptr)
    *this = WideBuffers();
  }
};

// What the last enqueue_decompose launched with, for msm377_g1_read_stage_ex: written next to the launch itself
// (sequencer.hip) from the values they were given, so that the read-back describes the kernels' arguments and not a second
// derivation of them.  valid: a whole call (front and back phase, from window 0) ran to its end under stage capture.
struct StageLayout {
  bool valid = false;
  msm377_stage_info info = {};
  const void* d_digits = nullptr;       // the digit matrix the decomposition wrote: ctx->d_digits (u16) or ctx->wide.digits (u32)
  const uint32_t* d_key_max = nullptr;  // the call's key_max words, or null where the sort reads none
  uint32_t coord_words = 16, limbs = 13;  // a bucket record of the pass: four coordinate slots of coord_words words, `limbs` of them used
};

struct msm377_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;      // base conversion, overlapped with decompose + sort
  hipEvent_t bases_ready = nullptr;
  uint64_t cap = 0;
  std::string err;
  // device buffers
  uint32_t* d_raw_points = nullptr;   // cap x 24 words (host-buffer API staging)
  uint32_t* d_raw_scalars = nullptr;  // cap x 8 words
  uint32_t* d_bases = nullptr;        // cap x 32 words
  uint16_t* d_digits = nullptr;       // 16 x cap
  uint32_t* d_range_counts = nullptr; // NRANGE x (window slots x chunks <= MAX_SORT_BLOCKS): per-chunk range counts, then write offsets
  uint32_t* d_region_base = nullptr;  // 16 x (NRANGE + 1)
  SortElem* d_sort_temp = nullptr;    // 16 x cap partitioned (index|sign, key) pairs; the packed form (SortElem4) fills half of it
  uint32_t* d_row_ptr = nullptr;      // 16 x RP
  uint32_t* d_val_idx = nullptr;      // 16 x cap
  uint32_t* d_buckets = nullptr;      // 16 x 52 x NB
  uint32_t* d_buckets_snap = nullptr; // stage capture only
  uint32_t* d_partials = nullptr;     // 2 slots x 16 x 16 x 52 (double-buffered for batches)
  WorkItem* d_work = nullptr;         // sorted accumulation work items (<= 16 NB + 16 cap / SEG)
  uint32_t* d_work_meta = nullptr;    // META_BLOCK_WORDS: [0..SEG] length histogram, [SEG_BINS..] cursors, then total, split-row count, overflow count, key_max[16]
  uint32_t* d_row_ovf_base = nullptr; // 16 x NB
  uint32_t* d_split_rows = nullptr;   // 16 x NB
  uint32_t* d_ovf = nullptr;          // overflow partial points, 52 words each (<= 16 cap / SEG)
  // Native input forms (msm377_ctx_set_input_format): the import pass (kernels/import.hpp) writes wire-format data into
  // d_raw_points / d_raw_scalars and the pipeline runs unchanged behind it.  All three allocated on first use.
  uint32_t point_form = MSM377_POINTS_WIRE, scalar_form = MSM377_SCALARS_WIRE;
  uint8_t* d_native = nullptr;        // host-buffer calls in a native form: cap x 104 bytes of points, then cap x 32 of scalars
  uint32_t* d_inf_mask = nullptr;     // two infinity masks (the one that travels with d_raw_points; the check calls' scratch), then their counters
  hipEvent_t import_done = nullptr;   // the side stream waits for it before it reads imported points
  ResidentBases resident;             // fixed-base mode: the bases of the last successful msm377_g1_set_bases* call
  BatchMulState bm;                   // fixed-base batch multiplication: its table and scratch (allocated on first use)
  WideBuffers wide;                   // the 20-bit-window sort's buffers (allocated with such a table; the twin's own set)
  int precomp_bits = MSM377_WINDOW_BITS;  // window width msm377_g1_set_bases_precomputed builds its next table for: 16 or 20 (msm377_ctx_set_precompute_window, MSM377_PRECOMP_BITS)
  uint32_t* d_aff_stash = nullptr;    // cap x 52 words: N1, N2, Z, running product per point (k_affine_up -> k_affine_down)
  uint32_t* d_aff_trees = nullptr;    // one product tree (2 x 256 nodes x 13 words) per AFF_BLOCK_POINTS points
  uint32_t* h_aff_prod = nullptr;     // pinned + coherent host memory the kernels access in place (dm_* = its device address)
  uint32_t* h_aff_inv = nullptr;
  uint32_t* h_aff_flag = nullptr;     // workgroups of k_affine_up that have delivered their product
  uint32_t *dm_aff_prod = nullptr, *dm_aff_inv = nullptr, *dm_aff_flag = nullptr;
  uint32_t* d_aff_count = nullptr;    // workgroups of k_affine_up that have delivered (device memory; the last one resets it)
  hipEvent_t aff_up_done = nullptr;
  std::vector<Fp64::El> aff_scratch;  // prefix products of the host's share of Montgomery's trick
  bool te_affine_msm = true;          // MSM377_TE_AFFINE_MSM=0: msm377_g1_msm_device keeps projective records (A/B knob)
  // Below this the batched conversion does not pay: it costs ~9 more products per point than the projective record and
  // saves 16, but its two kernels and the host round trip sit in front of the accumulation, which they cannot hide
  // under the (short) sort of a small input.  Interleaved A/B, projective / affine ms per MSM (tools/ab_knobs.py):
  // 2^15 0.69 / 0.88, 2^16 0.75 / 0.89, 2^17 0.88 / 0.97, 2^18 1.19 / 1.26, 2^19 1.76 / 1.78, 2^20 2.89 / 2.79.  MSM377_AFFINE_MIN.
  uint64_t affine_min_points = 1ull << 20;
  int* d_err = nullptr;               // 2 slots
  // pinned host
  uint32_t* h_partials = nullptr;     // 2 slots
  int* h_err = nullptr;               // 2 slots
  hipEvent_t done_ev[2] = {};
  // host-buffer entry points: pinned staging + copy workers (allocated on first use)
  uint8_t* h_stage = nullptr;  // cap x 128 bytes
  hipStream_t copy_stream[8] = {};
  // state
  uint64_t last_n = 0;
  uint32_t last_geom_windows = 0, last_geom_log = 0;  // window slots and bucket_log of the last enqueue (msm377_ctx_get_last_geometry, msm377_g1_read_stage)
  uint32_t last_sort_elem = 0;  // bytes per sort_temp element of the last enqueue's sort, 0: the narrow path (msm377_ctx_get_last_sort_elem_bytes)
  int last_form = -1;  // MSM377_STAGE_FORM_* of the buckets the last call left (stage read-backs)
  int capture = 0;  // msm377_ctx_set_stage_capture: 0 off, 1 the sixteen-equal-windows route of msm377_g1_read_stage, 2 as run
  StageLayout stage;  // what the last enqueue_decompose launched with; valid is enqueue_windows' (msm377_g1_read_stage_ex)
  // Zero-copy output of the full-MSM path (k_gather_partials, wait_zero_copy_out); MSM377_ZERO_COPY_OUT=0: D2H copies + event.
  int zc_out = 1;
  bool zc_active = false;         // the call being enqueued / waited for uses it
  uint32_t out_seq = 0;           // sequence number of the last zero-copy call
  uint32_t* h_out_flag = nullptr; // pinned: [0] sequence number, [1] error word
  uint32_t* dm_out_flag = nullptr;
  uint32_t* dm_partials = nullptr;  // device address of h_partials
  uint32_t* d_out_count = nullptr;
  int timing = 0;  // msm377_ctx_set_timing: 0 off, 1 every stage, 2 the accumulation kernel only
  // First reduction level run with one addition per lane quad: the first level whose 4 lanes x additions x windows fit
  // coop_threads -- level 7 for 16 windows (measured: 18-24 -> 13-18 us per level from there on, slower before), 6 for 8, 4
  // for the 2 windows a rank of an 8-GPU window-sharded run owns.
  // MSM377_COOP_THREADS: a tree level runs one lane quad per addition once that takes at most this many threads.  65536 / 131072 /
  // 262144 make no difference on the main path (2^20: 2.74 ms each); on the narrow path 131072 moves its levels 0-2 to quads.
  uint32_t coop_threads = 131072;
  // MSM377_NARROW_TAIL_FROM: tail_from of the narrow-window path (2048 buckets per window).  Reduce stage at 2^12 with
  // 7 / 5 / 4 / 3 / 2: 0.106 / 0.099 / 0.096 / 0.101 / 0.122 ms (profiles/r02_final/ab_narrow_tree.txt).
  uint32_t narrow_tail_from = 4;
  uint32_t narrow_seg = 0;  // MSM377_NARROW_SEG (>= NARROW_SEG: the buffers are sized for that); 0 = by input size (launch_record)
  uint64_t narrow_quad_items = 100000;  // MSM377_NARROW_QUAD_ITEMS: most work items k_accumulate_quad is used for (0: a thread per work item, like the main path)
  // First level of the single-launch tail of the reduction (k_reduce_tail); MSM377_TAIL_FROM, 15 = one launch per level throughout.
  uint32_t tail_from = 7;  // measured (tools/ab_knobs.py, 2^20): 15: 2.874 ms, 7: 2.842, 6: 2.885, 5: 2.916, 4: 3.062
  // MSM377_REDUCE_COLUMNS=0: the levels below tail_from run one launch per level (k_tree_step / k_tree_step_quad) instead of
  // as column launches of up to four levels each (k_tree_columns); same records either way, kept for A/B runs and the tests.
  bool reduce_columns = true;
  // GLV front end of the Weierstrass path: 0 = off (default), 1 = on.  phi(P) = [lambda] P holds only for points of
  // the prime-order subgroup, so it is an opt-in: the caller vouches for the inputs (every protocol use does).
  // Interleaved A/B on one MI355X (tools/ab_knobs.py), Weierstrass plain vs GLV ms per MSM: 2^18 1.39 / 1.24,
  // 2^19 2.08 / 2.00, 2^20 3.56 / 3.51, 2^22 12.56 / 12.39 (halved bucket reduction and host tail).
  int glv_mode = 0;
  int g1_form = 1;         // G1 full-MSM entry points: 1 = twisted Edwards form (te377.hpp, default), 0 = Weierstrass XYZZ (MSM377_G1_FORM)
  bool last_glv = false;
  uint32_t seg_plain = 0, seg_glv = 0;  // MSM377_SEG_PLAIN / MSM377_SEG_GLV: force the work-item length (SEG_MIN..SEG_MAX), 0 = auto_seg()
  hipEvent_t ev[MSM377_NUM_STAGES][2] = {};  // [stage][begin, end]
  uint64_t upload_chunk_min = 1ull << 18;  // msm377_g1_msm: inputs of at least this many points upload and run as two chunks (MSM377_UPLOAD_CHUNK_MIN)
  uint32_t upload_chunks = 4;              // chunks of the host-buffer upload (MSM377_UPLOAD_CHUNKS, 2..7): 2: 5.07, 3: 4.89, 4-6: 4.70, 8: 4.95 ms at 2^20 (round 2)
  uint32_t upload_split_pct = 30;          // share of the points in the first chunk (MSM377_UPLOAD_SPLIT, 5..90)
  std::function<int()> before_accumulate;  // host-buffer entry point: joins the point upload and launches the base conversion (enqueue_accumulate)
  TailPool tail_pool;
  int tail_threads = 6;               // MSM377_TAIL_THREADS: threads of the host tail (1..8, tail_horner_mt)
  // MSM377_TAIL_SPIN_US: how long at most the tail workers poll for their job after a call has armed them (TailPool;
  // 0 = they sleep until the job is posted).  Tail stage at 2^20, interleaved (tools/ab_knobs.py): one thread 0.140 ms,
  // six sleeping workers 0.124, six polling ones 0.089.  (Round 2 first measured no difference: the per-thread
  // exceptional-case flags shared a cache line then and the threads fought over it -- TeChecked is padded now.)
  // MSM377_AFF_PREWAKE_US: the helper threads that invert the conversion's block products are woken when the way up is
  // queued and poll for their share (at most this long) instead of being woken from their condition variable when the
  // products arrive -- the wake-up (20-60 us) sat in the middle of the front end's critical path.  0 = off.
  int64_t aff_prewake_us = 600;
  // MSM377_CONV_WAVE_PRIO: the conversion kernels (k_affine_up / k_affine_down) raise their waves' issue priority
  // (s_setprio 3) over the front-end kernels that run beside them on the main stream.
  uint32_t conv_wave_prio = 1;
  int64_t tail_spin_us = 1000;
  bool tail_trace = false;  // MSM377_TAIL_TRACE=1
  double stage_ms[MSM377_NUM_STAGES] = {};
  int last_products = 0;        // field products per bucket addition of the last accumulation launch (bench.py's int32-mad roof)
  // Inputs of at most this many points run the narrow-window path (22 windows of 2048 buckets instead of
  // 16 x 32768; MSM377_NARROW_MAX, 0 = never).  Interleaved A/B, 16-bit / narrow ms per MSM (tools/ab_knobs.py):
  // 2^10 0.64 / 0.46, 2^13 0.67 / 0.53, 2^14 0.68 / 0.51, 2^15 0.73 / 0.60, 2^16 0.74 / 0.71 (first version, 23 windows); at the end of
  // round 2: 2^16 0.605 / 0.56 (its bucket reduction 0.28 / 0.10 ms, its accumulation kernel 0.14 / 0.18), hence 2^16.
  uint64_t narrow_max_points = 1ull << 16;
  // Batches on two sets of streams and buffers (sequencer.hip twin_prepare)
  bool tail_lds = true;         // MSM377_TAIL_LDS=0: the single-launch reduction tail works in global memory (k_reduce_tail)
  bool even_windows = true;     // MSM377_EVEN_WINDOWS=0: sixteen 16-bit windows on the 16-window paths (kernels/decompose.hpp k_decompose); the narrow path keeps its geometry
  // MSM377_SORT_ELEM: bytes per sort_temp element of the main path's sort.  8 (default): SortElem.  4: the packed SortElem4
  // wherever the call allows it (common.hpp sort_elem_bytes), for A/B runs and the tests, which run both forms.  Interleaved
  // A/B at 2^20, 15 pairs (profiles/sort_elem4/ab_sort_elem.txt): sort stage 0.264 -> 0.249 ms, k_accumulate starts 12-17 us
  // sooner, whole MSM 2.477 -> 2.469 ms (medians) with run-to-run spreads of 0.06 and 0.09: inside the noise, so 8 stays the default.
  uint32_t sort_elem = 8;
  uint32_t acc_seq = 0;  // calls' accumulation kernels so far; h_out_flag[ACC_FLAG_WORD] follows it (k_merge_split_rows_quad)
  msm377_ctx* twin = nullptr;   // owned; borrows `resident` for the length of a batch call
  bool twin_batches = true;     // MSM377_TWIN_BATCH=0: batches run on this context alone
  bool twin_failed = false;
  // MSM377_BASE_CHECKS / msm377_ctx_set_base_checks: MSM377_CHECK_* flags (normalised) the set-bases calls check a base set
  // with before they convert it; 0 = none.  last_check: the report of the last such check.
  uint32_t base_checks = 0;
  msm377_check_report last_check = {0, 0, 0, 0, UINT64_MAX, 0, 0};
  uint64_t fallback_count = 0;  // reruns on the Weierstrass path after an exceptional case of the Edwards law
  uint64_t geometry_reruns = 0; // passes discarded because a scalar did not fit their window geometry (ERR_NARROW_RANGE) and run again on another; msm377_stage_info
  uint32_t fallback_mask = 0;   // MSM377_FB_* bits of the last one
};
