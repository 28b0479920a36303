// The engine context behind the opaque msm377_ctx of include/msm377.h: streams, events, device workspace (layout: DESIGN.md
// section 3), pinned host buffers, the knobs (knobs.hpp).  Shared by sequencer.hip, host_tail.hip and capi.hip; its life
// cycle -- create, destroy and every buffer that is allocated on demand -- is context.hip, and whatever a context
// allocates goes through its Resources, which gives all of it back.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

#include "common.hpp"
#include "fp64_host.hpp"
#include "knobs.hpp"
#include "tail_pool.hpp"

using msm377::SortElem;
using msm377::WorkItem;
using msm377::TailPool;
using msm377::Fp64;
using msm377::MAX_WINDOW_SLOTS;
using msm377::NARROW_SEG;
using msm377::Knobs;

// Everything a context has taken from the HIP runtime: device and pinned allocations, events, streams.  No allocator:
// hipMalloc and friends stay the calls underneath; this records what they returned so that release_all() -- the one
// place a context's resources end -- needs no list kept by hand.  A call that fails leaves *p null and returns the error.
struct Resources {
  std::vector<void*> device, pinned;
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> streams;
  hipError_t alloc(void** p, size_t bytes);
  hipError_t alloc_pinned(void** p, size_t bytes, unsigned flags = hipHostMallocDefault);
  hipError_t event(hipEvent_t* e, unsigned flags = hipEventDefault);
  hipError_t stream(hipStream_t* s, const int* priority = nullptr);  // non-blocking; priority: as hipStreamCreateWithPriority
  void release(void* p);  // a device buffer that is given back early or regrown (no-op on nullptr)
  void release_all();
};

// The resident base table of the fixed-base entry points.  Valid only from the successful end of a msm377_g1_set_bases*
// call until a call writes d_bases, d_raw_points or the table: every writer clear()s it first and a successful build
// sets it as its last step.  The twin of a context borrows the whole value for the length of a batch call.
struct ResidentBases {
  uint64_t n = 0;              // resident base count (0: none)
  int form = 0;                // TableForm (sequencer.hip) of the records
  uint32_t* bases = nullptr;   // the base records: the owner's d_bases
  // The precomputed-window table: `windows` x cap affine records, [2^(c w)] P_i at record w * n + i.  The allocation
  // outlives clear(); free_table (sequencer.hip) gives it back to the owner's Resources.
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

// One window table the batch calls keep between calls: the records, and the (base, width) they were built for.  The rule
// is the resident base table's and it is written once, in the table builder (sequencer.hip build_mul_tables): a build
// clears `valid` of every slot it rebuilds FIRST and sets it as its last step, behind a wait for its launches, so a
// failed build leaves no table behind.  Each slot is its own allocation, made when it is first built and regrown for a
// wider table.
struct MulTableSlot {
  bool valid = false;
  uint8_t key[96] = {};    // the base's wire bytes: 96 on G1; 64 on Edwards-BLS12, the rest zero
  int width = 0;           // window width of the table in `table`
  uint32_t* table = nullptr;
  uint64_t table_cap = 0;  // records allocated
};

// Fixed-base batch multiplication (msm377_g1_batch_mul*, kernels/batch_mul.hpp): the window table of ONE base and the
// fixed-size scratch a chunk of outputs passes through, which every other batch call borrows.  Nothing here is shared
// with the MSM paths or the check calls.
struct BatchMulState {
  int window = 0;          // msm377_ctx_set_mul_window: 0 = the rule by n, else the forced width
  int last_window = 0;     // width the last call ran (msm377_ctx_get_last_mul_window)
  uint64_t builds = 0;     // table builds so far (msm377_ctx_get_mul_table_builds)
  MulTableSlot single;     // the table of the single-base call
  uint32_t* stash = nullptr;        // BM_PIECES x BM_CHUNK 16-byte pieces
  uint32_t* trees = nullptr;        // one product tree per workgroup of a chunk
  uint32_t* block_prod = nullptr;   // 13 limbs per workgroup: its product, then (block_inv) the inverse
  uint32_t* block_inv = nullptr;
  uint32_t* row_bases = nullptr;    // (W + 1) table records: [2^(c w)]B
  uint32_t* base_wire = nullptr;    // the base's 96 bytes on the device
  // Variable-base calls (msm377_g1_batch_mul_var*, kernels/batch_mul_var.hpp): the per-point tables of ONE pass, [1..8]P_i
  // as 128-byte records (128 MB), rebuilt by every pass and never valid between calls.  They share the scratch above.
  // The pairwise linear combination (msm377_g1_batch_lincomb2*, kernels/batch_lincomb2.hpp) keeps the two tables of ITS
  // pass here, [1..8]P_i then [1..8]Q_i for half as many indices.
  uint32_t* var_table = nullptr;
};

// Multi-base batch multiplication (msm377_g1_batch_mul_multi*, kernels/batch_mul_multi.hpp): one window table per base
// POSITION.  The stash, the trees and the block products are BatchMulState's; the forced width and the last width are
// too (msm377_ctx_set_mul_window speaks for every batch_mul call).  Nothing else is shared with it: the single-base
// table, its key and its build count are not touched from here.
struct BatchMulMultiState {
  MulTableSlot slot[MSM377_MUL_MAX_BASES];
  uint64_t builds = 0;              // slots built so far (msm377_ctx_get_mul_multi_table_builds)
  uint32_t* row_bases = nullptr;    // MSM377_MUL_MAX_BASES x (W + 1) table records: [2^(c w)]B_b of the slots being built
  uint32_t* bases_wire = nullptr;   // their 96 bytes each on the device
};

// Edwards-BLS12 batch multiplication (msm377_ed_batch_mul_multi*, kernels/ed_batch_mul.hpp): one window table per base
// POSITION.  The stash, the trees, the block products, the build's row-base scratch (BatchMulMultiState's, used and
// waited for inside a build only) and the forced / last width are the G1 batch calls'; no G1 table, key or build count
// is read or written from here.
struct EdBatchMulState {
  MulTableSlot slot[MSM377_MUL_MAX_BASES];
  uint64_t builds = 0;  // slots built so far (msm377_ed_ctx_get_mul_table_builds)
  // The variable-base call (msm377_ed_batch_mul_var*, kernels/ed_batch_mul_var.hpp): the counters of ITS point check
  // (CHK_WORDS words, allocated on first use).  Its per-point tables are BatchMulState::var_table.
  uint32_t* point_check = nullptr;
  // The pairwise linear combination (msm377_ed_batch_lincomb2*, kernels/ed_batch_lincomb2.hpp): the counters of ITS two
  // point checks, p's then q's (2 x CHK_WORDS words, allocated on first use).
  uint32_t* pair_check = nullptr;
  // The k-term linear combination (msm377_ed_batch_lincomb*, kernels/ed_batch_lincomb.hpp): the counters of ITS point checks,
  // a set per term (MSM377_LINCOMB_MAX_TERMS x CHK_WORDS words, allocated on first use), and the per-point tables of ONE
  // pass of 2^16 outputs, [1..8]P_ij for lincomb_terms terms (64 MB each) as ONE allocation of the call's own: regrown when a
  // call brings more terms, never shrunk, never valid between calls.  BatchMulState::var_table is not used.
  uint32_t* lincomb_check = nullptr;
  uint32_t* lincomb_table = nullptr;
  uint32_t lincomb_terms = 0;
};

// The resident generator set of the row commitments (msm377_g1_set_generators / msm377_g1_commit_rows*,
// kernels/commit_rows.hpp): the window tables of k generators at ONE width as ONE allocation, table j at record
// j * bm_table_records(width).  The rule is ResidentBases': msm377_g1_set_generators drops the set (and gives its
// memory back) before anything else and sets k as its last step, behind a wait for the build.  The build's own buffers
// (row bases and wire bytes sized for k) live for the length of the build.  The calls borrow BatchMulState's stash, trees and block products and nothing else:
// no table, key, width or build count of the batch_mul calls is read or written from here.
// The Edwards-BLS12 calls (msm377_ed_set_generators / msm377_ed_commit_rows*, kernels/ed_commit_rows.hpp) keep a second
// set of the same shape, ed_gens, under the same rule: either set is set, dropped or failed without a look at the other.
struct GeneratorSet {
  uint32_t k = 0;             // resident generators (0: no set)
  int width = 0;              // window width of the tables: 8 or 16
  uint32_t* tables = nullptr;
  uint32_t* check = nullptr;  // Edwards-BLS12: the counters of the set's own generator check (CHK_WORDS words, allocated on first use, kept across sets)
  bool valid() const { return k != 0; }
};

// Work buffers of the 20-bit-window sort (kernels/wide.hpp) for up to `cap` points.
struct WideBuffers {
  uint32_t* digits = nullptr;  // 13 x n u32 biased 20-bit digits, the flat list the sort reads
  SortElem* temp = nullptr;    // output of the second partition pass (the first one writes d_sort_temp)
  uint32_t* counts = nullptr;  // the sort's counters and offsets (kernels/wide.hpp WC_*)
  uint64_t cap = 0;
  // counts_words: WC_WORDS of kernels/wide.hpp.  false: out of device memory (nothing allocated)
  bool ensure(Resources& own, uint64_t n, size_t counts_words);
  void release(Resources& own);
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
  // The window records of the pass, for msm377_g1_read_partials: written in enqueue_reduce beside the k_gather_partials
  // launch, from the launch's own arguments and the plan the host tail is then called with.
  msm377_partials_info partials = {};
  const uint32_t* d_partials = nullptr;  // what k_gather_partials wrote to (slot 0 of ctx->d_partials for every call the capture modes describe)
};

// What the last enqueue_accumulate launched with, for msm377_g1_read_work_list: written beside its launches (sequencer.hip)
// under stage capture, from the LaunchRecord they were given.  valid: from there until something else writes the front of
// d_work_meta (the check calls, msm377_scalars_width_device: they clear it); the read-back also asks for StageLayout::valid.
struct WorkListLayout {
  bool valid = false;
  msm377_work_list_info info = {};      // the host's half; items, the counters and the histogram are read from the device
  uint32_t bkt_words = 64, coord_words = 16, limbs = 13;  // an overflow record: the bucket record of the pass
  const uint32_t *d_hist = nullptr, *d_total = nullptr, *d_counters = nullptr;  // LaunchRecord::work_hist / total / counters
};

// What the last base conversion left, for msm377_g1_read_bases: written on the host where the conversion is queued
// (sequencer.hip note_bases), never derived afterwards.  valid: the call that queued it came back MSM377_OK.
struct BasesLayout {
  bool valid = false;
  msm377_bases_info info = {};
  const uint32_t* d_records = nullptr;    // ctx->d_bases, or the precomputed-window table
  const uint32_t* d_flagged = nullptr;    // per-call imports: the device counter of flagged points (null: info.flagged holds it)
};

// What the last pass of the last batch call left in BatchMulState's stash, for msm377_read_walk_stash and
// msm377_g1_read_walk_tables: written on the host beside the launches (sequencer.hip note_walk, batch_device_call) from the
// values they were given.  valid: from the successful end of a batch call that ran a pass until the next batch call or
// msm377_g1_set_generators / msm377_ed_set_generators starts (sequencer.hip forget_walk): whatever writes the stash goes through one of the two.
struct WalkLayout {
  bool valid = false;
  msm377_walk_stash_info info = {};
  msm377_walk_tables_info tables = {};  // tables == 0: the pass walked no per-point tables
  const uint32_t* d_tables = nullptr;   // where they are: BatchMulState::var_table, or the k-term call's own (EdBatchMulState::lincomb_table)
};

// ---- what belongs together, by the functions that use it ----

// The batched affine conversion (sequencer.hip affine_convert_begin / affine_convert_finish, host_tail.hip
// invert_block_products*): sized for the context's capacity at creation.
struct AffineConvert {
  uint32_t* d_stash = nullptr;    // cap x 52 words: N1, N2, Z, running product per point (k_affine_up -> k_affine_down)
  uint32_t* d_trees = nullptr;    // one product tree (2 x 256 nodes x 13 words) per AFF_BLOCK_POINTS points
  uint32_t* h_prod = nullptr;     // pinned + coherent host memory the kernels access in place (dm_* = its device address)
  uint32_t* h_inv = nullptr;
  uint32_t* h_flag = nullptr;     // workgroups of k_affine_up that have delivered their product
  uint32_t *dm_prod = nullptr, *dm_inv = nullptr, *dm_flag = nullptr;
  uint32_t* d_count = nullptr;    // workgroups of k_affine_up that have delivered (device memory; the last one resets it)
  hipEvent_t up_done = nullptr;
  std::vector<Fp64::El> scratch;  // prefix products of the host's share of Montgomery's trick
};

// Zero-copy output of the full-MSM path (k_gather_partials, wait_zero_copy_out); the knob is Knobs::zc_out.
struct ZeroCopyOut {
  bool active = false;            // the call being enqueued / waited for uses it
  uint32_t out_seq = 0;           // sequence number of the last zero-copy call
  uint32_t acc_seq = 0;           // calls' accumulation kernels so far; h_flag[ACC_FLAG_WORD] follows it (k_merge_split_rows_quad)
  uint32_t* h_flag = nullptr;     // pinned: [0] sequence number, [1] error word
  uint32_t* dm_flag = nullptr;
  uint32_t* dm_partials = nullptr;  // device address of h_partials
  uint32_t* d_count = nullptr;
};

// Native input forms (msm377_ctx_set_input_format): the import pass (kernels/import.hpp) writes wire-format data into
// d_raw_points / d_raw_scalars and the pipeline runs unchanged behind it.  All three allocated on first use
// (ensure_import_buffers).
struct NativeImport {
  uint64_t cap = 0;                   // the context's capacity: what the buffers are sized for
  uint8_t* d_native = nullptr;        // host-buffer calls in a native form: cap x 104 bytes of points, then cap x 32 of scalars
  uint32_t* d_inf_mask = nullptr;     // two infinity masks (the one that travels with d_raw_points; the check calls' scratch), then their counters
  hipEvent_t import_done = nullptr;   // the side stream waits for it before it reads imported points
  size_t mask_words() const { return (size_t)(((cap + 31) / 32 + 3) & ~3ull); }
  size_t points_bytes() const { return ((size_t)cap * 104 + 15) & ~(size_t)15; }
  uint8_t* native_points() const { return d_native; }
  uint8_t* native_scalars() const { return d_native + points_bytes(); }
};

// Host-buffer entry points: pinned staging + copy workers (allocated on first use, reserve_host_staging).
struct HostStaging {
  uint8_t* h_stage = nullptr;  // cap x 128 bytes
  hipStream_t copy_stream[8] = {};
};

// What the last call left for the getters and the stage read-backs.
struct LastCall {
  uint64_t n = 0;
  uint32_t geom_windows = 0, geom_log = 0;  // window slots and bucket_log of the last enqueue (msm377_ctx_get_last_geometry, msm377_g1_read_stage)
  uint32_t sort_elem = 0;  // bytes per sort_temp element of the last enqueue's sort, 0: the narrow path (msm377_ctx_get_last_sort_elem_bytes)
  int form = -1;  // MSM377_STAGE_FORM_* of the buckets the last call left (stage read-backs)
  bool glv = false;
  int products = 0;        // field products per bucket addition of the last accumulation launch (bench.py's int32-mad roof)
  double stage_ms[MSM377_NUM_STAGES] = {};
  StageLayout stage;  // what the last enqueue_decompose launched with; valid is enqueue_windows' (msm377_g1_read_stage_ex)
  WorkListLayout work;  // what the last enqueue_accumulate launched with (msm377_g1_read_work_list)
  BasesLayout bases;  // what the last base conversion wrote (msm377_g1_read_bases)
  WalkLayout walk;    // what the last batch call's last pass left in the stash (msm377_read_walk_stash)
};

struct Fallbacks {
  uint64_t count = 0;            // reruns on the Weierstrass path after an exceptional case of the Edwards law
  uint32_t mask = 0;             // MSM377_FB_* bits of the last one
  uint64_t geometry_reruns = 0;  // passes discarded because a scalar did not fit their window geometry (ERR_NARROW_RANGE) and run again on another; msm377_stage_info
};

struct msm377_ctx {
  int device = 0;
  Resources own;                      // everything below that came from the HIP runtime; release_all() at destroy
  Knobs knobs;                        // from the environment at creation, then the setters; a twin's: its owner's (twin_prepare)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;      // base conversion, overlapped with decompose + sort
  hipEvent_t bases_ready = nullptr;
  uint64_t cap = 0;
  std::string err;
  // device buffers: the pipeline workspace
  uint32_t* d_raw_points = nullptr;   // cap x 24 words (host-buffer API staging); a twin has none
  uint32_t* d_raw_scalars = nullptr;  // cap x 8 words
  uint32_t* d_bases = nullptr;        // cap x 32 words; a twin has none (it borrows `resident`)
  uint16_t* d_digits = nullptr;       // 16 x cap
  uint32_t* d_range_counts = nullptr; // NRANGE x (window slots x chunks <= MAX_SORT_BLOCKS): per-chunk range counts, then write offsets
  uint32_t* d_region_base = nullptr;  // 16 x (NRANGE + 1)
  SortElem* d_sort_temp = nullptr;    // 16 x cap partitioned (index|sign, key) pairs; the packed form (SortElem4) fills half of it
  uint32_t* d_row_ptr = nullptr;      // 16 x RP
  uint32_t* d_val_idx = nullptr;      // 16 x cap
  uint32_t* d_buckets = nullptr;      // 16 x 52 x NB
  uint32_t* d_buckets_snap = nullptr; // stage capture only (allocated by msm377_ctx_set_stage_capture)
  uint32_t* d_partials = nullptr;     // 2 slots x 16 x 16 x 52 (double-buffered for batches)
  WorkItem* d_work = nullptr;         // sorted accumulation work items (<= 16 NB + 16 cap / SEG)
  uint32_t* d_work_meta = nullptr;    // META_BLOCK_WORDS: [0..SEG] length histogram, [SEG_BINS..] cursors, then total, split-row count, overflow count, key_max[16]
  uint32_t* d_row_ovf_base = nullptr; // 16 x NB
  uint32_t* d_split_rows = nullptr;   // 16 x NB
  uint32_t* d_ovf = nullptr;          // overflow partial points, 52 words each (<= 16 cap / SEG)
  int* d_err = nullptr;               // 2 slots
  // pinned host
  uint32_t* h_partials = nullptr;     // 2 slots
  int* h_err = nullptr;               // 2 slots
  hipEvent_t done_ev[2] = {};
  hipEvent_t ev[MSM377_NUM_STAGES][2] = {};  // [stage][begin, end]
  // modes of use
  uint32_t point_form = MSM377_POINTS_WIRE, scalar_form = MSM377_SCALARS_WIRE;  // msm377_ctx_set_input_format
  int capture = 0;  // msm377_ctx_set_stage_capture: 0 off, 1 the sixteen-equal-windows route of msm377_g1_read_stage, 2 as run
  int timing = 0;   // msm377_ctx_set_timing: 0 off, 1 every stage, 2 the accumulation kernel only
  ResidentBases resident;             // fixed-base mode: the bases of the last successful msm377_g1_set_bases* call
  BatchMulState bm;                   // fixed-base batch multiplication: its table and scratch (allocated on first use)
  BatchMulMultiState bmm;             // multi-base batch multiplication: a table per base position (allocated when built)
  EdBatchMulState edbm;               // Edwards-BLS12 batch multiplication: a table per base position (allocated when built)
  GeneratorSet gens;                  // row commitments: the resident generator tables (one allocation per set)
  GeneratorSet ed_gens;               // Edwards-BLS12 row commitments: that curve's resident generator tables, independent of gens
  WideBuffers wide;                   // the 20-bit-window sort's buffers (allocated with such a table; the twin's own set)
  AffineConvert aff;
  ZeroCopyOut zc;
  NativeImport native;
  HostStaging staging;
  LastCall last;
  Fallbacks fallback;
  msm377_check_report last_check = {0, 0, 0, 0, UINT64_MAX, 0, 0};  // the report of the last check of a base set (Knobs::base_checks)
  std::function<int()> before_accumulate;  // host-buffer entry point: joins the point upload and launches the base conversion (enqueue_accumulate)
  TailPool tail_pool;
  // Batches on two sets of streams and buffers (sequencer.hip twin_prepare)
  msm377_ctx* twin = nullptr;   // owned; borrows `resident` for the length of a batch call
  bool twin_failed = false;
};

// ---- life cycle (context.hip) ----
namespace msm377 {
namespace eng {

// msm377_ctx_create is ctx_create(device, max_points, Knobs::from_env(), false, out).  borrows_bases: a twin, which
// only ever borrows the resident bases and is never given d_bases and d_raw_points (352 bytes per point).
int ctx_create(int device, uint64_t max_points, const Knobs& knobs, bool borrows_bases, msm377_ctx** out);
void ctx_destroy(msm377_ctx* ctx);
int set_stage_capture(msm377_ctx* ctx, int enabled);  // allocates the bucket snapshot with the first non-zero mode
int reserve_host_staging(msm377_ctx* ctx);
int ensure_import_buffers(msm377_ctx* ctx, bool host_staging);
int bm_alloc(msm377_ctx* ctx, uint32_t** p, size_t bytes);  // a buffer of BatchMulState, if it is not there yet

}  // namespace eng
}  // namespace msm377
