// msm377: BLS12-377 G1 multi-scalar multiplication for MI355X (gfx950), C ABI in include/msm377.h.
// This translation unit is the stage sequencer: it owns every kernel launch (kernels/*.hpp are compiled here and only
// here), the stream / event choreography of a call and the entry points' control flow (fallbacks, chunked uploads,
// batches, window shards).  The C ABI itself is capi.hip, the host tail host_tail.hip, the context context.hpp and
// its life cycle (create, destroy, every allocation) context.hip.
//
// Pipeline (each stage names the reference code it replaces; paths relative to /root/reference/src/submission/):
//   kernels/convert.hpp     k_affine_up / host inversion / k_affine_down (n >= 2^20, resident tables), k_convert_bases (otherwise)
//                           wire x||y -> Montgomery records            wgsl/cuzk/convert_point_coords_and_decompose_scalars.template.wgsl:41-99 + barrett.template.wgsl:60-82
//   kernels/decompose.hpp   k_decompose (16 windows), k_decompose_geom (inputs <= 2^16 points: 22 windows of 2^11 buckets, submission.ts:97)
//                           scalars -> signed digits                   same file :100-141; model cuzk/utils.ts:66-109
//   kernels/sort.hpp        k_range_count / k_range_scan / k_partition / k_local_sort (k_small_sort on the narrow path)
//                           per-window counting sort -> CSR            wgsl/cuzk/transpose_serial.wgsl:34-76 (16 serial threads there); model cuzk/transpose.ts:14-62
//   kernels/accumulate.hpp  k_accumulate: bucket sums (the dominant kernel)   wgsl/cuzk/smvp_bls12_377.template.wgsl:72-160
//   kernels/reduce.hpp      k_tree_step / k_tree_columns / k_tree_step_quad / k_reduce_tail / k_gather_partials
//                           bucket reduction, log-depth bit planes     wgsl/cuzk/bpr.template.wgsl:69-173; models cuzk/bpr.ts:5-126
//   host_tail.hip           Horner over windows + one inversion        submission.ts:290-321
// In front of all of it, only while msm377_ctx_set_input_format names a native form: kernels/import.hpp k_import_points /
// k_import_scalars (Montgomery coordinates and scalars, infinity flags -> wire records in d_raw_points / d_raw_scalars).
// The kernels are templates over a curve policy (curves.hpp): TeDev (default: G1 in twisted Edwards form, te377.hpp -- 7 field
// products per bucket addition on affine base records (TeAffBase), 8 on projective ones, unified law, exceptional cases
// detected and rerun), G1Dev (G1 in Weierstrass XYZZ coordinates, g1_xyzz.hpp: the fallback, the GLV front end, the
// stage read-backs) and EdDev (Edwards-BLS12 over the scalar field, ed_ext.hpp).  Everything behind the sort takes the
// bucket geometry as a run-time argument L (2^L buckets per window: 15 on the main path, 11 on the narrow one).
// HBM layout: DESIGN.md section 3.
//
// Host control flow, top to bottom in this file: a WindowPlan says which windows one attempt of a call runs and how the
// host combines their records (one constructor per geometry); enqueue_windows queues the stages of a Phase for its plan:
// one LaunchRecord of derived values, then enqueue_decompose / _sort / _accumulate / _reduce, one function per stage;
// wait_windows / geometry_refused / collect_windows / run_tail are the steps behind it.  g1_table_msm strings them together for
// every G1 MSM on base records that are in place, at full width or over short scalars, and the entry points are thin wrappers over one
// flow per kind of input (g1_device_flow, g1_host_flow, g1_fixed_base_flow, ed_device_flow); the chunked uploads, the
// batches and the window shards keep schedules of their own over the same steps.
// The batch calls (every output its own point: fixed-base, multi-base, Edwards-BLS12, row commitments, variable-base,
// pairwise) are not MSM paths and sit behind all of that, over one machinery of their own: one table builder, one
// normalisation, one flow of a device call, one staging of a host-buffer call; an entry point supplies its checks, its
// pass length and the launch of its hot kernel.
#include "sequencer.hpp"

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <initializer_list>
#include <thread>
#include <type_traits>
#include <vector>

#include "context.hpp"
#include "host_tail.hpp"
#include "ed_batch_mul_host.hpp"
#include "ed_batch_mul_var_host.hpp"
#include "ed_batch_lincomb2_host.hpp"
#include "ed_batch_lincomb_host.hpp"
#include "ed_commit_rows_host.hpp"
#include "validate_host.hpp"
#include "kernels/accumulate.hpp"
#include "kernels/batch_mul.hpp"
#include "kernels/batch_mul_multi.hpp"
#include "kernels/ed_batch_mul.hpp"
#include "kernels/ed_commit_rows.hpp"
#include "kernels/commit_rows.hpp"
#include "kernels/convert.hpp"
#include "kernels/decompose.hpp"
#include "kernels/generate.hpp"
#include "kernels/reduce.hpp"
#include "kernels/sort.hpp"
#include "kernels/validate.hpp"
#include "kernels/import.hpp"
#include "kernels/batch_mul_var.hpp"
#include "kernels/ed_batch_mul_var.hpp"
#include "kernels/ed_batch_lincomb2.hpp"
#include "kernels/ed_batch_lincomb.hpp"
#include "kernels/batch_lincomb2.hpp"
#include "kernels/wide.hpp"

namespace msm377 {
namespace eng {

bool hip_ok(msm377_ctx* ctx, int hip_error, const char* what) {
  const hipError_t e = (hipError_t)hip_error;
  if (e == hipSuccess) return true;
  if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}

namespace {

void note_fallback(msm377_ctx* ctx, uint32_t mask) {
  ctx->fallback.count++;
  ctx->fallback.mask = mask;
}

// Pageable host memory -> device through a pinned staging buffer: four workers copy ~4 MB pieces
// into it and queue the DMA of each piece on their own stream, so the CPU copy of one piece
// overlaps the DMA of the others.  Measured on the MI355X box for 160 MB: 4.2 ms, against 28 ms
// for a first hipMemcpy from fresh pageable pages (4.4 ms once the runtime has pinned them) and
// 3.3 + 2.9 ms for hipHostRegister + copy.  Returns when the data is on the device.  An upload thread passes `fail`: a
// HIP error and the call that failed go there, and the thread that joins it records them (only that one writes ctx->err).
struct HipFail {
  hipError_t e = hipSuccess;
  const char* what = "";
  int record(msm377_ctx* ctx, int rc) const {  // (no-op when nothing failed)
    hip_ok(ctx, e, what);
    return rc;
  }
};
int h2d_staged(msm377_ctx* ctx, void* d_dst, const uint8_t* src, size_t bytes, size_t stage_off, HipFail* fail = nullptr) {
#define H2D_TRY(call)                \
  do {                               \
    const hipError_t e_ = (call);    \
    if (e_ != hipSuccess) {          \
      if (fail) *fail = {e_, #call}; \
      else hip_ok(ctx, e_, #call);   \
      return MSM377_EHIP;            \
    }                                \
  } while (0)
  constexpr int NT_MAX = 8;
  constexpr int NT = 4;  // copy workers: 2, 4, 6 or 8 all moved 128 MB in 2.9-3.0 ms (round 2) -- the DMA sets the pace
  constexpr size_t SMALL = 8u << 20, PIECE = 4u << 20;
  if (bytes < SMALL) {  // not worth four threads
    H2D_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return MSM377_OK;
  }
  if (!ctx->staging.h_stage && reserve_host_staging(ctx) != MSM377_OK) {
    (void)hipGetLastError();
    H2D_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));  // fall back to the runtime's pageable path
    return MSM377_OK;
  }
  // Pieces of about 4 MB, their number a multiple of the worker count (with fixed 8 MB pieces a 48 MB upload took as
  // long as a 64 MB one); a thread's host copy of its next piece overlaps the DMA of the one before.  The pieces are
  // CLAIMED from a counter, by the NT workers and by the calling thread alike: every thread ends up with the same
  // amount when all run, and a worker that has lost its CPU leaves its pieces to the others instead of holding up the call.
  size_t npieces = (bytes + PIECE - 1) / PIECE;
  npieces = (npieces + NT - 1) / NT * NT;
  const size_t piece = ((bytes + npieces - 1) / npieces + 4095) & ~(size_t)4095;
  uint8_t* stage = ctx->staging.h_stage + stage_off;
  hipError_t errs[NT_MAX + 1];
  std::thread workers[NT_MAX];
  const int device = ctx->device;
  std::atomic<size_t> next{0};
  auto copy_pieces = [&, device](int t) {  // t: this thread's copy stream
    hipError_t e = hipSetDevice(device);
    for (;;) {
      const size_t c = next.fetch_add(1, std::memory_order_relaxed);
      const size_t off = c * piece;
      if (c >= npieces || off >= bytes || e != hipSuccess) break;
      const size_t len = (bytes - off < piece) ? bytes - off : piece;
      memcpy(stage + off, src + off, len);
      e = hipMemcpyAsync((uint8_t*)d_dst + off, stage + off, len, hipMemcpyHostToDevice, ctx->staging.copy_stream[t]);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->staging.copy_stream[t]);
    errs[t] = e;
  };
  for (int t = 0; t <= NT; t++) errs[t] = hipSuccess;
  for (int t = 0; t < NT; t++) workers[t] = std::thread([&copy_pieces, t] { copy_pieces(t); });
  copy_pieces(NT);  // the caller takes pieces too (its own stream)
  for (int t = 0; t < NT; t++) workers[t].join();
  for (int t = 0; t <= NT; t++) H2D_TRY(errs[t]);
  return MSM377_OK;
#undef H2D_TRY
}

void identity_wire(uint8_t out[96]) {
  memset(out, 0, 96);
  out[48] = 1;
}

struct StageTimer {  // HIP events around one stage of a call, on its stream
  msm377_ctx* c;
  int s;
  hipStream_t st;
  bool on() const { return c->timing == 1 || (c->timing == 2 && s == MSM377_STAGE_ACC_KERNEL); }
  StageTimer(msm377_ctx* ctx, int stage, hipStream_t stream) : c(ctx), s(stage), st(stream) {
    if (on()) (void)hipEventRecord(c->ev[s][0], st);
  }
  ~StageTimer() {
    if (on()) (void)hipEventRecord(c->ev[s][1], st);
  }
};

// The layout of the base records a conversion is about to leave (msm377_g1_read_bases): host bookkeeping next to the
// launch, nothing is queued or allocated.  first != 0: a later chunk of a chunked upload, behind the records of the chunks
// before it.  Under MSM377_POINTS_MONT_FLAG the import pass in front of every G1 conversion has counted the flagged points
// on the device (MASK_BASES); the read-back fetches the count from there.
void note_bases(msm377_ctx* ctx, uint32_t form, const uint32_t* d_records, uint64_t n, uint64_t first = 0, bool glv = false) {
  static const uint32_t REC[4] = {64, 40, 32, 32}, LIMBS[4] = {13, 13, 13, 9}, COORDS[4] = {4, 3, 2, 3};
  BasesLayout b;
  b.info.form = form;
  b.info.record_words = REC[form];
  b.info.limbs = LIMBS[form];
  b.info.coords = COORDS[form];
  b.info.n = first + n;
  b.info.windows = 1;
  b.info.glv = glv ? 1 : 0;
  b.info.window_stride = first + n;
  b.info.records = (glv ? 2 : 1) * (first + n);
  b.d_records = d_records;
  if (form != MSM377_BASES_ED && ctx->point_form == MSM377_POINTS_MONT_FLAG && ctx->native.d_inf_mask) b.d_flagged = ctx->native.d_inf_mask + 2 * ctx->native.mask_words();
  b.valid = true;
  ctx->last.bases = b;
}
template <class CV>
constexpr uint32_t bases_form_of() {
  return std::is_same<CV, TeDev>::value ? MSM377_BASES_TE_PROJECTIVE : std::is_same<CV, EdDev>::value ? MSM377_BASES_ED : MSM377_BASES_WEIERSTRASS;
}

template <class CV>
int convert_bases(msm377_ctx* ctx, const uint32_t* d_raw, uint64_t n, uint64_t first = 0, bool clear_err = true) {
  // Runs on the side stream: it depends on the points only, while decomposition and the sort
  // depend on the scalars only, so the two overlap (HBM-bound vs LDS/latency-bound);
  // k_accumulate waits for `bases_ready`.  The previous call's readers of d_bases are done: every entry point ends with
  // a host-side wait -- for the main stream's completion event, or (zero-copy output) for the sequence number that the
  // gather kernel publishes, and that kernel is the LAST launch of a call and reads the buckets only (the invariant
  // is spelled out at publish_to_host, kernels/reduce.hpp).
  if (n == 0) return MSM377_OK;
  if (ctx->timing == 1) (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][0], ctx->stream2);
  if (clear_err) hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, ctx->stream2, (uint32_t*)(ctx->d_err + 2), 1u, (uint32_t*)nullptr, 0u);
  hipLaunchKernelGGL(k_convert_bases<CV>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream2, d_raw, ctx->d_bases + first * CV::REC_WORDS, n,
                     ctx->d_err + 2);
  HIP_TRY(ctx, hipGetLastError());
  note_bases(ctx, bases_form_of<CV>(), ctx->d_bases, n, first);
  if (ctx->timing == 1) (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][1], ctx->stream2);
  HIP_TRY(ctx, hipEventRecord(ctx->bases_ready, ctx->stream2));
  return MSM377_OK;
}

// Phase 1, queued on the side stream: products up to one value per workgroup, delivered into pinned host memory.
// (Round 3 tried the conversion as TWO launches per direction, blocks [0, h) and [h, nblk), so that the host inverts the
// first half's products while the second half is still on its way up and the ~50 us round trip idles nothing: slower,
// 2.60 -> 2.72 ms at 2^20.  The conversion is latency-bound at two workgroups per CU -- a half-size launch is one
// workgroup per CU and takes 104 us where the full one takes 171 -- so the chain grew from 171 + 50 + 170 to 4 x ~110 us.)
// prev_window_records: build a window of a precomputed table instead, `doublings` doublings above the previous one's.
int affine_convert_begin(msm377_ctx* ctx, const uint32_t* d_raw, uint64_t n, const uint32_t* prev_window_records = nullptr, uint32_t doublings = 0,
                         bool clear_err = true) {
  if (n == 0) return MSM377_OK;
  const uint32_t nblk = affine_blocks(n);
  if (ctx->timing == 1) (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][0], ctx->stream2);
  __atomic_store_n(ctx->aff.h_flag, 0u, __ATOMIC_RELEASE);
  if (clear_err) hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, ctx->stream2, (uint32_t*)(ctx->d_err + 2), 1u, (uint32_t*)nullptr, 0u);
  if (prev_window_records)
    hipLaunchKernelGGL(k_affine_up<AffDoublingSource>, dim3(nblk), dim3(AFF_THREADS), 0, ctx->stream2, AffDoublingSource{prev_window_records, doublings}, n,
                       ctx->aff.d_stash, ctx->aff.d_trees, ctx->aff.dm_prod, ctx->aff.dm_flag, ctx->aff.d_count, ctx->d_err + 2, ctx->knobs.conv_wave_prio);
  else
    hipLaunchKernelGGL(k_affine_up<AffWireSource>, dim3(nblk), dim3(AFF_THREADS), 0, ctx->stream2, AffWireSource{d_raw}, n, ctx->aff.d_stash, ctx->aff.d_trees,
                       ctx->aff.dm_prod, ctx->aff.dm_flag, ctx->aff.d_count, ctx->d_err + 2, ctx->knobs.conv_wave_prio);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->aff.up_done, ctx->stream2));
  if (ctx->knobs.tail_threads > 1 && nblk >= 32) ctx->tail_pool.prewake(ctx->knobs.aff_prewake_us, std::min(ctx->knobs.tail_threads, TailPool::WORKERS + 1) - 1);
  return MSM377_OK;
}

// Phase 2: waits for phase 1 (the main stream keeps the GPU busy meanwhile), inverts the block products on the tail
// threads, queues the way down and signals `bases_ready`.
int affine_convert_finish(msm377_ctx* ctx, uint32_t* d_records_out, uint64_t n) {
  if (n == 0) return MSM377_OK;
  const uint32_t nblk = affine_blocks(n);
  // Poll the flag in pinned memory (no runtime calls: they would contend with nothing, but they are not free either);
  // after 20 ms fall back to the event, which also surfaces a failed kernel.
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 0; __atomic_load_n(ctx->aff.h_flag, __ATOMIC_ACQUIRE) != nblk; spins++) {
    __builtin_ia32_pause();
    if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
      HIP_TRY(ctx, hipEventSynchronize(ctx->aff.up_done));
      break;
    }
  }
  if (__atomic_load_n(ctx->aff.h_flag, __ATOMIC_ACQUIRE) != nblk) {
    ctx->err = "batched affine conversion: the block products did not arrive";
    return MSM377_EHIP;
  }
  {
    const int inv_rc = invert_block_products_mt(ctx, 0, nblk);
    ctx->tail_pool.disarm();  // (armed by affine_convert_begin; the tail arms them again once the accumulation is through)
    if (inv_rc) return inv_rc;
  }
  // The way down starts as soon as the host has inverted the block products, beside whatever the sort is doing (letting
  // it wait for the sort was measured both ways in round 2: 2^20 2.62 -> 2.59 ms, 2^22 10.39 -> 10.21 without the wait).
  hipLaunchKernelGGL(k_affine_down, dim3(nblk), dim3(AFF_THREADS), 0, ctx->stream2, n, ctx->aff.d_stash, ctx->aff.d_trees, ctx->aff.dm_inv, d_records_out, ctx->knobs.conv_wave_prio);
  HIP_TRY(ctx, hipGetLastError());
  note_bases(ctx, MSM377_BASES_TE_AFFINE, d_records_out, n);  // (a precomputed table: its last window; the caller describes the whole)
  if (ctx->timing == 1) (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][1], ctx->stream2);
  HIP_TRY(ctx, hipEventRecord(ctx->bases_ready, ctx->stream2));
  return MSM377_OK;
}

// Entries per accumulation work item.  The kernel is a list of ~(rows + entries / SEG) independent serial chains
// handed out longest-first to 2048 resident waves: too few, too long chains leave the last round of waves
// half-empty (GLV at 2^20 with SEG 96: 4400 waves, 2.83 ms; SEG 64: 6100 waves, 2.47 ms), too short ones pay an
// overflow record and a merge addition per extra chain.  Interleaved A/B runs (tools/ab_knobs.py) put the best
// length near entries / 2^18 for both front ends (entries = windows in this call x points per window): 32 at
// n = 2^19, 64 at 2^20, 96-128 at 2^21; a rank that owns one or two windows of a sharded MSM gets short chains,
// so that its few rows still fill the GPU.
uint32_t auto_seg(const msm377_ctx* ctx, uint64_t entries, bool glv) {
  const uint32_t forced = glv ? ctx->knobs.seg_glv : ctx->knobs.seg_plain;
  if (forced) return forced;
  const uint64_t s = ((entries >> 18) + 7) & ~7ull;
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(s, SEG_MIN), SEG_MAX);
}


// The windows of ONE attempt of a call: what the kernels run (launch_record reads the first half) and what the host
// tail combines afterwards (run_tail reads the second), written once, by the constructor of the geometry.  The recode
// families carry the names of tests/stage_model.py.
enum Recode { RECODE_EQUAL16, RECODE_EVEN16, RECODE_NARROW22, RECODE_SHORT, RECODE_WIDE13, RECODE_GLV8 };
enum TailKind { TE_TAIL, XYZZ_TAIL, ED_TAIL };  // te_tail / xyzz_tail / ed_tail, or (on_caller) teh_combine / g1h_combine
struct WindowPlan {
  Recode recode = RECODE_EQUAL16;
  uint32_t slots = MSM377_NUM_WINDOWS;           // window slots the call runs (GLV: over twice the columns; wide: one, fed 13 digits per point)
  uint32_t bucket_log = MSM377_WINDOW_BITS - 1;  // L: 2^L buckets per slot; everything behind the sort takes it as a run-time argument
  // Precomputed-window tables (msm377_g1_set_bases_precomputed): window slot ws gathers from record ws * table_stride + i
  // of `table`, and because the table already carries the windows' weights the bucket sets are ADDED together before
  // the reduction: one window's reduction, one window's partial record.
  const uint32_t* table = nullptr;
  uint64_t table_stride = 0;
  const uint32_t* bases_override = nullptr;  // base records of the call if not ctx->d_bases (the wide table's window 0 = the plain affine records)
  // Short scalars (RECODE_SHORT): d_scalars holds n x short_bytes bytes, every scalar below 2^short_bits.
  uint32_t short_bytes = 0, short_bits = 0;
  // The host tail: `records` window records of cbits()-bit digits, from window short_from on one bit narrower.
  TailKind tail = TE_TAIL;
  bool on_caller = false;  // combined on the calling thread: one folded record, the GLV windows, the MSMs of a batch beside the GPU
  int records = MSM377_NUM_WINDOWS;
  int short_from = 0;
  int cbits() const { return (int)bucket_log + 1; }  // signed digits: a window of c bits has 2^(c - 1) buckets
  int planes() const { return (int)bucket_log; }
};

// One constructor per geometry.
WindowPlan plan_equal16(TailKind tail, uint32_t slots = MSM377_NUM_WINDOWS) {  // sixteen 16-bit windows, or a shard's `slots` of them
  WindowPlan p;
  p.tail = tail;
  p.slots = slots;
  p.records = (int)slots;
  return p;
}
WindowPlan plan_even16(TailKind tail) {  // whole MSMs: the top three windows 15 bits wide (kernels/decompose.hpp k_decompose)
  WindowPlan p = plan_equal16(tail);
  p.recode = RECODE_EVEN16;
  p.short_from = EVEN_FROM;
  return p;
}
WindowPlan plan_narrow22() {  // small inputs: eleven signed 12-bit + eleven unsigned 11-bit windows (k_decompose_geom + k_small_sort)
  WindowPlan p = plan_equal16(TE_TAIL, NARROW_EVEN_WINDOWS);
  p.recode = RECODE_NARROW22;
  p.bucket_log = NARROW_LOG;
  p.short_from = NARROW_EVEN_SIGNED;
  return p;
}
// Behind a precomputed 16-bit table: the slots are folded on the GPU and the host combines the one record that is left.
WindowPlan folded_behind_table(WindowPlan p, const uint32_t* table, uint64_t stride) {
  p.table = table;
  p.table_stride = stride;
  p.records = 1;
  p.on_caller = true;
  return p;
}
// The 20-bit table (kernels/wide.hpp): `table` holds [2^(20 w)] P_i for 13 windows, the call has ONE window slot of 2^19
// buckets fed by the flat list of 13 n digits.
WindowPlan plan_wide13(const uint32_t* table, uint64_t stride) {
  WindowPlan p = folded_behind_table(plan_equal16(TE_TAIL, 1), table, stride);
  p.recode = RECODE_WIDE13;
  p.bucket_log = WIDE_LOG;
  return p;
}
WindowPlan plan_glv8(uint32_t slots = GLV_WINDOWS) {  // GLV front end: n scalars become 2 n (point, half-scalar) columns over 8 windows
  WindowPlan p = plan_equal16(XYZZ_TAIL, slots);
  p.recode = RECODE_GLV8;
  p.on_caller = true;
  return p;
}
// Scalars below 2^bits in `bytes` bytes each: short_windows(bits, L) slots recoded by k_decompose_short, on 2^11
// buckets (small inputs in the Edwards form) or 2^15.
WindowPlan plan_short(TailKind tail, uint32_t bytes, uint32_t bits, bool narrow) {
  const uint32_t L = narrow ? NARROW_LOG : (uint32_t)MSM377_WINDOW_BITS - 1;
  WindowPlan p = plan_equal16(tail, short_windows(bits, L));
  p.recode = RECODE_SHORT;
  p.bucket_log = L;
  p.short_bytes = bytes;
  p.short_bits = bits;
  return p;
}
// Whole MSMs on sixteen windows: even in the Edwards forms unless MSM377_EVEN_WINDOWS=0 (the Weierstrass forms keep equal ones).
WindowPlan plan_whole16(const msm377_ctx* ctx, TailKind tail) { return ctx->knobs.even_windows && tail != XYZZ_TAIL ? plan_even16(tail) : plan_equal16(tail); }

// This geometry refused a scalar that sixteen equal windows may still take: the pass is discarded and the call runs
// the plan next_plan names.  (A scalar that overflows the recode outright, ERR_SCALAR, fits no geometry: no rerun.)
bool geometry_refused(const WindowPlan& p, int err) {
  if (p.recode == RECODE_GLV8) return (err & ERR_GLV_RANGE) != 0;  // a half scalar of 2^127 and more
  const bool can_refuse = p.recode == RECODE_EVEN16 || p.recode == RECODE_NARROW22 || p.recode == RECODE_WIDE13;  // a scalar of 2^253 and more
  return can_refuse && (err & ERR_NARROW_RANGE) && !(err & ERR_SCALAR);
}
// Sixteen equal windows with the same kind of tail; after the wide table over its window 0, the plain affine records:
// every slot gathers from the same records, and sixteen records reach the host.
WindowPlan next_plan(const WindowPlan& refused) {
  WindowPlan p = plan_equal16(refused.tail);
  if (refused.recode == RECODE_WIDE13) p.bases_override = refused.table;
  return p;
}

// Which stages of a call to enqueue (all of them, except for the chunked host-buffer entry point), and on which windows.
struct Phase {
  bool clear_err = true;   // first chunk of a call
  bool front = true;       // decompose .. merge
  bool into = false;       // accumulate on top of the buckets of an earlier chunk
  bool back = true;        // bucket reduction, gather, D2H, completion event
  bool zc_out = false;     // the gather kernel writes the records and the error word into pinned host memory itself (k_gather_partials)
  uint64_t base_first = 0; // first record of ctx->d_bases this chunk's indices refer to
  WindowPlan plan;
};

// What the host needs of the curve policies of a pass: CV's form and buckets and records out, BP's base records in;
// quad_items: k_accumulate_quad serves the pair (TeDev on its own projective records).
struct CurveDims { int form; uint32_t bkt_words, coord_words, limbs, pt_words, out_words, rec_words; bool quad_items; };
template <class CV, class BP>
constexpr CurveDims curve_dims() {
  return {CV::FORM_ID, CV::BKT_WORDS, CV::COORD_WORDS, CV::NL, CV::PT_WORDS, CV::OUT_WORDS, BP::REC_WORDS, std::is_same<BP, CV>::value && std::is_same<CV, TeDev>::value};
}

// What ONE enqueue_windows call launches with: every size, route flag and per-slot word its stages read, derived once by
// launch_record (no HIP call) from the plan, the phase and the context's knobs; the ctx->d_* buffers are read where used.
struct LaunchRecord {
  const WindowPlan& plan;
  CurveDims cv;
  uint32_t into;               // Phase::into, as the accumulation kernels take it
  uint64_t n_scalars, n;       // scalars of the call; columns of the digit matrix (2 n_scalars behind the GLV front end)
  uint32_t wb, slots;          // windows [wb, wb + slots)
  uint32_t L, buckets, rows;   // 2^L buckets per slot, slots x buckets rows
  uint64_t entries, max_items; // (window, point) pairs this call accumulates; every row has a work item, extra ones are full segments
  uint32_t SEG;                // entries per accumulation work item
  uint32_t wc_out, pp;         // window records out (precomputed-window tables fold the windows on the GPU), points per record
  bool narrow, wide, glv, even, is_short, quad_acc, packed_sort;  // the route
  // reduction schedule: levels [0, coop_from): one thread per addition (VALU-bound: 2^18 additions per level at first);
  // [coop_from, tail_from): one lane quad per addition, one launch per level; [tail_from, L): k_reduce_tail, one launch.
  uint32_t coop_from, tail_from;
  size_t tail_lds_bytes;  // the stretch of buckets a workgroup of the tail works on
  int* d_err;            // the slot's error word ...
  uint32_t* d_partials;  // ... and partial records
  const uint32_t* bases;
  uint32_t *work_hist, *cursor, *total, *counters;  // the meta block: [work-list counters | key_max[16]]; counters: [0] split rows, [1] overflow slots
  uint32_t *key_max, *top_key_max;
};

LaunchRecord launch_record(msm377_ctx* ctx, const Phase& ph, uint64_t n_scalars, uint32_t wb, int slot, const CurveDims& cv) {
  const WindowPlan& plan = ph.plan;
  LaunchRecord k{plan, cv, ph.into ? 1u : 0u};
  k.glv = plan.recode == RECODE_GLV8, k.wide = plan.recode == RECODE_WIDE13, k.even = plan.recode == RECODE_EVEN16, k.is_short = plan.short_bytes != 0;
  k.n_scalars = n_scalars, k.n = k.glv ? 2 * n_scalars : n_scalars, k.wb = wb, k.slots = plan.slots;
  k.L = plan.bucket_log, k.buckets = 1u << k.L;  // this call's bucket geometry
  k.narrow = !k.wide && k.L != MSM377_WINDOW_BITS - 1;  // the small-input front end (k_small_sort), at full width or short
  k.entries = (k.wide ? (uint64_t)WIDE_WINDOWS : (uint64_t)k.slots) * k.n;
  // Each launch must fill the GPU on its own.  Narrow windows: a small input is all latency -- a work item is
  // a serial chain of ~10 us additions -- so its chains are cut at 8 entries (the buffers, sized for 16 windows of
  // 2^15 rows plus entries / SEG_MIN items, hold the 22 x 2^11 rows and 22 n / 8 items of an input this small easily).
  // (With the even geometry and quad-cooperative record loads in the merge, 16 entries win from 2^14 points on and 12
  // at 2^13 -- accumulate + merge 0.288 / 0.277 / 0.284 / 0.270 ms for 8 / 10 / 12 / 16 at 2^16, 0.077 / 0.077 / 0.074 /
  // 0.085 at 2^13, profiles/r03_final/sweep_narrow_seg_even.txt; below that a row has two entries on average.)
  static_assert((uint64_t)NARROW_EVEN_WINDOWS * SMALL_SORT_MAX / NARROW_SEG + NARROW_EVEN_WINDOWS * (1u << NARROW_LOG) <= (uint64_t)MSM377_NUM_WINDOWS * 32768,
                "narrow work items fit the work-item buffer");
  k.SEG = (k.narrow && !ctx->knobs.seg_plain) ? (ctx->knobs.narrow_seg ? ctx->knobs.narrow_seg : (k.n > 8192 ? 16u : 12u)) : auto_seg(ctx, k.entries, k.glv);
  k.rows = k.slots * k.buckets, k.max_items = (uint64_t)k.rows + k.entries / k.SEG;
  k.wc_out = plan.table ? 1u : k.slots, k.pp = k.wide ? WIDE_POINTS : (uint32_t)MSM377_G1_PARTIAL_POINTS;
  // a lane quad per work item while the launch is one chain's latency (up to 2^14 points: ~94 k items); beyond that
  // the quads are VALU-bound like threads and only add their exchange instructions (kernel at 2^16: 0.216 / 0.183 ms)
  k.quad_acc = cv.quad_items && k.narrow && !plan.table && k.max_items <= ctx->knobs.narrow_quad_items;
  // (One launch for the whole front end of such a call -- each window's workgroup recoding, sorting and listing its
  // work items itself, one global atomic per list and workgroup -- was built and dropped: 0.271 -> 0.293 ms at 2^12,
  // 0.342 -> 0.373 at 2^14.  Saving four dispatch latencies did not pay for a work list that is sorted by length
  // only within each window: the accumulation kernel went from 0.038 to 0.054 ms at 2^12.)
  // sort_temp elements: 8 bytes, or with MSM377_SORT_ELEM=4 packed into 4 while every column index fits 23 bits
  // (common.hpp sort_elem_bytes); the buffer is sized for 8 either way.
  k.packed_sort = !k.wide && !k.narrow && ctx->knobs.sort_elem == 4 && sort_elem_bytes(k.n, false) == 4;
  for (k.coop_from = 0; k.coop_from < k.L && 4ull * (k.coop_from + 1) * (k.buckets >> (k.coop_from + 1)) * k.wc_out > ctx->knobs.coop_threads;) k.coop_from++;
  // (wide windows: 2^19 buckets in one window -- the lists of the single-launch tail must be down to one round of
  // 128 lane quads, which is level L - 8)
  k.tail_from = std::min(k.wide ? k.L - 8 : k.narrow ? ctx->knobs.narrow_tail_from : ctx->knobs.tail_from, k.L);
  k.tail_lds_bytes = (size_t)(k.buckets >> k.tail_from) * cv.pt_words * 4;
  k.d_err = ctx->d_err + slot, k.d_partials = ctx->d_partials + (size_t)slot * SLOT_WORDS;
  const uint32_t* records = ctx->resident.valid() ? ctx->resident.bases : ctx->d_bases;  // (a twin's resident bases are lent)
  k.bases = plan.table ? plan.table : plan.bases_override ? plan.bases_override : records + ph.base_first * cv.rec_words;
  k.work_hist = ctx->d_work_meta, k.cursor = k.work_hist + SEG_BINS, k.total = k.work_hist + 2 * SEG_BINS, k.counters = k.total + 1;
  k.key_max = k.work_hist + (2 * SEG_BINS + 4);
  // The recode measures the top slot where its digits are unsigned: window 15 of the plain front end, the top slot of a
  // short call on the main path (its ranges narrowed by its largest key, win_shift).
  const bool measured = k.is_short ? !k.narrow : (!k.glv && !k.even && wb + k.slots == MSM377_NUM_WINDOWS);
  k.top_key_max = measured ? k.key_max + (k.slots - 1) : nullptr;
  return k;
}

// Stage 1: scalars -> digits, and the stage layout (msm377_g1_read_stage_ex) from the very values the launch is given,
// so that the read-back describes the kernels' arguments and not a second derivation of them.
int enqueue_decompose(msm377_ctx* ctx, const LaunchRecord& k, const uint32_t* d_scalars) {
  StageTimer t(ctx, MSM377_STAGE_DECOMPOSE, ctx->stream);
  hipStream_t st = ctx->stream;
  const dim3 grid((unsigned)((k.n_scalars + 255) / 256)), block(256);  // (one thread per scalar; n_scalars = n except behind GLV)
  // digit_key's bias per slot: k_decompose / k_decompose_glv 2^15, k_decompose_wide's BIAS, the narrow path's 2^L; the top
  // slot of a short call on the main path holds unsigned digits
  const uint32_t bias = k.wide ? 1u << WIDE_LOG : k.narrow ? k.buckets : 1u << (MSM377_WINDOW_BITS - 1);
  const uint32_t top_bias = k.is_short && !k.narrow ? 0u : bias;
  if (k.is_short) {  // k_decompose_short for the stride of the call (4, 8, 16 or 32 bytes: checked by the entry points)
    const uint32_t sb = k.plan.short_bytes;
    const auto recode = sb == 4 ? k_decompose_short<4> : sb == 8 ? k_decompose_short<8> : sb == 16 ? k_decompose_short<16> : k_decompose_short<32>;
    hipLaunchKernelGGL(recode, grid, block, 0, st, (const uint8_t*)d_scalars, ctx->d_digits, k.n, k.plan.short_bits, k.L, k.slots, bias, top_bias, k.d_err, k.top_key_max);
  } else if (k.wide)
    hipLaunchKernelGGL(k_decompose_wide, grid, block, 0, st, d_scalars, ctx->wide.digits, k.n, k.d_err);
  else if (k.narrow)
    hipLaunchKernelGGL(k_decompose_geom, grid, block, 0, st, d_scalars, ctx->d_digits, k.n, k.L, NARROW_EVEN_SIGNED, k.slots, bias, k.d_err);
  else if (k.glv)
    hipLaunchKernelGGL(k_decompose_glv, grid, block, 0, st, d_scalars, ctx->d_digits, k.n_scalars, k.wb, k.slots, k.d_err);
  else
    hipLaunchKernelGGL(k_decompose, grid, block, 0, st, d_scalars, ctx->d_digits, k.n, k.wb, k.slots, k.d_err, k.top_key_max, k.even ? 1u : 0u);
  HIP_TRY(ctx, hipGetLastError());
  static_assert(MAX_WINDOW_SLOTS <= MSM377_STAGE_MAX_SLOTS, "a stage layout names every window slot");
  msm377_stage_info& info = ctx->last.stage.info = msm377_stage_info{};
  info.slots = k.slots, info.bucket_log = k.L;
  info.columns = k.entries / k.slots;  // n; 2 n_scalars behind the GLV front end; 13 n in the one slot of the wide table
  info.digit_bytes = k.wide ? 4u : 2u;
  info.row_ptr_len = k.buckets + 2, info.bucket_records = k.buckets;
  info.form = k.cv.form, info.table_stride = k.plan.table_stride, info.geometry_reruns = ctx->fallback.geometry_reruns;
  for (uint32_t s = 0; s < k.slots; s++) info.bias[s] = s + 1 < k.slots ? bias : top_bias;
  if (k.is_short && !k.narrow) info.key_unsigned[k.slots - 1] = 1u;  // (KEY_UNSIGNED in that slot's key_max word)
  ctx->last.stage.d_digits = k.wide ? (const void*)ctx->wide.digits : (const void*)ctx->d_digits;
  ctx->last.stage.d_key_max = (k.wide || k.narrow) ? nullptr : k.key_max;  // k_local_sort_lds of the wide table and k_small_sort read none
  ctx->last.stage.coord_words = k.cv.coord_words, ctx->last.stage.limbs = k.cv.limbs;  // the bucket records of the pass: four slots of coord_words, `limbs` used
  return MSM377_OK;
}

// Stage 2: digits -> CSR (row_ptr, val_idx) per window slot.
int enqueue_sort(msm377_ctx* ctx, const LaunchRecord& k) {
  StageTimer t(ctx, MSM377_STAGE_SORT, ctx->stream);
  hipStream_t st = ctx->stream;
  if (k.wide) {  // the 13 n entries into 4096 fine ranges: two staged partition passes per window (kernels/wide.hpp), then k_local_sort_lds
    uint32_t* counts = ctx->wide.counts;
    ctx->last.sort_elem = sort_elem_bytes(k.entries, true);
    hipLaunchKernelGGL(k_wide_count, dim3(WS_CHUNKS, WIDE_WINDOWS), dim3(1024), 0, st, (const uint32_t*)ctx->wide.digits, counts, k.n);
    hipLaunchKernelGGL(k_wide_sums, dim3(WIDE_NRANGE / 256, WIDE_WINDOWS), dim3(256), 0, st, counts);
    hipLaunchKernelGGL(k_wide_scan, dim3(1), dim3(1024), 0, st, counts, ctx->d_region_base);
    hipLaunchKernelGGL(k_wide_offsets1, dim3(WIDE_WINDOWS), dim3(WS_COARSE), 0, st, counts, k.n);
    hipLaunchKernelGGL(k_wide_part1, dim3(WS_CHUNKS, WIDE_WINDOWS), dim3(1024), 0, st, (const uint32_t*)ctx->wide.digits, (const uint32_t*)counts, ctx->d_sort_temp, k.n, (uint32_t)k.plan.table_stride);
    hipLaunchKernelGGL(k_wide_part2, dim3(WS_COARSE, WIDE_WINDOWS), dim3(1024), 0, st, (const SortElem*)ctx->d_sort_temp, (const uint32_t*)counts, ctx->wide.temp);
    hipLaunchKernelGGL(k_local_sort_lds<SortElem>, dim3(WIDE_NRANGE, 1), dim3(256), 0, st, (const SortElem*)ctx->wide.temp, ctx->d_region_base, ctx->d_row_ptr, ctx->d_val_idx,
                       k.entries, (const uint32_t*)nullptr, WIDE_NRANGE, k.buckets);
    HIP_TRY(ctx, hipGetLastError());
  } else if (k.narrow) {
    ctx->last.sort_elem = 0;
    hipLaunchKernelGGL(k_small_sort, dim3(k.slots), dim3(1024), 0, st, ctx->d_digits, ctx->d_row_ptr, ctx->d_val_idx, (uint32_t)k.n, k.L);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    uint32_t chunks = MAX_SORT_BLOCKS / k.slots;
    const uint64_t want = (k.n + 4095) / 4096;  // at least ~4096 elements per block
    if (chunks > want) chunks = (uint32_t)(want ? want : 1);
    const uint64_t per_chunk = (k.n + chunks - 1) / chunks;
    const dim3 grid(chunks, k.slots);
    // (is_short: the top slot holds unsigned digits, KEY_UNSIGNED)
    hipLaunchKernelGGL(k.is_short ? k_range_count<true> : k_range_count<false>, grid, dim3(1024), 0, st, ctx->d_digits, ctx->d_range_counts, k.n, chunks, per_chunk, k.key_max);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_range_scan, dim3(k.slots), dim3(NRANGE), 0, st, ctx->d_range_counts, ctx->d_region_base, chunks);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last.sort_elem = k.packed_sort ? 4u : 8u;
    auto partition_and_sort = [&](auto* temp) {
      using E = std::remove_pointer_t<decltype(temp)>;
      hipLaunchKernelGGL((k.is_short ? k_partition_staged<E, true> : k_partition_staged<E, false>), grid, dim3(1024), 0, st, ctx->d_digits, ctx->d_range_counts, temp, k.n, chunks,
                         per_chunk, k.key_max);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_local_sort_lds<E>, dim3(NRANGE, k.slots), dim3(256), 0, st, (const E*)temp, ctx->d_region_base, ctx->d_row_ptr, ctx->d_val_idx, k.n, k.key_max, NRANGE,
                         k.buckets);
      return hipGetLastError();
    };
    HIP_TRY(ctx, k.packed_sort ? partition_and_sort(reinterpret_cast<SortElem4*>(ctx->d_sort_temp)) : partition_and_sort(ctx->d_sort_temp));
  }
  return MSM377_OK;
}

// The accumulation launch of stage 3: a thread per work item, or (quad_acc) a lane quad.
template <class CV, class BP>
void launch_accumulate(msm377_ctx* ctx, const LaunchRecord& k) {
  StageTimer tk(ctx, MSM377_STAGE_ACC_KERNEL, ctx->stream);
  hipStream_t st = ctx->stream;
  if constexpr (curve_dims<CV, BP>().quad_items) {
    if (k.quad_acc) {
      hipLaunchKernelGGL(k_accumulate_quad<CV>, dim3((unsigned)((4 * k.max_items + 255) / 256)), dim3(256), 0, st, ctx->d_row_ptr, ctx->d_val_idx, k.bases, ctx->d_buckets, k.n,
                         ctx->d_work, k.total, ctx->d_row_ovf_base, ctx->d_ovf, k.SEG, k.d_err, ctx->d_err + 2, k.into, k.L);
      return;
    }
  }
  hipLaunchKernelGGL((k_accumulate<CV, 2, BP>), dim3((unsigned)((k.max_items + 255) / 256)), dim3(256), 0, st, ctx->d_row_ptr, ctx->d_val_idx, k.bases, ctx->d_buckets, k.n,
                     ctx->d_work, k.total, ctx->d_row_ovf_base, ctx->d_ovf, k.SEG, k.d_err, ctx->d_err + 2, k.into, k.plan.table_stride, k.L);
}

// Stage 3: work list, accumulation, merge of split rows.  The before_accumulate hook (the host-buffer entry points: join
// the point upload, launch the base conversion) is swapped out of the context and called once k_work_scatter is queued
// and BEFORE the wait for bases_ready is queued: the wait binds to the event's latest record.
template <class CV, class BP>
int enqueue_accumulate(msm377_ctx* ctx, const LaunchRecord& k) {
  StageTimer t(ctx, MSM377_STAGE_ACCUMULATE, ctx->stream);
  hipStream_t st = ctx->stream;
  const dim3 row_grid((k.rows + 1023) / 1024);
  hipLaunchKernelGGL(k_work_hist, row_grid, dim3(1024), 0, st, ctx->d_row_ptr, k.L, k.rows, k.SEG, k.work_hist, ctx->d_row_ovf_base, k.counters, ctx->d_split_rows);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_work_scatter, row_grid, dim3(1024), 0, st, ctx->d_row_ptr, k.L, k.rows, k.SEG, (const uint32_t*)k.work_hist, k.cursor, k.total, ctx->d_work);
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->before_accumulate) {
    std::function<int()> f;
    f.swap(ctx->before_accumulate);
    const int hook_rc = f();
    if (hook_rc) return hook_rc;
  }
  HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->bases_ready, 0));
  ctx->last.products = BP::MADD_PRODUCTS;
  launch_accumulate<CV, BP>(ctx, k);
  HIP_TRY(ctx, hipGetLastError());
  ctx->zc.acc_seq++;
  int32_t fold_slot = -1;  // the slot k_fold_long_rows is launched on (msm377_g1_read_work_list)
  if (k.is_short) {  // the top window of a short call: few rows, thousands of partials each -- folded before the merge
    hipLaunchKernelGGL(k_fold_long_rows<CV>, dim3(FOLD_BLOCKS), dim3(FOLD_THREADS), 0, st, ctx->d_row_ptr, ctx->d_row_ovf_base, ctx->d_ovf, k.SEG, k.d_err, k.L, k.slots - 1);
    HIP_TRY(ctx, hipGetLastError());
    fold_slot = (int32_t)(k.slots - 1);
  }
  // (grid-stride over the split-row list: with the even windows few rows split, and 8192 workgroups that only read the
  // count cost 11 us at 2^20)
  hipLaunchKernelGGL(k_merge_split_rows_quad<CV>, dim3(std::min<uint32_t>((k.rows + 63) / 64, 1024u)), dim3(256), 0, st, ctx->d_row_ptr, ctx->d_buckets, k.counters,
                     ctx->d_split_rows, ctx->d_row_ovf_base, ctx->d_ovf, k.SEG, k.d_err, k.L, ctx->zc.dm_flag + ACC_FLAG_WORD, ctx->zc.acc_seq);
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->capture) {  // the work list of the pass (msm377_g1_read_work_list), from the arguments of the launches above
    WorkListLayout& wl = ctx->last.work;
    msm377_work_list_info& wi = wl.info = msm377_work_list_info{};
    wi.seg = k.SEG, wi.rows = k.rows, wi.max_items = k.max_items, wi.quad = k.quad_acc ? 1u : 0u;
    wi.fold_slot = fold_slot;
    wi.record_words = 4 * k.cv.limbs, wi.form = k.cv.form, wi.bucket_log = k.L;
    wl.bkt_words = k.cv.bkt_words, wl.coord_words = k.cv.coord_words, wl.limbs = k.cv.limbs;
    wl.d_hist = k.work_hist, wl.d_total = k.total, wl.d_counters = k.counters;
    wl.valid = true;
  }
  return MSM377_OK;
}

// Stage 4: bucket reduction (schedule: LaunchRecord::coop_from / tail_from) and the gather of the window records.
// (Fusing pairs of thread-level levels -- four buckets a quarter-list apart per thread, four additions, three
// stores -- halves their HBM traffic and was slower all the same: reduce 0.290 -> 0.310 ms at 2^20, 0.278 -> 0.296
// at 2^16.  The first levels are VALU-bound at two waves per SIMD, the later ones cost one addition's latency
// per launch; a thread with four serial additions only lengthens that.)
// More waves do not help either: k_tree_step at 3 / 4 waves per SIMD (132 VGPRs, no scratch) reduces in 0.300 /
// 0.32 ms against 0.298 at 2; lane quads for levels 0-4 (MSM377_COOP_THREADS up to 2^20 threads) in 0.36.
// What does help is not going through memory between the levels at all: the levels below tail_from run as column
// launches of up to four levels each (k_tree_columns: 0-3 and 4-6 on the main path, 0-3 on the narrow one, 0-3,
// 4-7, 8-10 for a wide window), every geometry and window count alike.  coop_from does not choose their kernel any more;
// it only tells them from which level on the per-level launches add empty buckets like any other (k_tree_step_quad),
// so that both give the same records.  MSM377_REDUCE_COLUMNS=0: one launch per level.
template <class CV>
int enqueue_reduce(msm377_ctx* ctx, const LaunchRecord& k) {
  static_assert(CV::HAS_QUAD, "every curve policy has the quad-cooperative addition");
  StageTimer t(ctx, MSM377_STAGE_REDUCE, ctx->stream);
  hipStream_t st = ctx->stream;
  // behind a table, slots [half, m) onto [0, m - half): 16 -> 8 -> 4 -> 2 -> 1; a short call folds any count
  for (uint32_t m = k.plan.table ? k.slots : 1; m > 1;) {
    const uint32_t half = (m + 1) / 2, count = m - half;
    hipLaunchKernelGGL(k_fold_windows<CV>, dim3(count * k.buckets / 256), dim3(256), 0, st, ctx->d_buckets, k.L, half, count, k.d_err);
    HIP_TRY(ctx, hipGetLastError());
    m = half;
  }
  const bool columns = ctx->knobs.reduce_columns != 0;
  bool tail_in_lds = false;
  uint32_t r = 0;
  while (columns && r < k.tail_from) {
    const uint32_t levels = std::min(k.tail_from - r, COLUMN_LEVELS_MAX);
    const uint32_t threads = (r + 1) * (k.buckets >> (r + 1));  // per window: (r + 1) arrays x (buckets >> (r + levels)) columns x 2^(levels-1) lanes
    hipLaunchKernelGGL(k_tree_columns<CV>, dim3((threads + 255) / 256, k.wc_out), dim3(256), 0, st, ctx->d_buckets, k.L, r, levels, k.coop_from, threads, k.d_err);
    HIP_TRY(ctx, hipGetLastError());
    r += levels;
  }
  for (; r < k.tail_from; r++) {
    const uint32_t ops = (r + 1) * (k.buckets >> (r + 1));
    if (r >= k.coop_from)
      hipLaunchKernelGGL(k_tree_step_quad<CV>, dim3((4 * ops + 255) / 256, k.wc_out), dim3(256), 0, st, ctx->d_buckets, k.L, r, ops, k.d_err);
    else
      hipLaunchKernelGGL(k_tree_step<CV>, dim3((ops + 255) / 256, k.wc_out), dim3(256), 0, st, ctx->d_buckets, k.L, r, ops, k.d_err);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (k.tail_from < k.L) {
    const bool in_lds = tail_in_lds = ctx->knobs.tail_lds && k.tail_lds_bytes <= TAIL_LDS_BYTES_MAX;
    if (in_lds && k.tail_lds_bytes > 64 * 1024)  // (only with MSM377_TAIL_FROM below its default; per device, so every time)
      HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_reduce_tail_lds<CV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TAIL_LDS_BYTES_MAX));
    if (in_lds)
      hipLaunchKernelGGL(k_reduce_tail_lds<CV>, dim3(k.tail_from + 1, k.wc_out), dim3(TAIL_THREADS), k.tail_lds_bytes, st, ctx->d_buckets, k.L, k.tail_from, k.d_err);
    else
      hipLaunchKernelGGL(k_reduce_tail<CV>, dim3(k.tail_from + 1, k.wc_out), dim3(TAIL_THREADS), 0, st, ctx->d_buckets, k.L, k.tail_from, k.d_err);
    HIP_TRY(ctx, hipGetLastError());
  }
  // Zero-copy output: the kernel writes the records and the error word into pinned host memory itself and publishes out_seq.
  const bool zc = ctx->zc.active;
  hipLaunchKernelGGL(k_gather_partials<CV>, dim3((k.wc_out * k.pp * 4 + 63) / 64), dim3(64), 0, st, ctx->d_buckets, k.d_partials, k.wc_out, k.L, zc ? ctx->zc.dm_partials : nullptr,
                     zc ? ctx->zc.dm_flag : nullptr, zc ? ctx->zc.d_count : nullptr, zc ? (const int*)k.d_err : nullptr, zc ? ctx->zc.out_seq : 0u, k.pp);
  HIP_TRY(ctx, hipGetLastError());
  // The records of the pass (msm377_g1_read_partials), from the arguments of the launches above and the plan run_tail takes.
  msm377_partials_info& pi = ctx->last.stage.partials = msm377_partials_info{};
  pi.records = k.wc_out, pi.points = k.pp, pi.planes = k.L, pi.coord_words = k.cv.out_words / 4, pi.form = k.cv.form;
  pi.folded_slots = k.plan.table ? k.slots : 1u;
  pi.tail_kind = (uint32_t)k.plan.tail, pi.tail_windows = (uint32_t)k.plan.records, pi.tail_cbits = (uint32_t)k.plan.cbits(), pi.tail_planes = (uint32_t)k.plan.planes();
  pi.tail_short_from = (uint32_t)k.plan.short_from;
  pi.coop_from = k.coop_from, pi.tail_from = k.tail_from, pi.columns = columns ? 1u : 0u, pi.tail_lds = tail_in_lds ? 1u : 0u;
  ctx->last.stage.d_partials = k.d_partials;
  return MSM377_OK;
}

// Enqueue stages decompose .. gather for windows [wb, wb + plan.slots) against ctx->d_bases on the main stream, the D2H
// of the partial records into slot `slot` of ctx->h_partials (unless the gather kernel delivered them) and that slot's
// completion event: one LaunchRecord, then the stage functions above in order.  Nothing here waits for the GPU.
// (Rounds 1 and 2 could run a large call as TWO parts of half the windows on two streams, so that one part's sort and
// reduction hid under the other's accumulation: 3.19 vs 3.17 ms at 2^20, then 2.72 -> 2.89 on round 2's kernels -- the
// accumulation kernel owns every VGPR of the chip, kernels of another stream do not become co-resident.  Removed in
// round 3.)
template <class CV, class BP = CV>
int enqueue_windows(msm377_ctx* ctx, const uint32_t* d_scalars, uint64_t n_scalars, uint32_t wb, int slot, const Phase& ph) {
  const LaunchRecord k = launch_record(ctx, ph, n_scalars, wb, slot, curve_dims<CV, BP>());
  hipStream_t st = ctx->stream;
  ctx->last.stage.valid = false;  // set again at the end of a whole call under stage capture
  ctx->zc.active = ph.zc_out && ph.back && ctx->knobs.zc_out && slot == 0 && !k.plan.table;
  if (ctx->zc.active) ctx->zc.out_seq++;
  // The error word is cleared by the call's first kernel: with the front stages one launch clears the call's work-list
  // counters, its key_max words (0 = full-width ranges; the recode then measures the top slot) and the error word.
  if (ph.front) {
    hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, st, k.work_hist, META_BLOCK_WORDS, (uint32_t*)k.d_err, ph.clear_err ? 1u : 0u);
    int rc = enqueue_decompose(ctx, k, d_scalars);
    if (rc == MSM377_OK) rc = enqueue_sort(ctx, k);
    if (rc == MSM377_OK) rc = enqueue_accumulate<CV, BP>(ctx, k);
    if (rc) return rc;
  } else if (ph.clear_err)
    hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, st, (uint32_t*)k.d_err, 1u, (uint32_t*)nullptr, 0u);
  if (!ph.back) return MSM377_OK;
  if (ctx->capture) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_buckets_snap, ctx->d_buckets, (size_t)k.slots * k.cv.bkt_words * k.buckets * 4, hipMemcpyDeviceToDevice, st));
  const int rc = enqueue_reduce<CV>(ctx, k);
  if (rc) return rc;
  if (!ctx->zc.active) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_partials + (size_t)slot * SLOT_WORDS, k.d_partials, (size_t)k.wc_out * k.pp * k.cv.out_words * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_err + slot, k.d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->done_ev[slot], st));
  ctx->last.n = k.n, ctx->last.glv = k.glv, ctx->last.form = k.cv.form;
  ctx->last.geom_windows = k.slots, ctx->last.geom_log = k.L;
  // A whole call in one piece from window 0: the layout written at the decomposition describes it.  Capture mode 1 is G1's:
  // an Edwards-BLS12 call is described as run only (mode 2).
  ctx->last.stage.valid = ctx->capture && ph.front && !ph.into && wb == 0 && (k.cv.form != MSM377_STAGE_FORM_ED || ctx->capture == 2);
  return MSM377_OK;
}

// Zero-copy output (Phase::zc_out, slot 0): poll the sequence number the gather kernel's last block writes behind the records;
// the stream's completion event is waited for only when stage timing needs it (or after 50 ms without the flag, which
// then also surfaces a failed kernel).
int wait_zero_copy_out(msm377_ctx* ctx) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 0; __atomic_load_n(&ctx->zc.h_flag[0], __ATOMIC_ACQUIRE) != ctx->zc.out_seq; spins++) {
    __builtin_ia32_pause();
    if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) {
      HIP_TRY(ctx, hipEventSynchronize(ctx->done_ev[0]));
      break;
    }
  }
  if (__atomic_load_n(&ctx->zc.h_flag[0], __ATOMIC_ACQUIRE) != ctx->zc.out_seq) {
    ctx->err = "zero-copy output: the window records did not arrive";
    return MSM377_EHIP;
  }
  ctx->h_err[0] = (int)__atomic_load_n(&ctx->zc.h_flag[1], __ATOMIC_RELAXED);
  return MSM377_OK;
}

// Wait for slot `slot`: its error word is then in ctx->h_err[slot], its records in ctx->h_partials + slot * SLOT_WORDS.
int wait_windows(msm377_ctx* ctx, int slot) {
  if (ctx->zc.active && slot == 0) {
    const int rc = wait_zero_copy_out(ctx);
    if (rc || !ctx->timing) return rc;
  }
  HIP_TRY(ctx, hipEventSynchronize(ctx->done_ev[slot]));
  return MSM377_OK;
}

// Behind wait_windows, once the caller has decided to keep the pass: the stage times, and the one error no geometry helps.
int collect_windows(msm377_ctx* ctx, int slot) {
  if (ctx->timing) {
    for (int s = 0; s < MSM377_NUM_STAGES; s++) {
      if (s == MSM377_STAGE_TAIL) continue;  // host wall time, set by run_tail
      if (ctx->timing == 2 && s != MSM377_STAGE_ACC_KERNEL) {
        ctx->last.stage_ms[s] = 0.0;
        continue;
      }
      float ms = 0.f;
      ctx->last.stage_ms[s] = hipEventElapsedTime(&ms, ctx->ev[s][0], ctx->ev[s][1]) == hipSuccess ? ms : 0.0;
    }
    (void)hipGetLastError();  // a stage that did not run in this call must not leave its error for the next launch check
  }
  if (ctx->h_err[slot] & ERR_SCALAR) {
    ctx->err = "a scalar overflows the signed 16-bit window recode (final carry)";
    return MSM377_ESCALAR;
  }
  return MSM377_OK;
}

inline bool use_glv(const msm377_ctx* ctx) { return ctx->knobs.glv_mode == 1; }  // see Knobs::glv_mode

// Base conversion for the G1 entry points: with the GLV front end the table also gets phi(P_i).
int convert_bases_g1(msm377_ctx* ctx, const uint32_t* d_raw, uint64_t n, bool glv) {
  if (!glv) return convert_bases<G1Dev>(ctx, d_raw, n);
  if (n == 0) return MSM377_OK;
  if (ctx->timing == 1) (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][0], ctx->stream2);
  hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, ctx->stream2, (uint32_t*)(ctx->d_err + 2), 1u, (uint32_t*)nullptr, 0u);
  hipLaunchKernelGGL(k_convert_bases_glv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream2, d_raw, ctx->d_bases, n);
  HIP_TRY(ctx, hipGetLastError());
  note_bases(ctx, MSM377_BASES_WEIERSTRASS, ctx->d_bases, n, 0, true);
  if (ctx->timing == 1) (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][1], ctx->stream2);
  HIP_TRY(ctx, hipEventRecord(ctx->bases_ready, ctx->stream2));
  return MSM377_OK;
}

// What ctx->d_bases holds for the G1 entry points.
enum TableForm { TABLE_XYZZ = 0, TABLE_XYZZ_GLV = 1, TABLE_TE = 2, TABLE_TE_AFFINE = 3, TABLE_TE_PRECOMP = 4 };
inline bool form_is_te(int form) { return form == TABLE_TE || form == TABLE_TE_AFFINE || form == TABLE_TE_PRECOMP; }
constexpr int RC_TE_FALLBACK = 1;  // internal: an exceptional case of the twisted Edwards law, rerun on the Weierstrass path

// A prefix of a GLV table (records 0..n-1 = the plain points) serves the plain path; the phi half needs all of it.
inline int resident_form(const msm377_ctx* ctx, uint64_t n) {
  return (ctx->resident.form == TABLE_XYZZ_GLV && n != ctx->resident.n) ? TABLE_XYZZ : ctx->resident.form;
}
// The resident table is the 20-bit-window one: 13 windows over one set of 2^19 buckets.
inline bool wide_table(const ResidentBases& r) { return r.form == TABLE_TE_PRECOMP && r.windows == WIDE_WINDOWS; }
inline int weierstrass_form(const msm377_ctx* ctx) { return use_glv(ctx) ? TABLE_XYZZ_GLV : TABLE_XYZZ; }
inline int pick_form(const msm377_ctx* ctx) { return ctx->knobs.g1_form == 1 ? TABLE_TE : weierstrass_form(ctx); }

int convert_table(msm377_ctx* ctx, const uint32_t* d_raw, uint64_t n, int form) {
  if (form == TABLE_TE) return convert_bases<TeDev>(ctx, d_raw, n);
  if (form == TABLE_TE_AFFINE) {  // resident tables: both phases back to back (the caller waits for the side stream anyway)
    const int rc = affine_convert_begin(ctx, d_raw, n);
    return rc ? rc : affine_convert_finish(ctx, ctx->d_bases, n);
  }
  return convert_bases_g1(ctx, d_raw, n, form == TABLE_XYZZ_GLV);
}

// The host tail `plan` names over the window records at `partials`, timed into stage_ms[MSM377_STAGE_TAIL].
// RC_TE_FALLBACK (noted): the Edwards tail hit an exceptional case, out_xy is untouched.
int run_tail(msm377_ctx* ctx, const WindowPlan& plan, const uint32_t* partials, uint8_t* out_xy) {
  const auto t0 = std::chrono::steady_clock::now();
  int tr = TAIL_OK;
  if (plan.tail == ED_TAIL)
    tr = ed_tail(ctx, partials, out_xy, plan.short_from);
  else if (plan.tail == XYZZ_TAIL && plan.on_caller)
    g1h_combine(partials, plan.records, out_xy, plan.short_from);
  else if (plan.tail == XYZZ_TAIL)
    tr = xyzz_tail(ctx, partials, out_xy, plan.short_from, plan.records);
  else if (plan.on_caller)
    tr = teh_combine(partials, plan.records, out_xy, plan.cbits(), plan.planes(), plan.short_from) ? TAIL_EXCEPTIONAL : TAIL_OK;
  else
    tr = te_tail(ctx, partials, out_xy, plan.records, plan.cbits(), plan.planes(), plan.short_from);
  ctx->last.stage_ms[MSM377_STAGE_TAIL] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (tr != TAIL_EXCEPTIONAL) return tr;
  note_fallback(ctx, MSM377_FB_TAIL);
  return RC_TE_FALLBACK;
}

// Arms the tail workers of one call once its accumulation kernel is through (TailPool::prewake: they poll for their
// jobs while the GPU reduces the buckets); disarmed when the tail is done.
struct TailArm {
  msm377_ctx* c;
  bool armed = false;
  explicit TailArm(msm377_ctx* ctx) : c(ctx) {}
  void arm() {
    if (armed || c->knobs.tail_threads <= 1 || c->knobs.tail_spin_us <= 0) return;
    armed = true;
    c->tail_pool.prewake(c->knobs.tail_spin_us, std::min(c->knobs.tail_threads, TailPool::WORKERS + 1) - 1);
  }
  // A small input is over in a few hundred microseconds, its bucket reduction in 0.1 ms -- no longer than a sleeping
  // worker may take to come back -- so its call arms the workers before it enqueues anything.
  void at_start(uint64_t n) {
    if (n <= (1ull << 17)) arm();
  }
  void after_accumulation() {
    if (armed || c->knobs.tail_threads <= 1 || c->knobs.tail_spin_us <= 0) return;
    // k_merge_split_rows_quad, the launch behind the accumulation kernel, writes the call's sequence number; without it
    // within 100 ms the caller's own wait reports whatever went wrong
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; __atomic_load_n(&c->zc.h_flag[ACC_FLAG_WORD], __ATOMIC_ACQUIRE) != c->zc.acc_seq; spins++) {
      __builtin_ia32_pause();
      if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(100)) return;
    }
    arm();
  }
  ~TailArm() { c->tail_pool.disarm(); }
};

// enqueue_windows for the records of a table form, from window 0.
int enqueue_form(msm377_ctx* ctx, int form, const uint32_t* d_scalars, uint64_t n, int slot, const Phase& ph) {
  if (form == TABLE_TE) return enqueue_windows<TeDev>(ctx, d_scalars, n, 0, slot, ph);
  if (form_is_te(form)) return enqueue_windows<TeDev, TeAffBase>(ctx, d_scalars, n, 0, slot, ph);
  return enqueue_windows<G1Dev>(ctx, d_scalars, n, 0, slot, ph);
}

// The first plan of a G1 MSM of n scalars on records of `form`.  sbytes = 0: 32-byte scalars of any width; else scalars
// of sbytes bytes below 2^bits (never even, never behind the GLV front end: a GLV table serves through its plain half).
WindowPlan first_plan(const msm377_ctx* ctx, uint64_t n, int form, uint32_t sbytes, uint32_t bits) {
  if (!form_is_te(form)) return sbytes ? plan_short(XYZZ_TAIL, sbytes, bits, false) : form == TABLE_XYZZ_GLV ? plan_glv8() : plan_equal16(XYZZ_TAIL);
  const ResidentBases& r = ctx->resident;
  // Small inputs: narrow windows; the window-indexed buffers are sized for them too (context.hip ctx_create: wcap).  A
  // precomputed table has its own geometry, and capture mode 1 describes sixteen equal 16-bit windows.
  const bool precomp = form == TABLE_TE_PRECOMP;
  const bool narrow = !precomp && n <= ctx->knobs.narrow_max_points && n <= SMALL_SORT_MAX && ctx->capture != 1;
  if (sbytes) {
    WindowPlan p = plan_short(TE_TAIL, sbytes, bits, narrow);
    if (precomp && wide_table(r))
      p.bases_override = r.table;  // the 20-bit table serves through its window 0, the plain affine records
    else if (precomp)
      p = folded_behind_table(p, r.table, r.n);
    return p;
  }
  if (precomp) return wide_table(r) ? plan_wide13(r.table, r.n) : folded_behind_table(plan_equal16(TE_TAIL), r.table, r.n);
  if (narrow) return plan_narrow22();  // (whatever MSM377_EVEN_WINDOWS says)
  return ctx->capture == 1 ? plan_equal16(TE_TAIL) : plan_whole16(ctx, TE_TAIL);
}

int short_width_error(msm377_ctx* ctx, uint32_t bits) {
  ctx->err = "a scalar does not fit the declared width of " + std::to_string(bits) + " bits (scalar_bits)";
  return MSM377_ESCALAR;
}

// G1 MSM of n scalars against the base records in form `form` (ctx->d_bases or the resident table; already converted or
// being converted on the side stream).  A geometry that refuses a scalar hands the call to the next one (each refusal
// counts one geometry rerun); a short call (sbytes != 0) runs ONE pass: a scalar of 2^bits or more is the caller's
// error (MSM377_ESCALAR, out_xy untouched), not a reason to rerun at full width.  RC_TE_FALLBACK: an addition or an
// input point hit an exceptional case of the Edwards law (the caller reconverts to TABLE_XYZZ and calls again).
// Zero-copy output and the early arming of the tail workers belong to the Edwards forms.
int g1_table_msm(msm377_ctx* ctx, const uint32_t* d_scalars, uint64_t n, int form, uint8_t out_xy[96], uint32_t sbytes = 0, uint32_t bits = 0) {
  const bool te = form_is_te(form);
  TailArm arm(ctx);
  arm.at_start(n);
  Phase ph;
  ph.zc_out = te;
  ph.plan = first_plan(ctx, n, form, sbytes, bits);
  for (;;) {
    int rc = enqueue_form(ctx, form, d_scalars, n, 0, ph);
    if (rc) return rc;
    if (te) arm.after_accumulation();
    rc = wait_windows(ctx, 0);
    if (rc) return rc;
    const int err = ctx->h_err[0];
    if (geometry_refused(ph.plan, err)) {
      ctx->fallback.geometry_reruns++;
      ph.plan = next_plan(ph.plan);
      continue;
    }
    if (sbytes && (err & ERR_SHORT_WIDTH)) return short_width_error(ctx, bits);
    if (te && (err & ERR_TE_ANY)) {
      note_fallback(ctx, (uint32_t)(err & ERR_TE_ANY));
      return RC_TE_FALLBACK;
    }
    rc = collect_windows(ctx, 0);
    if (rc) return rc;
    return run_tail(ctx, ph.plan, ctx->h_partials, out_xy);
  }
}

// The resident table hit an exceptional case of the Edwards law: rebuild it in Weierstrass form from the raw
// copy kept by msm377_g1_set_bases_device.  Nothing is resident if that fails.
int resident_table_to_weierstrass(msm377_ctx* ctx) {
  const int form = TABLE_XYZZ;  // points outside the prime-order subgroup: never the GLV front end
  const uint64_t n = ctx->resident.n;
  const uint32_t flagged = ctx->resident.flagged;  // the mask describes the raw copy, whatever form its records take
  const uint32_t* mask = ctx->resident.inf_mask;
  ctx->resident.clear();
  ctx->last.bases.valid = false;  // the records are being overwritten: described again once the rebuild is through
  int rc = convert_table(ctx, ctx->d_raw_points, n, form);
  ctx->last.bases.valid = false;
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
  ctx->resident.set(ctx->d_bases, n, form, flagged, mask);
  ctx->last.bases.info.flagged = flagged;  // the set's own count: the input form may have changed since the set was imported
  ctx->last.bases.d_flagged = nullptr;
  ctx->last.bases.valid = true;
  return MSM377_OK;
}

// scalar_bytes in {4, 8, 16, 32}, 1 <= scalar_bits <= min(8 scalar_bytes, 253) (include/msm377.h).
int check_short_args(msm377_ctx* ctx, uint32_t sbytes, uint32_t bits) {
  if (sbytes != 4 && sbytes != 8 && sbytes != 16 && sbytes != 32) {
    ctx->err = "scalar_bytes must be 4, 8, 16 or 32";
    return MSM377_EINVAL;
  }
  if (bits < 1 || bits > 8 * sbytes || bits > 253) {
    ctx->err = "scalar_bits must be between 1 and min(8 scalar_bytes, 253)";
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

// Host-buffer entry points with large inputs: the upload (3.0-3.6 ms for the 128 MB of a 2^20-point G1 input from
// pageable memory, box to box) is longer than the whole computation, so the two overlap: the MSM runs as K chunks of
// points, later chunks accumulate on top of the buckets the earlier ones left (Phase::into), reduction, gather and D2H
// are queued once, with the last chunk.  A chunk's scalars AND points go up together and the chunk runs the whole front
// end -- decompose .. accumulate .. merge -- while the next one is on its way.  (Sorting all scalars once and
// accumulating each chunk through its own sub-rows was built, passed and measured slower: HISTORY.md, "Sort-once
// schedule".)
// Every chunk runs `plan` (g1_msm / ed_msm: the even geometry in the Edwards forms; they rerun in one piece when a scalar
// does not fit it) and the last one queues the back phase; the caller waits, classifies and runs the plan's tail.
template <class CV>
int run_chunked_upload(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, const WindowPlan& plan) {
  constexpr size_t PB = CV::RAW_WORDS * 4;  // bytes per wire point
  uint64_t cut[10];  // chunk c = points [cut[c], cut[c + 1]): the first one upload_split_pct of n, the rest even
  uint32_t K = 0;
  cut[0] = 0;
  for (uint32_t c = 1; c < ctx->knobs.upload_chunks; c++) {
    const uint64_t first_end = std::max<uint64_t>(64, (n * ctx->knobs.upload_split_pct / 100) & ~63ull);
    const uint64_t b = c == 1 ? first_end : (first_end + (n - first_end) * (c - 1) / (ctx->knobs.upload_chunks - 1)) & ~63ull;
    if (b > cut[K] && b < n) cut[++K] = b;  // no empty chunks (small n)
  }
  cut[++K] = n;
  const size_t sc_stage = (size_t)ctx->cap * 96;
  auto upload_chunk = [&](uint32_t c, HipFail* fail) -> int {
    const uint64_t first = cut[c], cnt = cut[c + 1] - cut[c];
    int r = h2d_staged(ctx, (uint8_t*)ctx->d_raw_scalars + first * 32, scalars + first * 32, cnt * 32, sc_stage + first * 32, fail);
    if (r == MSM377_OK) r = h2d_staged(ctx, (uint8_t*)ctx->d_raw_points + first * PB, points + first * PB, cnt * PB, first * PB, fail);
    return r;
  };
  int rc = upload_chunk(0, nullptr);
  if (rc) return rc;
  int up_rc = MSM377_OK;
  HipFail up_fail;
  std::atomic<uint32_t> uploaded{1};  // chunks on the device so far
  std::atomic<bool> upload_done{false};
  std::thread upload([&] {
    if (hipSetDevice(ctx->device) != hipSuccess) up_rc = MSM377_EHIP;
    for (uint32_t c = 1; c < K && up_rc == MSM377_OK; c++) {
      up_rc = upload_chunk(c, &up_fail);
      if (up_rc == MSM377_OK) uploaded.store(c + 1, std::memory_order_release);
    }
    upload_done.store(true, std::memory_order_release);
  });
  for (uint32_t c = 0; c < K && rc == MSM377_OK; c++) {
    while (uploaded.load(std::memory_order_acquire) <= c && !upload_done.load(std::memory_order_acquire)) std::this_thread::yield();
    if (uploaded.load(std::memory_order_acquire) <= c) {  // the upload thread stopped on an error
      rc = up_fail.record(ctx, up_rc ? up_rc : MSM377_EHIP);
      break;
    }
    const uint64_t first = cut[c], cnt = cut[c + 1] - cut[c];
    Phase ph;
    ph.clear_err = c == 0;
    ph.into = c > 0;
    ph.back = c + 1 == K;
    ph.base_first = first;
    ph.plan = plan;
    rc = convert_bases<CV>(ctx, ctx->d_raw_points + first * CV::RAW_WORDS, cnt, first, c == 0);
    if (rc == MSM377_OK) rc = enqueue_windows<CV>(ctx, ctx->d_raw_scalars + first * 8, cnt, 0, 0, ph);
  }
  upload.join();
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

int check_args(msm377_ctx* ctx, const void* a, const void* b, uint64_t n, bool need_a) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  if (n > ctx->cap) {
    ctx->err = "n exceeds the context capacity";
    return MSM377_EINVAL;
  }
  if (n && ((need_a && !a) || !b)) {
    ctx->err = "null input pointer";
    return MSM377_EINVAL;
  }
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15)) {
    ctx->err = "device input pointers must be 16-byte aligned";
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

// One check call (include/msm377.h "input validation"): a tiny clear, k_check_curve, and k_check_subgroup over the
// points that passed -- on the main stream, then a host-side wait like every entry point.  The scratch lives where no
// resident form reads: the counters in the front of d_work_meta (every MSM clears that block for itself), the index
// list in d_val_idx (rebuilt by every MSM's sort).  d_points may be d_raw_points or the caller's memory; it is only read.
template <class CK>
int check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  if (!out) return MSM377_EINVAL;
  flags = check_flags_normal(flags);
  if (!flags) return MSM377_EINVAL;
  int rc = check_args(ctx, d_points, d_points, n, true);
  if (rc) return rc;
  check_report_empty(out, n);
  if (n == 0) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t* scratch = ctx->d_work_meta;
  ctx->last.work.valid = false;  // msm377_g1_read_work_list reads its counters from these words
  static_assert(CHK_WORDS <= META_BLOCK_WORDS, "the check's counters fit the work-list block");
  uint32_t* list = (flags & MSM377_CHECK_SUBGROUP) ? ctx->d_val_idx : nullptr;  // cap entries at least (capi.hip: wcap >= 16 cap)
  const dim3 grid((unsigned)((n + CHK_THREADS - 1) / CHK_THREADS));
  hipLaunchKernelGGL(k_check_clear, dim3(1), dim3(64), 0, ctx->stream, scratch);
  // msm377_ctx_set_timing(1): k_check_curve reads as the CONVERT stage, k_check_subgroup as the accumulation kernel
  const bool timed = ctx->timing == 1;
  {
    StageTimer t(ctx, MSM377_STAGE_CONVERT, ctx->stream);
    hipLaunchKernelGGL(k_check_curve<CK>, grid, dim3(CHK_THREADS), 0, ctx->stream, (const uint32_t*)d_points, n, (flags & MSM377_CHECK_CURVE) ? 1u : 0u, scratch, list);
  }
  if (list) {
    StageTimer t(ctx, MSM377_STAGE_ACC_KERNEL, ctx->stream);
    hipLaunchKernelGGL(k_check_subgroup<CK>, grid, dim3(CHK_THREADS), 0, ctx->stream, (const uint32_t*)d_points, scratch, (const uint32_t*)list);
  }
  HIP_TRY(ctx, hipGetLastError());
  uint32_t h[CHK_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (timed) {
    for (int s = 0; s < MSM377_NUM_STAGES; s++) {
      float ms = 0.f;
      const bool ran = s == MSM377_STAGE_CONVERT || (list && s == MSM377_STAGE_ACC_KERNEL);
      ctx->last.stage_ms[s] = ran && hipEventElapsedTime(&ms, ctx->ev[s][0], ctx->ev[s][1]) == hipSuccess ? ms : 0.0;
    }
  }
  out->noncanonical = h[CHK_NONCANON];
  out->off_curve = h[CHK_OFFCURVE];
  out->outside_subgroup = h[CHK_OUTSIDE];
  const uint64_t key = (uint64_t)h[CHK_FIRST] | ((uint64_t)h[CHK_FIRST + 1] << 32);
  if (key != UINT64_MAX) {
    out->first_bad = key >> 2;
    const uint32_t cls = (uint32_t)(key & 3);
    out->first_bad_reason = cls == CHK_CLASS_NONCANON ? MSM377_CHECK_CANONICAL : cls == CHK_CLASS_OFFCURVE ? MSM377_CHECK_CURVE : MSM377_CHECK_SUBGROUP;
  }
  return MSM377_OK;
}

// Host-buffer variant: the points go up into d_sort_temp (128 bytes per point of capacity; like the scratch above it
// belongs to no resident form -- d_raw_points does: it keeps the raw copy of a resident base set).
template <class CK>
int check_points_from_host(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  if (!ctx || !out || !check_flags_normal(flags)) return MSM377_EINVAL;
  ctx->err.clear();
  if (n > ctx->cap) {
    ctx->err = "n exceeds the context capacity";
    return MSM377_EINVAL;
  }
  if (n && !points) {
    ctx->err = "null input pointer";
    return MSM377_EINVAL;
  }
  static_assert(MSM377_NUM_WINDOWS * sizeof(SortElem) >= CK::CV::RAW_WORDS * 4, "d_sort_temp holds the wire points of a full context");
  if (n) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = h2d_staged(ctx, ctx->d_sort_temp, points, n * CK::CV::RAW_WORDS * 4, 0);
    if (rc) return rc;
  }
  return check_points_device<CK>(ctx, ctx->d_sort_temp, n, flags, out);
}

// The opt-in check of the set-bases calls (ctx->knobs.base_checks): MSM377_EPOINT with index and reason in ctx->err.
int check_base_set(msm377_ctx* ctx, const void* d_points, uint64_t n) {
  if (!ctx->knobs.base_checks) return MSM377_OK;
  const int rc = check_points_device<G1Check>(ctx, d_points, n, ctx->knobs.base_checks, &ctx->last_check);
  if (rc) return rc;
  const msm377_check_report& r = ctx->last_check;
  if (r.first_bad == UINT64_MAX) return MSM377_OK;
  const char* why = r.first_bad_reason == MSM377_CHECK_CANONICAL ? "has a coordinate that is not below p"
                    : r.first_bad_reason == MSM377_CHECK_CURVE   ? "is not on the curve"
                                                                 : "is outside the prime-order subgroup";
  ctx->err = "base set refused: point " + std::to_string(r.first_bad) + " " + why + " (" + std::to_string(r.noncanonical + r.off_curve + r.outside_subgroup) + " of " +
             std::to_string(r.checked) + " points failed)";
  return MSM377_EPOINT;
}

// ---- native input forms (include/msm377.h "native input forms"; kernels/import.hpp) ----
// The import pass sits in front of the entry points: it writes wire-format data into the context's staging
// (d_raw_points, d_raw_scalars) and the call goes on with those pointers.  With the default forms every function below
// returns at once: no launch, no allocation, the caller's pointers.
inline bool native_forms(const msm377_ctx* ctx) { return ctx->point_form != MSM377_POINTS_WIRE || ctx->scalar_form != MSM377_SCALARS_WIRE; }
inline size_t point_stride(const msm377_ctx* ctx) { return ctx->point_form == MSM377_POINTS_MONT_FLAG ? 104 : 96; }
enum { MASK_BASES = 0, MASK_CHECK = 1 };  // which of the two masks (and counters) in native.d_inf_mask

// n points in the context's (non-wire) point form at d_in -> wire records at d_out, on the main stream; the side stream,
// which converts them, is ordered behind.  `which`: the mask and counter the pass writes (the counter is cleared first).
int import_points(msm377_ctx* ctx, const void* d_in, uint64_t n, uint32_t* d_out, int which) {
  int rc = ensure_import_buffers(ctx, false);
  if (rc) return rc;
  uint32_t* mask = ctx->native.d_inf_mask + (size_t)which * ctx->native.mask_words();
  uint32_t* count = ctx->native.d_inf_mask + 2 * ctx->native.mask_words() + which;
  const dim3 grid((unsigned)((n + IMPORT_THREADS - 1) / IMPORT_THREADS)), block(IMPORT_THREADS);
  if (ctx->point_form == MSM377_POINTS_MONT_FLAG) {
    hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, ctx->stream, count, 1u, (uint32_t*)nullptr, 0u);
    hipLaunchKernelGGL(k_import_points<MSM377_POINTS_MONT_FLAG>, grid, block, 0, ctx->stream, (const uint8_t*)d_in, d_out, n, mask, count);
  } else {
    hipLaunchKernelGGL(k_import_points<MSM377_POINTS_MONT>, grid, block, 0, ctx->stream, (const uint8_t*)d_in, d_out, n, mask, count);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->native.import_done, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->native.import_done, 0));
  return MSM377_OK;
}

// The scalars of a call as the decomposition kernels read them: d_in itself for wire scalars without a mask (nothing is
// launched), else ctx->d_raw_scalars, written on the main stream by k_import_scalars.  words: u32 per scalar (8; 1, 2
// or 4 for compact short scalars, wire form only).  mask: the infinity mask of the call's points, or null.
int import_scalars(msm377_ctx* ctx, const void* d_in, uint64_t n, uint32_t words, const uint32_t* mask, const uint32_t** d_out) {
  *d_out = (const uint32_t*)d_in;
  const bool mont = ctx->scalar_form == MSM377_SCALARS_MONT;
  if ((!mont && !mask) || n == 0) return MSM377_OK;
  const dim3 grid((unsigned)((n + IMPORT_THREADS - 1) / IMPORT_THREADS)), block(IMPORT_THREADS);
  const uint32_t* in = (const uint32_t*)d_in;
  uint32_t* out = ctx->d_raw_scalars;
  if (mont && mask) hipLaunchKernelGGL((k_import_scalars<MSM377_SCALARS_MONT, true>), grid, block, 0, ctx->stream, in, out, n, words, mask);
  else if (mont) hipLaunchKernelGGL((k_import_scalars<MSM377_SCALARS_MONT, false>), grid, block, 0, ctx->stream, in, out, n, words, mask);
  else hipLaunchKernelGGL((k_import_scalars<MSM377_SCALARS_WIRE, true>), grid, block, 0, ctx->stream, in, out, n, words, mask);
  HIP_TRY(ctx, hipGetLastError());
  *d_out = out;
  return MSM377_OK;
}

// Points and scalars of a per-call MSM: both pointers are replaced by the staging the pass wrote.  The caller has
// dropped the resident bases (the pass overwrites their raw copy).
int import_inputs(msm377_ctx* ctx, const void** d_points, const void** d_scalars, uint64_t n, uint32_t scalar_words = 8) {
  if (!native_forms(ctx)) return MSM377_OK;
  const uint32_t* mask = nullptr;
  if (ctx->point_form != MSM377_POINTS_WIRE) {
    const int rc = import_points(ctx, *d_points, n, ctx->d_raw_points, MASK_BASES);
    if (rc) return rc;
    *d_points = ctx->d_raw_points;
    if (ctx->point_form == MSM377_POINTS_MONT_FLAG) mask = ctx->native.d_inf_mask;
  }
  const uint32_t* sc = nullptr;
  const int rc = import_scalars(ctx, *d_scalars, n, scalar_words, mask, &sc);
  *d_scalars = sc;
  return rc;
}

// A base set: the points alone, and the number of flagged ones for the resident-base value (a host-side wait: the
// set-bases calls wait for the device anyway).
int import_base_set(msm377_ctx* ctx, const void** d_points, uint64_t n, uint32_t* flagged) {
  *flagged = 0;
  if (ctx->point_form == MSM377_POINTS_WIRE || n == 0) return MSM377_OK;
  const int rc = import_points(ctx, *d_points, n, ctx->d_raw_points, MASK_BASES);
  if (rc) return rc;
  *d_points = ctx->d_raw_points;
  if (ctx->point_form == MSM377_POINTS_MONT_FLAG) {
    HIP_TRY(ctx, hipMemcpyAsync(flagged, ctx->native.d_inf_mask + 2 * ctx->native.mask_words() + MASK_BASES, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MSM377_OK;
}

// Host-buffer calls in a native form: each array goes up in one piece into d_native (no chunked overlap), and the call
// continues on the device-pointer path, which imports from there.  Either array may be absent.
int upload_native(msm377_ctx* ctx, const uint8_t* points, size_t point_bytes, const uint8_t* scalars, size_t scalar_bytes) {
  int rc = ensure_import_buffers(ctx, true);
  if (rc == MSM377_OK && points && point_bytes) rc = h2d_staged(ctx, ctx->native.native_points(), points, point_bytes, 0);
  if (rc == MSM377_OK && scalars && scalar_bytes) rc = h2d_staged(ctx, ctx->native.native_scalars(), scalars, scalar_bytes, 0);
  return rc;
}

int refuse_mont_short(msm377_ctx* ctx) {
  if (ctx->scalar_form != MSM377_SCALARS_MONT) return MSM377_OK;
  ctx->err = "short-scalar calls take wire-format scalars: there is no compact Montgomery scalar (msm377_ctx_set_input_format)";
  return MSM377_EINVAL;
}

}  // namespace

// ---- entry points (C ABI: capi.hip forwards) ----

// G1 points in a native form are imported into d_sort_temp first (as the host-buffer variant uploads there: it belongs to
// no resident form), with the check calls' own mask: a coordinate of p or more arrives unchanged and is counted
// non-canonical, a flagged point arrives as the generator and is counted in no class.
int g1_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  if (ctx && ctx->point_form != MSM377_POINTS_WIRE && out && check_flags_normal(flags) && n) {
    int rc = check_args(ctx, d_points, d_points, n, true);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = import_points(ctx, d_points, n, (uint32_t*)ctx->d_sort_temp, MASK_CHECK);
    if (rc) return rc;
    d_points = ctx->d_sort_temp;
  }
  return check_points_device<G1Check>(ctx, d_points, n, flags, out);
}
int g1_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  if (ctx && ctx->point_form != MSM377_POINTS_WIRE && out && check_flags_normal(flags) && n && n <= ctx->cap && points) {
    ctx->err.clear();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = upload_native(ctx, points, n * point_stride(ctx), nullptr, 0);
    return rc ? rc : g1_check_points_device(ctx, ctx->native.native_points(), n, flags, out);
  }
  return check_points_from_host<G1Check>(ctx, points, n, flags, out);
}
int ed_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out) { return check_points_device<EdCheck>(ctx, d_points, n, flags, out); }
int ed_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) { return check_points_from_host<EdCheck>(ctx, points, n, flags, out); }

// ---- per-call G1 MSMs: msm377_g1_msm* and, with a short spec (sbytes scalar bytes, every scalar below 2^bits; 0 = full
// width), msm377_g1_msm_short* ----
namespace {

// An exceptional case of the Edwards law means points outside the prime-order subgroup: the call runs again on
// Weierstrass records, never behind the GLV front end.
int g1_rerun_weierstrass(msm377_ctx* ctx, const uint32_t* d_points, const uint32_t* d_scalars, uint64_t n, uint8_t out_xy[96], uint32_t sbytes, uint32_t bits) {
  const int rc = convert_table(ctx, d_points, n, TABLE_XYZZ);
  return rc ? rc : g1_table_msm(ctx, d_scalars, n, TABLE_XYZZ, out_xy, sbytes, bits);
}

// Device pointers: import, pick the form, convert, run the table call, rerun on the Weierstrass path if it asks for it.
int g1_device_flow(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[96], uint32_t sbytes, uint32_t bits) {
  if (n == 0) {
    identity_wire(out_xy);
    return MSM377_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->resident.clear();
  int rc = import_inputs(ctx, &d_points, &d_scalars, n, sbytes ? sbytes / 4 : 8);  // (native input forms only)
  if (rc) return rc;
  const uint32_t *pts = (const uint32_t*)d_points, *sc = (const uint32_t*)d_scalars;
  int form = sbytes && ctx->knobs.g1_form != 1 ? (int)TABLE_XYZZ : pick_form(ctx);  // a short call never takes the GLV front end
  // (Queueing the conversion after k_decompose instead was measured: decompose 77 -> 23 us, sort 272 -> 386 us.)
  if (form == TABLE_TE && ctx->knobs.te_affine_msm && n >= ctx->knobs.affine_min_points) {
    // Affine records (7-product additions) by the batched conversion: its way up is queued now, the host's inversion
    // and the way down happen from the hook, once decompose .. work list are queued on the main stream.
    form = TABLE_TE_AFFINE;
    rc = affine_convert_begin(ctx, pts, n);
    if (rc) return rc;
    ctx->before_accumulate = [ctx, n]() -> int { return affine_convert_finish(ctx, ctx->d_bases, n); };
  } else {
    rc = convert_table(ctx, pts, n, form);
    if (rc) return rc;
  }
  rc = g1_table_msm(ctx, sc, n, form, out_xy, sbytes, bits);
  ctx->before_accumulate = nullptr;
  return rc == RC_TE_FALLBACK ? g1_rerun_weierstrass(ctx, pts, sc, n, out_xy, sbytes, bits) : rc;
}

// Host buffers in one piece.  Scalars first: decomposition, sort and the work lists need nothing else, so they run
// while the points (three quarters of the bytes at full width) are still on their way on the upload thread; the hook
// joins it and launches the conversion to `form` right before the accumulation is queued (TABLE_TE_AFFINE: both phases
// of the batched conversion back to back).
int g1_host_flow(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, int form, uint8_t out_xy[96], uint32_t sbytes, uint32_t bits) {
  const uint32_t *d_sc = ctx->d_raw_scalars, *d_pt = ctx->d_raw_points;
  int rc = h2d_staged(ctx, ctx->d_raw_scalars, scalars, n * (sbytes ? sbytes : 32), (size_t)ctx->cap * 96);
  if (rc) return rc;
  int up_rc = MSM377_OK;
  HipFail up_fail;
  std::thread upload([&] { up_rc = hipSetDevice(ctx->device) == hipSuccess ? h2d_staged(ctx, ctx->d_raw_points, points, n * 96, 0, &up_fail) : MSM377_EHIP; });
  ctx->before_accumulate = [&]() -> int {
    if (upload.joinable()) upload.join();
    if (up_rc) return up_fail.record(ctx, up_rc);
    return convert_table(ctx, d_pt, n, form);
  };
  rc = g1_table_msm(ctx, d_sc, n, form, out_xy, sbytes, bits);
  ctx->before_accumulate = nullptr;
  if (upload.joinable()) upload.join();  // an error before the hook ran
  return rc == RC_TE_FALLBACK ? g1_rerun_weierstrass(ctx, d_pt, d_sc, n, out_xy, sbytes, bits) : rc;
}

}  // namespace

int g1_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[96]) {
  if (!out_xy) return MSM377_EINVAL;
  const int rc = check_args(ctx, d_points, d_scalars, n, true);
  return rc ? rc : g1_device_flow(ctx, d_points, d_scalars, n, out_xy, 0, 0);
}

int g1_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]) {
  if (!ctx || !out_xy) return MSM377_EINVAL;
  ctx->err.clear();
  if (n > ctx->cap || (n && (!points || !scalars))) {
    ctx->err = "bad arguments";
    return MSM377_EINVAL;
  }
  if (n == 0) {
    identity_wire(out_xy);
    return MSM377_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (native_forms(ctx)) {  // one upload per array, then the device-pointer path
    const int up = upload_native(ctx, points, n * point_stride(ctx), scalars, n * 32);
    return up ? up : g1_msm_device(ctx, ctx->native.native_points(), ctx->native.native_scalars(), n, out_xy);
  }
  ctx->resident.clear();
  const int form = pick_form(ctx);  // (projective Edwards records at any n)
  if (n < ctx->knobs.upload_chunk_min || form == TABLE_XYZZ_GLV || ctx->capture)  // (stage read-backs describe the plain row layout)
    return g1_host_flow(ctx, points, scalars, n, form, out_xy, 0, 0);
  const bool te = form == TABLE_TE;
  const WindowPlan plan = plan_whole16(ctx, te ? TE_TAIL : XYZZ_TAIL);
  int rc = te ? run_chunked_upload<TeDev>(ctx, points, scalars, n, plan) : run_chunked_upload<G1Dev>(ctx, points, scalars, n, plan);
  if (rc == MSM377_OK) rc = wait_windows(ctx, 0);
  if (rc) return rc;
  // Whatever sends the call round again below finds everything on the device by now and runs in one piece.
  const int err = ctx->h_err[0];
  if (te && (err & ERR_TE_ANY)) {
    note_fallback(ctx, (uint32_t)(err & ERR_TE_ANY));
  } else if (geometry_refused(plan, err)) {  // a scalar of 2^253 and more: g1_table_msm falls back to sixteen equal windows by itself
    ctx->fallback.geometry_reruns++;
    rc = convert_table(ctx, ctx->d_raw_points, n, form);
    if (rc == MSM377_OK) rc = g1_table_msm(ctx, ctx->d_raw_scalars, n, form, out_xy);
    if (rc != RC_TE_FALLBACK) return rc;
  } else {
    rc = collect_windows(ctx, 0);
    if (rc == MSM377_OK) rc = run_tail(ctx, plan, ctx->h_partials, out_xy);
    if (rc != RC_TE_FALLBACK) return rc;
  }
  return g1_rerun_weierstrass(ctx, ctx->d_raw_points, ctx->d_raw_scalars, n, out_xy, 0, 0);
}

int g1_msm_short_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t sbytes, uint32_t bits, uint8_t out_xy[96]) {
  if (!out_xy) return MSM377_EINVAL;
  int rc = check_args(ctx, d_points, d_scalars, n, true);
  if (rc == MSM377_OK) rc = check_short_args(ctx, sbytes, bits);
  if (rc == MSM377_OK) rc = refuse_mont_short(ctx);
  return rc ? rc : g1_device_flow(ctx, d_points, d_scalars, n, out_xy, sbytes, bits);
}

// Host buffers: the compact scalars go up first (n x scalar_bytes), always in one piece (a chunked short upload is not
// implemented), on affine records from affine_min_points on.
int g1_msm_short(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t sbytes, uint32_t bits, uint8_t out_xy[96]) {
  if (!ctx || !out_xy) return MSM377_EINVAL;
  ctx->err.clear();
  if (n > ctx->cap || (n && (!points || !scalars))) {
    ctx->err = "bad arguments";
    return MSM377_EINVAL;
  }
  int rc = check_short_args(ctx, sbytes, bits);
  if (rc == MSM377_OK) rc = refuse_mont_short(ctx);
  if (rc) return rc;
  if (n == 0) {
    identity_wire(out_xy);
    return MSM377_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (native_forms(ctx)) {
    rc = upload_native(ctx, points, n * point_stride(ctx), scalars, n * sbytes);
    return rc ? rc : g1_msm_short_device(ctx, ctx->native.native_points(), ctx->native.native_scalars(), n, sbytes, bits, out_xy);
  }
  ctx->resident.clear();
  const bool te = ctx->knobs.g1_form == 1;
  const bool affine = te && ctx->knobs.te_affine_msm && n >= ctx->knobs.affine_min_points;
  return g1_host_flow(ctx, points, scalars, n, !te ? TABLE_XYZZ : affine ? TABLE_TE_AFFINE : TABLE_TE, out_xy, sbytes, bits);
}

int scalars_width_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t sbytes, uint32_t* bits_out) {
  if (!ctx || !bits_out) return MSM377_EINVAL;
  ctx->err.clear();
  if (sbytes != 4 && sbytes != 8 && sbytes != 16 && sbytes != 32) {
    ctx->err = "scalar_bytes must be 4, 8, 16 or 32";
    return MSM377_EINVAL;
  }
  if ((n && !d_scalars) || ((uintptr_t)d_scalars & 15)) {
    ctx->err = "the device scalars pointer must be non-null and 16-byte aligned";
    return MSM377_EINVAL;
  }
  *bits_out = 0;
  if (n == 0) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the result word: the front of the work-list block, which every MSM clears for itself and no resident form reads
  uint32_t* d_out = ctx->d_work_meta;
  ctx->last.work.valid = false;  // msm377_g1_read_work_list reads its histogram from these words
  const uint64_t nwords = n * (sbytes / 4);
  const unsigned blocks = (unsigned)std::min<uint64_t>((nwords / 4 + 255) / 256 + 1, 2048);
  hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, ctx->stream, d_out, 1u, (uint32_t*)nullptr, 0u);
  hipLaunchKernelGGL(k_scalars_width, dim3(blocks), dim3(256), 0, ctx->stream, (const uint32_t*)d_scalars, nwords, sbytes / 4, d_out);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t h = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&h, d_out, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *bits_out = h;
  return MSM377_OK;
}

// ---- Edwards-BLS12 (BASELINE.json config 3): same pipeline, EdDev policy ----
namespace {
// equal_windows: the rerun of a chunked upload whose scalars did not fit the even geometry.
int ed_device_flow(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[64], bool equal_windows) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->resident.clear();
  int rc = convert_bases<EdDev>(ctx, (const uint32_t*)d_points, n);
  if (rc) return rc;
  TailArm arm(ctx);
  arm.at_start(n);
  Phase ph;
  ph.zc_out = true;
  ph.plan = equal_windows || ctx->capture == 1 ? plan_equal16(ED_TAIL) : plan_whole16(ctx, ED_TAIL);
  for (;;) {
    rc = enqueue_windows<EdDev>(ctx, (const uint32_t*)d_scalars, n, 0, 0, ph);
    if (rc) return rc;
    arm.after_accumulation();
    rc = wait_windows(ctx, 0);
    if (rc) return rc;
    if (geometry_refused(ph.plan, ctx->h_err[0])) {  // a scalar of 2^253 and more: sixteen equal windows
      ctx->fallback.geometry_reruns++;
      ph.plan = next_plan(ph.plan);
      continue;
    }
    rc = collect_windows(ctx, 0);
    return rc ? rc : run_tail(ctx, ph.plan, ctx->h_partials, out_xy);
  }
}
}  // namespace

int ed_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[64]) {
  if (!out_xy) return MSM377_EINVAL;
  int rc = check_args(ctx, d_points, d_scalars, n, true);
  if (rc) return rc;
  if (n == 0) {  // the neutral element (0, 1)
    memset(out_xy, 0, 64);
    out_xy[32] = 1;
    return MSM377_OK;
  }
  return ed_device_flow(ctx, d_points, d_scalars, n, out_xy, false);
}

int ed_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[64]) {
  if (!ctx || !out_xy) return MSM377_EINVAL;
  ctx->err.clear();
  if (n > ctx->cap || (n && (!points || !scalars))) {
    ctx->err = "bad arguments";
    return MSM377_EINVAL;
  }
  if (n == 0) return ed_msm_device(ctx, nullptr, nullptr, 0, out_xy);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->resident.clear();  // (both paths upload into d_raw_points)
  if (n >= ctx->knobs.upload_chunk_min && !ctx->capture) {  // chunks of points, like g1_msm: a chunk computes while the next one uploads (stage read-backs describe the plain row layout)
    const WindowPlan plan = plan_whole16(ctx, ED_TAIL);
    int rc = run_chunked_upload<EdDev>(ctx, points, scalars, n, plan);
    if (rc == MSM377_OK) rc = wait_windows(ctx, 0);
    if (rc) return rc;
    if (geometry_refused(plan, ctx->h_err[0])) {  // everything is on the device: once more in one piece
      ctx->fallback.geometry_reruns++;
      return ed_device_flow(ctx, ctx->d_raw_points, ctx->d_raw_scalars, n, out_xy, true);
    }
    rc = collect_windows(ctx, 0);
    return rc ? rc : run_tail(ctx, plan, ctx->h_partials, out_xy);
  }
  int rc = h2d_staged(ctx, ctx->d_raw_points, points, n * 64, 0);
  if (rc == MSM377_OK) rc = h2d_staged(ctx, ctx->d_raw_scalars, scalars, n * 32, (size_t)ctx->cap * 96);
  if (rc) return rc;
  return ed_msm_device(ctx, ctx->d_raw_points, ctx->d_raw_scalars, n, out_xy);
}

int ed_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out) {
  if (!ctx || (n && !d_points_out) || ((uintptr_t)d_points_out & 15)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_generate_bases_ed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, seed, n, (uint32_t*)d_points_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM377_OK;
}

// The precomputed-window table and its wide-window work buffers (allocated on demand, 2.2-2.7 GB at 2^20 points), once
// nothing queued on either stream reads them any more.
int free_table(msm377_ctx* ctx) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
  ctx->own.release(ctx->resident.table);
  ctx->resident = ResidentBases();  // (its callers have cleared it)
  ctx->wide.release(ctx->own);
  return MSM377_OK;
}

// The four set-bases entry points clear the resident bases before anything else and set them as their last step: a
// call that fails, for whatever reason, leaves none (include/msm377.h).
static int build_bases(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flagged);
int g1_set_bases_device(msm377_ctx* ctx, const void* d_points, uint64_t n) {
  if (ctx) ctx->resident.clear();
  int rc = check_args(ctx, d_points, d_points, n, true);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t flagged = 0;
  rc = import_base_set(ctx, &d_points, n, &flagged);  // (native point forms only)
  if (rc) return rc;
  return build_bases(ctx, d_points, n, flagged);
}

// d_points: wire records (the caller's, or d_raw_points after an upload or an import); flagged: how many of them stand
// in for identity points, ctx->native.d_inf_mask says which.
static int build_bases(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flagged) {
  int rc = check_base_set(ctx, d_points, n);  // opt-in (msm377_ctx_set_base_checks)
  if (rc) return rc;
  int form = pick_form(ctx);
  if (form == TABLE_TE) form = TABLE_TE_AFFINE;  // resident: affine records by the batched inversion, once
  rc = convert_table(ctx, (const uint32_t*)d_points, n, form);
  if (rc) return rc;
  // raw copy for the (never expected) fallback from the Edwards form: see resident_table_to_weierstrass
  if (form_is_te(form) && d_points != ctx->d_raw_points)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_raw_points, d_points, n * 96, hipMemcpyDeviceToDevice, ctx->stream2));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
  if (ctx->resident.table) {  // a plain table replaces a precomputed one: give its gigabytes back
    rc = free_table(ctx);
    if (rc) return rc;
  }
  ctx->resident.set(ctx->d_bases, n, form, flagged, ctx->native.d_inf_mask);
  return MSM377_OK;
}

// The host-buffer variants: the points go up into d_raw_points, and the device variant builds from there.
static int set_bases_from_host(msm377_ctx* ctx, const uint8_t* points, uint64_t n, int (*build)(msm377_ctx*, const void*, uint64_t)) {
  if (ctx) ctx->resident.clear();
  if (!ctx || n > ctx->cap || (n && !points)) return MSM377_EINVAL;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->point_form != MSM377_POINTS_WIRE) {  // the native records go up as they are; the device variant imports them
    const int up = upload_native(ctx, points, n * point_stride(ctx), nullptr, 0);
    return up ? up : build(ctx, ctx->native.native_points(), n);
  }
  int rc = h2d_staged(ctx, ctx->d_raw_points, points, n * 96, 0);
  return rc ? rc : build(ctx, ctx->d_raw_points, n);
}

int g1_set_bases(msm377_ctx* ctx, const uint8_t* points, uint64_t n) { return set_bases_from_host(ctx, points, n, g1_set_bases_device); }

// Precomputed-window tables (BASELINE.json config 5 "precomputed-point reuse"; the reference lists precomputation as
// future work, README.md:558-563): T[w][i] = [2^(c w)] P_i as affine Edwards records.  Window 0 is the batched
// conversion of the input; every further window doubles the previous one c times (unified law) and runs through the
// same batched inversion (k_affine_up<AffDoublingSource> -> host -> k_affine_down).
//   c = 16 (round 2): 16 windows, the main path's geometry; the 16 bucket sets are folded after the accumulation.
//   c = 20 (round 3, msm377_ctx_set_precompute_window): 13 windows over ONE set of 2^19 buckets -- 13 n bucket
//          additions per MSM instead of 16 n (kernels/wide.hpp).
int g1_set_bases_precomputed_device(msm377_ctx* ctx, const void* d_points, uint64_t n) {
  if (ctx) ctx->resident.clear();
  int rc = check_args(ctx, d_points, d_points, n, true);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t flagged = 0;
  rc = import_base_set(ctx, &d_points, n, &flagged);  // (native point forms only)
  if (rc) return rc;
  if (ctx->knobs.g1_form != 1 || n == 0) return build_bases(ctx, d_points, n, flagged);  // Weierstrass form: no precomputation
  rc = check_base_set(ctx, d_points, n);  // opt-in (msm377_ctx_set_base_checks), before anything is allocated or converted
  if (rc) return rc;
  const bool wide = ctx->knobs.precomp_bits == (int)WIDE_BITS;
  if (wide && (uint64_t)WIDE_WINDOWS * n >= (1ull << 31)) {
    ctx->err = "precomputed-window table: too many points for 20-bit windows (13 n must stay below 2^31)";
    return MSM377_EINVAL;
  }
  const uint32_t windows = wide ? WIDE_WINDOWS : (uint32_t)MSM377_NUM_WINDOWS;
  ResidentBases& r = ctx->resident;
  if (r.cap < n || r.windows != windows) {
    rc = free_table(ctx);
    if (rc) return rc;
    if (ctx->own.alloc((void**)&r.table, (size_t)windows * n * TeAffBase::REC_WORDS * 4) != hipSuccess || (wide && !ctx->wide.ensure(ctx->own, n, WC_WORDS))) {
      (void)free_table(ctx);
      (void)hipGetLastError();
      ctx->err = "precomputed-window table: out of device memory";
      return MSM377_ENOMEM;
    }
    r.cap = n;
    r.windows = windows;
  }
  for (uint32_t w = 0; w < windows && rc == MSM377_OK; w++) {
    const uint32_t doublings = !wide ? (uint32_t)MSM377_WINDOW_BITS : w ? wide_width(w - 1) : 0u;  // from the previous window's multiple to this one's
    uint32_t* mine = r.table + (size_t)w * n * TeAffBase::REC_WORDS;
    rc = affine_convert_begin(ctx, (const uint32_t*)d_points, n, w == 0 ? nullptr : mine - (size_t)n * TeAffBase::REC_WORDS, doublings, w == 0);
    if (rc == MSM377_OK) rc = affine_convert_finish(ctx, mine, n);
  }
  if (rc) return rc;
  if (d_points != ctx->d_raw_points) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_raw_points, d_points, n * 96, hipMemcpyDeviceToDevice, ctx->stream2));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
  r.set(ctx->d_bases, n, TABLE_TE_PRECOMP, flagged, ctx->native.d_inf_mask);
  BasesLayout& bl = ctx->last.bases;  // affine_convert_finish described the last window; the table is all of them, n records apart
  bl.d_records = r.table;
  bl.info.windows = windows;
  bl.info.window_stride = n;
  bl.info.records = (uint64_t)windows * n;
  for (uint32_t w = 0; w < windows; w++) bl.info.window_bits[w] = wide ? wide_width(w) : (uint32_t)MSM377_WINDOW_BITS;
  return MSM377_OK;
}

int g1_set_bases_precomputed(msm377_ctx* ctx, const uint8_t* points, uint64_t n) {
  return set_bases_from_host(ctx, points, n, g1_set_bases_precomputed_device);
}

// Whatever the last set-bases call left resident serves, at full width or (sbytes != 0) over scalars of a declared width.
static int g1_fixed_base_flow(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint8_t out_xy[96], uint32_t sbytes, uint32_t bits) {
  if (n > ctx->resident.n) {
    ctx->err = "fixed-base MSM needs g1_set_bases with at least n points first";
    return MSM377_ESTATE;
  }
  if (n == 0) {
    identity_wire(out_xy);
    return MSM377_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->timing == 1) {  // no conversion in this mode
    (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][0], ctx->stream);
    (void)hipEventRecord(ctx->ev[MSM377_STAGE_CONVERT][1], ctx->stream);
  }
  // (records 0 .. n-1 of a GLV table are the plain points: a short call reads those and never the phi half)
  auto form = [&] { return sbytes && ctx->resident.form == TABLE_XYZZ_GLV ? (int)TABLE_XYZZ : resident_form(ctx, n); };
  const uint32_t* sc = nullptr;  // d_scalars, or their import: Montgomery scalars, the zeroed scalars of flagged bases
  int rc = import_scalars(ctx, d_scalars, n, sbytes ? sbytes / 4 : 8, ctx->resident.flagged ? ctx->resident.inf_mask : nullptr, &sc);
  if (rc) return rc;
  rc = g1_table_msm(ctx, sc, n, form(), out_xy, sbytes, bits);
  if (rc != RC_TE_FALLBACK) return rc;
  rc = resident_table_to_weierstrass(ctx);
  return rc ? rc : g1_table_msm(ctx, sc, n, form(), out_xy, sbytes, bits);
}

int g1_msm_fixed_base_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint8_t out_xy[96]) {
  if (!out_xy) return MSM377_EINVAL;
  const int rc = check_args(ctx, nullptr, d_scalars, n, false);
  return rc ? rc : g1_fixed_base_flow(ctx, d_scalars, n, out_xy, 0, 0);
}

int g1_msm_fixed_base_short_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t sbytes, uint32_t bits, uint8_t out_xy[96]) {
  if (!out_xy) return MSM377_EINVAL;
  int rc = check_args(ctx, nullptr, d_scalars, n, false);
  if (rc == MSM377_OK) rc = check_short_args(ctx, sbytes, bits);
  if (rc == MSM377_OK) rc = refuse_mont_short(ctx);
  return rc ? rc : g1_fixed_base_flow(ctx, d_scalars, n, out_xy, sbytes, bits);
}

// `batch` MSMs of n scalars each against the table resident in (or lent to, twin_borrow) `ctx`, on ctx's own stream and
// buffers.  RC_TE_FALLBACK: an exceptional case of the Edwards law; nothing of out_xy is valid then.
static int fixed_base_batch_share(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t batch, uint8_t* out_xy) {
  int rc = MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t* sc = (const uint32_t*)d_scalars;
  // MSM b's scalars as its decomposition reads them: in place, or imported into THIS context's staging right in front
  // of it on its stream -- the decomposition is the only reader, so MSM b + 1's import may follow MSM b's kernels.
  const uint32_t* inf_mask = ctx->resident.flagged ? ctx->resident.inf_mask : nullptr;
  auto scalars_of = [&](uint32_t b, const uint32_t** out) { return import_scalars(ctx, sc + (size_t)b * n * 8, n, 8, inf_mask, out); };
  const uint32_t* sb = nullptr;
  const int form = resident_form(ctx, n);
  const bool glv = form == TABLE_XYZZ_GLV, te = form_is_te(form);
  Phase ph;  // every MSM of the share runs this plan; its records are combined on this thread, beside the GPU
  ph.plan = wide_table(ctx->resident)    ? plan_wide13(ctx->resident.table, ctx->resident.n)
            : form == TABLE_TE_PRECOMP ? folded_behind_table(plan_equal16(TE_TAIL), ctx->resident.table, ctx->resident.n)
            : glv                      ? plan_glv8()
                                       : plan_whole16(ctx, te ? TE_TAIL : XYZZ_TAIL);
  ph.plan.on_caller = true;
  std::vector<uint32_t> redo;  // elements whose scalars fall outside the GLV range: rerun plain afterwards
  std::vector<uint32_t> redo_wide;  // elements with a scalar of 2^253 and more on the wide table or the even windows: rerun one by one (g1_table_msm falls back)
  bool te_fallback = false;
  // Software pipeline over the batch: while the GPU runs MSM b, the host finishes MSM b-1
  // (Horner + inversion on the other slot's partial records).
  for (uint32_t b = 0; b <= batch; b++) {
    if (b < batch && !te_fallback) {
      rc = scalars_of(b, &sb);
      if (rc) return rc;
      rc = enqueue_form(ctx, form, sb, n, (int)(b & 1), ph);
      if (rc) return rc;
    }
    if (b > 0) {
      const int slot = (int)((b - 1) & 1);
      rc = wait_windows(ctx, slot);
      if (rc) return rc;
      const int err = ctx->h_err[slot];
      if (te && !te_fallback && (err & ERR_TE_ANY)) {
        te_fallback = true;
        note_fallback(ctx, (uint32_t)(err & ERR_TE_ANY));
      }
      if (te_fallback) continue;
      if (geometry_refused(ph.plan, err)) {
        (glv ? redo : redo_wide).push_back(b - 1);
        if (!glv) ctx->fallback.geometry_reruns++;
        continue;
      }
      rc = collect_windows(ctx, slot);
      if (rc == MSM377_OK) rc = run_tail(ctx, ph.plan, ctx->h_partials + (size_t)slot * SLOT_WORDS, out_xy + (size_t)96 * (b - 1));
      if (rc == RC_TE_FALLBACK)
        te_fallback = true;
      else if (rc)
        return rc;
    }
  }
  if (te_fallback) {  // an exceptional case of the Edwards law somewhere in the batch: the caller rebuilds the table and reruns
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RC_TE_FALLBACK;
  }
  for (uint32_t b : redo) {
    rc = scalars_of(b, &sb);
    if (rc == MSM377_OK) rc = g1_table_msm(ctx, sb, n, TABLE_XYZZ, out_xy + (size_t)96 * b);
    if (rc) return rc;
  }
  for (uint32_t b : redo_wide) {
    rc = scalars_of(b, &sb);
    if (rc == MSM377_OK) rc = g1_table_msm(ctx, sb, n, form, out_xy + (size_t)96 * b);
    if (rc) return rc;  // RC_TE_FALLBACK included
  }
  return MSM377_OK;
}

void twin_return(msm377_ctx* ctx) {
  if (ctx->twin) ctx->twin->resident = ResidentBases();
}

// The twin of a context: a second context on the same device -- own streams, work buffers, pinned records -- that BORROWS
// the resident table for the length of one batch call.  Created with the first batch that is large enough; its cost
// (the work buffers a second time, ~0.7 GB at 2^20 points) is why small batches do not ask for it.
constexpr uint32_t TWIN_MIN_BATCH = 4;

static int twin_prepare(msm377_ctx* ctx) {
  if (!ctx->twin) {
    if (ctx->twin_failed) return MSM377_ENOMEM;
    msm377_ctx* tw = nullptr;
    if (ctx_create(ctx->device, ctx->cap, ctx->knobs, true, &tw) != MSM377_OK) {  // (true: it only ever borrows the resident bases)
      ctx->twin_failed = true;  // out of memory for a second set: batches run on one
      (void)hipGetLastError();
      return MSM377_ENOMEM;
    }
    ctx->twin = tw;
  }
  msm377_ctx* tw = ctx->twin;
  if (wide_table(ctx->resident) && !tw->wide.ensure(tw->own, ctx->resident.n, WC_WORDS)) return MSM377_ENOMEM;
  // lend the table, and the conversion's verdict that travels with it (d_err[2], read by the accumulation kernels)
  tw->resident = ctx->resident;
  tw->scalar_form = ctx->scalar_form;  // (its share imports its own scalars into its own staging)
  tw->knobs = ctx->knobs;  // every launch shape of its share is its owner's, whatever a setter has changed since it was made
  tw->knobs.twin_batches = false;
  if (hipMemcpyAsync(tw->d_err + 2, ctx->d_err + 2, sizeof(int), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    twin_return(ctx);
    return MSM377_EHIP;
  }
  return MSM377_OK;
}

int g1_msm_fixed_base_batch_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t batch, uint8_t* out_xy) {
  if (!out_xy) return MSM377_EINVAL;
  int rc = check_args(ctx, nullptr, d_scalars, n, false);
  if (rc) return rc;
  if (n > ctx->resident.n) {
    ctx->err = "fixed-base MSM needs g1_set_bases with at least n points first";
    return MSM377_ESTATE;
  }
  if (n == 0) {
    for (uint32_t b = 0; b < batch; b++) identity_wire(out_xy + (size_t)96 * b);
    return MSM377_OK;
  }
  // Batches run as two halves on two sets of streams and buffers (twin_prepare): the low-occupancy ends of one MSM --
  // the last tree levels and the tail of its reduction, the drain of its accumulation kernel, its memory-bound sort --
  // fill with the other half's kernels.  Two contexts side by side measured 2.01 -> 1.89 ms per MSM on the 20-bit table
  // and 2.19 -> 2.09 on the plain one (tools/twin_probe.py, profiles/r03_final/twin_probe.txt).
  const bool split = batch >= TWIN_MIN_BATCH && ctx->knobs.twin_batches && !ctx->timing && !ctx->capture && twin_prepare(ctx) == MSM377_OK;
  msm377_ctx* tw = split ? ctx->twin : nullptr;
  const uint32_t mine = split ? batch - batch / 2 : batch;
  int rc2 = MSM377_OK;
  std::thread other;
  if (tw) other = std::thread([&] { rc2 = fixed_base_batch_share(tw, (const uint32_t*)d_scalars + (size_t)mine * n * 8, n, batch - mine, out_xy + (size_t)96 * mine); });
  rc = fixed_base_batch_share(ctx, d_scalars, n, mine, out_xy);
  if (tw) other.join();
  // A share that failed may have left kernels queued that read the (borrowed) table, which the caller may rebuild or
  // free next: after an error every stream of both contexts is idle before the twin gives it back and the call returns.
  if (rc || rc2)
    for (msm377_ctx* c : {ctx, tw})
      if (c) (void)hipStreamSynchronize(c->stream), (void)hipStreamSynchronize(c->stream2);
  if (tw) {
    twin_return(ctx);
    if (rc2 && !rc) {  // the first half's error wins; RC_TE_FALLBACK of either half reruns the whole batch
      rc = rc2;
      if (rc2 != RC_TE_FALLBACK) ctx->err = tw->err;
    }
    if (tw->fallback.count) {
      ctx->fallback.count += tw->fallback.count;
      ctx->fallback.mask = tw->fallback.mask;
      tw->fallback.count = 0;
    }
  }
  if (rc != RC_TE_FALLBACK) return rc;
  rc = resident_table_to_weierstrass(ctx);  // whole batch again on the Weierstrass table
  if (rc) return rc;
  return g1_msm_fixed_base_batch_device(ctx, d_scalars, n, batch, out_xy);
}

int g1_msm_fixed_base(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]) {
  if (!ctx || !out_xy || n > ctx->cap || (n && !scalars)) return MSM377_EINVAL;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->scalar_form != MSM377_SCALARS_WIRE || ctx->resident.flagged) {  // the import reads them from the native staging
    const int up = upload_native(ctx, nullptr, 0, scalars, n * 32);
    return up ? up : g1_msm_fixed_base_device(ctx, ctx->native.native_scalars(), n, out_xy);
  }
  int rc = h2d_staged(ctx, ctx->d_raw_scalars, scalars, n * 32, (size_t)ctx->cap * 96);
  if (rc) return rc;
  return g1_msm_fixed_base_device(ctx, ctx->d_raw_scalars, n, out_xy);
}

// Windows [win_begin, win_begin + win_count) of a G1 MSM; the records go to a host buffer, a device buffer, or both.
int window_partials(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin, uint32_t win_count,
                           uint8_t* host_out, void* dev_out) {
  int rc = check_args(ctx, d_points, d_scalars, n, true);
  if (rc) return rc;
  if (win_count == 0 || win_begin >= MSM377_NUM_WINDOWS || win_count > MSM377_NUM_WINDOWS - win_begin) {
    ctx->err = "window range outside 0..16";
    return MSM377_EINVAL;
  }
  if ((uintptr_t)dev_out & 15) {
    ctx->err = "device output pointer must be 16-byte aligned";
    return MSM377_EINVAL;
  }
  const size_t bytes = (size_t)win_count * MSM377_G1_WINDOW_PARTIAL_BYTES;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n == 0) {  // identity partials: ZZ = 0 everywhere
    if (host_out) memset(host_out, 0, bytes);
    if (dev_out) HIP_TRY(ctx, hipMemset(dev_out, 0, bytes));
    return MSM377_OK;
  }
  ctx->resident.clear();
  rc = import_inputs(ctx, &d_points, &d_scalars, n);  // (native input forms only)
  if (rc) return rc;
  // The records are complete in ctx->d_partials (slot 0) once the call's completion event has fired; the copy
  // to the caller's device buffer rides the same stream and the call returns with that stream idle, so a
  // collective on any other stream may read the buffer.
  auto deliver = [&]() -> int {
    if (host_out) memcpy(host_out, ctx->h_partials, bytes);
    if (dev_out) {
      HIP_TRY(ctx, hipMemcpyAsync(dev_out, ctx->d_partials, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MSM377_OK;
  };
  Phase ph;
  ph.plan = plan_equal16(TE_TAIL, win_count);  // (a shard of sixteen equal windows; the records go to the caller, no tail here)
  if (ctx->knobs.g1_form == 1) {  // twisted Edwards form; k_gather_partials tags the records (fp64_host.hpp TE_RECORD_TAG)
    // Affine base records (7-product additions, batched inversion) once a point takes part in enough additions to pay for
    // its ~9 extra conversion products: windows x points >= 2^24 -- e.g. the 8 windows a rank of a 2-GPU run owns at 2^21
    // points and more, the 2 of an 8-GPU run at 2^23 (msm377_g1_msm_device: 16 windows, n >= 2^20).
    const bool affine = ctx->knobs.te_affine_msm && n >= ctx->knobs.affine_min_points / 4 && (uint64_t)win_count * n >= 16 * ctx->knobs.affine_min_points;
    if (affine) {
      rc = affine_convert_begin(ctx, (const uint32_t*)d_points, n);
      if (rc) return rc;
      ctx->before_accumulate = [ctx, n]() -> int { return affine_convert_finish(ctx, ctx->d_bases, n); };
      rc = enqueue_windows<TeDev, TeAffBase>(ctx, (const uint32_t*)d_scalars, n, win_begin, 0, ph);
      ctx->before_accumulate = nullptr;
    } else {
      rc = convert_bases<TeDev>(ctx, (const uint32_t*)d_points, n);
      if (rc) return rc;
      rc = enqueue_windows<TeDev>(ctx, (const uint32_t*)d_scalars, n, win_begin, 0, ph);
    }
    if (rc == MSM377_OK) rc = wait_windows(ctx, 0);
    if (rc) return rc;
    if ((ctx->h_err[0] & ERR_TE_ANY) == 0) {
      rc = collect_windows(ctx, 0);
      return rc ? rc : deliver();
    }
    note_fallback(ctx, (uint32_t)(ctx->h_err[0] & ERR_TE_ANY));
    // an exceptional case of the Edwards law in THESE windows: they alone rerun below, untagged
  }
  rc = convert_bases<G1Dev>(ctx, (const uint32_t*)d_points, n);
  if (rc == MSM377_OK) rc = enqueue_windows<G1Dev>(ctx, (const uint32_t*)d_scalars, n, win_begin, 0, ph);
  if (rc == MSM377_OK) rc = wait_windows(ctx, 0);
  if (rc == MSM377_OK) rc = collect_windows(ctx, 0);
  return rc ? rc : deliver();
}

int g1_glv_window_partials_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin,
                                         uint32_t win_count, uint8_t* partials_out) {
  if (!partials_out) return MSM377_EINVAL;
  int rc = check_args(ctx, d_points, d_scalars, n, true);
  if (rc) return rc;
  if (win_count == 0 || win_begin >= GLV_WINDOWS || win_count > GLV_WINDOWS - win_begin) {
    ctx->err = "GLV window range outside 0..8";
    return MSM377_EINVAL;
  }
  if (n == 0) {
    memset(partials_out, 0, (size_t)win_count * MSM377_G1_WINDOW_PARTIAL_BYTES);
    return MSM377_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->resident.clear();
  rc = import_inputs(ctx, &d_points, &d_scalars, n);  // (native input forms only)
  if (rc) return rc;
  rc = convert_bases_g1(ctx, (const uint32_t*)d_points, n, true);
  if (rc) return rc;
  Phase ph;
  ph.plan = plan_glv8(win_count);
  rc = enqueue_windows<G1Dev>(ctx, (const uint32_t*)d_scalars, n, win_begin, 0, ph);
  if (rc == MSM377_OK) rc = wait_windows(ctx, 0);
  if (rc) return rc;
  if (geometry_refused(ph.plan, ctx->h_err[0])) {
    ctx->err = "a scalar is outside the GLV range; use the plain window path";
    return MSM377_EGLVRANGE;
  }
  rc = collect_windows(ctx, 0);
  if (rc) return rc;
  memcpy(partials_out, ctx->h_partials, (size_t)win_count * MSM377_G1_WINDOW_PARTIAL_BYTES);
  return MSM377_OK;
}

// ---- the batch calls (include/msm377.h: fixed-base, multi-base, Edwards-BLS12, row commitments on both curves, variable-base, pairwise) ----
// Their entry points over one machinery:
//   normalise          the stash -> affine records of a form, three launches, on either curve
//   build_mul_tables   ONE table builder: row bases, then the concatenated records in passes of at most BM_CHUNK
//   ensure_mul_tables  ONE keeper of the table slots: which (base, width) keys are missing, and when a slot is valid
//   batch_device_call  ONE flow of a device call: the checks in their order, the scratch, the passes, the one host wait
//   HostStage          ONE staging of a host-buffer call: the parts of a piece in one device allocation
// Everything runs on ctx->stream, launch after launch; the one host wait of a warm call is the synchronisation at its end.
namespace {

// The scratch of one chunk: fixed sizes, whatever n and the context's capacity are.
int bm_ensure_scratch(msm377_ctx* ctx) {
  BatchMulState& bm = ctx->bm;
  int rc = bm_alloc(ctx, &bm.stash, (size_t)BM_PIECES * BM_CHUNK * 16);
  if (!rc) rc = bm_alloc(ctx, &bm.trees, (size_t)BM_CHUNK_BLOCKS * BM_TREE_WORDS * 4);
  if (!rc) rc = bm_alloc(ctx, &bm.block_prod, (size_t)BM_CHUNK_BLOCKS * 13 * 4);
  if (!rc) rc = bm_alloc(ctx, &bm.block_inv, (size_t)BM_CHUNK_BLOCKS * 13 * 4);
  if (!rc) rc = bm_alloc(ctx, &bm.row_bases, (size_t)(bm_windows(BM_MIN_WIDTH) + 1) * BM_REC_WORDS * 4);
  if (!rc) rc = bm_alloc(ctx, &bm.base_wire, 96);
  return rc;
}

// ---- what the stash holds, for msm377_read_walk_stash / msm377_g1_read_walk_tables (context.hpp WalkLayout) ----
// forget_walk: every batch call starts with it (the two argument checks that open each of them) and so do
// msm377_g1_set_generators and msm377_ed_set_generators: from here on the stash is no longer what the last description said.  note_walk: beside a
// pass's walk launch, from the launch's own arguments.  batch_device_call adds the pass (n, offset, length) and marks the
// description valid behind the call's one wait.
void forget_walk(msm377_ctx* ctx) { ctx->last.walk.valid = false; }

void note_walk(msm377_ctx* ctx, uint32_t kind, uint32_t form, uint32_t width, uint32_t k, uint32_t segments = 1, uint64_t stride = 0, uint32_t tables = 0) {
  WalkLayout& wl = ctx->last.walk;
  wl.info = msm377_walk_stash_info{};
  wl.info.kind = kind;
  wl.info.form = form;
  wl.info.point_words = form == MSM377_WALK_FORM_ED ? EDBM_POINT_PIECES * 4 : BM_POINT_PIECES * 4;
  wl.info.product_words = form == MSM377_WALK_FORM_ED ? 9 : 13;
  wl.info.product_pad = (form == MSM377_WALK_FORM_ED ? (EDBM_PIECES - EDBM_POINT_PIECES) * 4 : (BM_PIECES - BM_POINT_PIECES) * 4) - wl.info.product_words;
  wl.info.width = width;
  wl.info.k = k;
  wl.info.segments = segments;
  wl.info.stride = stride;
  wl.tables = msm377_walk_tables_info{};
  wl.tables.tables = tables;
  wl.tables.entries = tables ? (uint32_t)BMV_ENTRIES : 0;
  wl.d_tables = tables ? ctx->bm.var_table : nullptr;  // (the k-term call names its own behind this)
}

// What the normalisation, the builder and the pointer check need to know of a curve: the bytes of a base on the wire, the
// build kernels, the normalisation kernels and the form of a table record.  The hot kernels are each call's own.
struct G1Mul {
  static constexpr size_t WIRE = 96;
  static constexpr uint32_t FORM_TABLE = BM_FORM_TABLE;
  static constexpr const char* MISALIGNED = "device pointers must be 16-byte aligned (8-byte for mont_flag records)";
  static constexpr auto row_bases = k_bmm_row_bases;
  static constexpr auto entries = k_bmm_entries;
  static constexpr auto up = k_bm_up;
  static constexpr auto across = k_bm_across;
  static void down(hipStream_t s, uint32_t blocks, uint32_t form, const uint4* stash, uint64_t m, const uint32_t* trees, const uint32_t* inv, uint8_t* out, uint8_t* out_inf) {
    const auto k = form == MSM377_POINTS_WIRE ? k_bm_down<MSM377_POINTS_WIRE> : form == MSM377_POINTS_MONT_FLAG ? k_bm_down<MSM377_POINTS_MONT_FLAG> : k_bm_down<BM_FORM_TABLE>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(BM_THREADS), 0, s, stash, m, trees, inv, out, out_inf);
  }
};
struct EdMul {
  static constexpr size_t WIRE = 64;
  static constexpr uint32_t FORM_TABLE = EDBM_FORM_TABLE;
  static constexpr const char* MISALIGNED = "device pointers must be 16-byte aligned";
  static constexpr auto row_bases = k_edbm_row_bases;
  static constexpr auto entries = k_edbm_entries;
  static constexpr auto up = k_edbm_up;
  static constexpr auto across = k_edbm_across;
  static void down(hipStream_t s, uint32_t blocks, uint32_t form, const uint4* stash, uint64_t m, const uint32_t* trees, const uint32_t* inv, uint8_t* out, uint8_t*) {
    const auto k = form == EDBM_FORM_WIRE ? k_edbm_down<EDBM_FORM_WIRE> : k_edbm_down<EDBM_FORM_TABLE>;  // no flag array: the identity is the record (0, 1)
    hipLaunchKernelGGL(k, dim3(blocks), dim3(BM_THREADS), 0, s, stash, m, trees, inv, out);
  }
};

// The m <= BM_CHUNK points the stash holds -> records of `form` at d_out (G1: and their flags at d_out_inf): three launches.
template <class MC>
int normalise(msm377_ctx* ctx, uint64_t m, uint32_t form, void* d_out, uint8_t* d_out_inf) {
  BatchMulState& bm = ctx->bm;
  const uint32_t blocks = (uint32_t)((m + BM_BLOCK - 1) / BM_BLOCK);
  uint4* stash = reinterpret_cast<uint4*>(bm.stash);
  hipLaunchKernelGGL(MC::up, dim3(blocks), dim3(BM_THREADS), 0, ctx->stream, stash, m, bm.trees, bm.block_prod);
  hipLaunchKernelGGL(MC::across, dim3(1), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)bm.block_prod, blocks, bm.block_inv);
  MC::down(ctx->stream, blocks, form, stash, m, bm.trees, bm.block_inv, (uint8_t*)d_out, d_out_inf);
  HIP_TRY(ctx, hipGetLastError());
  return MSM377_OK;
}

// A whole build of the window tables of m bases at width c, all of them side by side: the bases' wire bytes up, ONE
// row-base launch (a workgroup per base: the 256 dependent doublings of the last row are paid once per build), then the
// entries of the m tables as one run of records cut into passes of at most BM_CHUNK, wherever the cut falls.  A pass's
// records go straight to their place in `into` where the tables are one allocation; else (`slots`: table b is
// slots[b]->table, its own allocation) through a staging buffer -- the down kernel writes a pass as one run -- and from
// there, piece by piece, into the tables the pass covers (device copies of at most 64 MB beside a 6 ms chain of
// doublings).  row_bases and d_wire: device scratch for m x (W + 1) records and m bases.  Returns behind ONE wait for
// all of it, the staging given back: the tables are there, or the call failed (rc, then the copy, then the wait).
template <class MC>
int build_mul_tables(msm377_ctx* ctx, const uint8_t* wire, uint32_t m, int c, uint32_t* row_bases, uint32_t* d_wire, uint32_t* into, MulTableSlot* const* slots) {
  const uint64_t records = bm_table_records((uint32_t)c), rows = (uint64_t)bm_windows(c) + 1, total = records * m;
  uint32_t* staging = nullptr;
  int rc = into ? MSM377_OK : bm_alloc(ctx, &staging, (size_t)std::min<uint64_t>(total, BM_CHUNK) * BM_REC_WORDS * 4);
  if (rc) return rc;
  uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
  hipError_t e = hipMemcpyAsync(d_wire, wire, (size_t)m * MC::WIRE, hipMemcpyHostToDevice, ctx->stream);  // (pageable memory: staged before the call returns)
  if (e == hipSuccess) {
    hipLaunchKernelGGL(MC::row_bases, dim3(m), dim3(64), 0, ctx->stream, (const uint32_t*)d_wire, (uint32_t)c, stash);
    rc = normalise<MC>(ctx, rows * m, MC::FORM_TABLE, row_bases, nullptr);
  }
  for (uint64_t first = 0; first < total && !rc && e == hipSuccess; first += BM_CHUNK) {
    const uint64_t count = std::min<uint64_t>(BM_CHUNK, total - first);
    hipLaunchKernelGGL(MC::entries, dim3((unsigned)((count + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)row_bases, (uint32_t)c, first, count, stash);
    rc = normalise<MC>(ctx, count, MC::FORM_TABLE, into ? into + first * BM_REC_WORDS : staging, nullptr);
    for (uint64_t g = first; !into && g < first + count && !rc && e == hipSuccess;) {  // the pieces of this pass, one per table it covers
      const uint64_t b = g / records, t = g - b * records, len = std::min<uint64_t>(records - t, first + count - g);
      e = hipMemcpyAsync(slots[b]->table + t * BM_REC_WORDS, staging + (g - first) * BM_REC_WORDS, (size_t)len * BM_REC_WORDS * 4, hipMemcpyDeviceToDevice, ctx->stream);
      g += len;
    }
  }
  const hipError_t waited = hipStreamSynchronize(ctx->stream);  // the wire bytes are the caller's; and the staging goes back
  ctx->own.release(staging);
  if (rc) return rc;
  HIP_TRY(ctx, e);
  HIP_TRY(ctx, waited);
  return MSM377_OK;
}

// The window tables of (base j, c) in slot[j], j < k: a slot whose key is that stays; every other one is rebuilt, all of
// them in ONE build.  A build drops the old tables FIRST and marks the new ones valid as its last step, behind the
// build's wait: a failed build leaves no table behind.  contiguous: the one slot (k = 1) takes its records directly.
template <class MC>
int ensure_mul_tables(msm377_ctx* ctx, MulTableSlot* slot, const uint8_t* bases_xy, uint32_t k, int c, uint32_t* row_bases, uint32_t* d_wire, bool contiguous, uint64_t* builds) {
  MulTableSlot* missing[MSM377_MUL_MAX_BASES];
  uint8_t wire[MSM377_MUL_MAX_BASES * 96];
  uint32_t m = 0;
  for (uint32_t j = 0; j < k; j++) {
    const uint8_t* base = bases_xy + (size_t)j * MC::WIRE;
    if (slot[j].valid && slot[j].width == c && memcmp(slot[j].key, base, MC::WIRE) == 0) continue;
    memcpy(wire + (size_t)m * MC::WIRE, base, MC::WIRE);
    missing[m++] = &slot[j];
  }
  if (m == 0) return MSM377_OK;
  for (uint32_t b = 0; b < m; b++) missing[b]->valid = false;
  const uint64_t records = bm_table_records((uint32_t)c);
  int rc = MSM377_OK;
  for (uint32_t b = 0; b < m && !rc; b++) {
    MulTableSlot& sl = *missing[b];
    if (sl.table_cap >= records) continue;
    ctx->own.release(sl.table);
    sl.table = nullptr;
    sl.table_cap = 0;
    rc = bm_alloc(ctx, &sl.table, (size_t)records * BM_REC_WORDS * 4);
    if (!rc) sl.table_cap = records;
  }
  if (!rc) rc = build_mul_tables<MC>(ctx, wire, m, c, row_bases, d_wire, contiguous ? missing[0]->table : nullptr, missing);
  if (rc) return rc;
  for (uint32_t b = 0; b < m; b++) {
    memcpy(missing[b]->key, wire + (size_t)b * MC::WIRE, MC::WIRE);  // (the rest of a 64-byte key stays zero)
    missing[b]->width = c;
    missing[b]->valid = true;
    ++*builds;
  }
  return MSM377_OK;
}

// The slots of the multi-base calls, G1 or Edwards-BLS12, over the row-base scratch the two share.
template <class MC>
int ensure_multi_tables(msm377_ctx* ctx, MulTableSlot* slot, const uint8_t* bases_xy, uint32_t k, int c, uint64_t* builds) {
  BatchMulMultiState& mm = ctx->bmm;
  int rc = bm_alloc(ctx, &mm.row_bases, (size_t)MSM377_MUL_MAX_BASES * (bm_windows(BM_MIN_WIDTH) + 1) * BM_REC_WORDS * 4);
  if (!rc) rc = bm_alloc(ctx, &mm.bases_wire, (size_t)MSM377_MUL_MAX_BASES * 96);
  return rc ? rc : ensure_mul_tables<MC>(ctx, slot, bases_xy, k, c, mm.row_bases, mm.bases_wire, false, builds);
}

// ---- argument checks: nothing is allocated, launched or changed before they pass ----
int bm_check_form(msm377_ctx* ctx, uint32_t out_form) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // every G1 batch call, device or host buffers, opens with this check
  if (out_form == MSM377_POINTS_WIRE || out_form == MSM377_POINTS_MONT_FLAG) return MSM377_OK;
  ctx->err = out_form == MSM377_POINTS_MONT ? "batch_mul outputs need a form that can say \"identity\": MSM377_POINTS_WIRE or MSM377_POINTS_MONT_FLAG" : "unknown output form";
  return MSM377_EINVAL;
}

// k and the strides of a k x n scalar matrix.
int check_shape(msm377_ctx* ctx, uint32_t k, uint32_t k_max, const char* message, uint64_t out_stride, uint64_t base_stride) {
  if (k < 1 || k > k_max) {
    ctx->err = message;
    return MSM377_EINVAL;
  }
  if (!out_stride || !base_stride || (out_stride & 31) || (base_stride & 31)) {
    ctx->err = "out_stride and base_stride are byte counts: non-zero multiples of 32";
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

int null_pointer(msm377_ctx* ctx) {
  ctx->err = "null pointer";
  return MSM377_EINVAL;
}

// The pointers of a device call: none null (host: the bases, which live in host memory); scalars and records of 64 or 96
// bytes 16-byte aligned, 104-byte records 8-byte aligned.
template <class MC>
int check_pointers(msm377_ctx* ctx, std::initializer_list<const void*> host, std::initializer_list<const void*> scalars, std::initializer_list<const void*> points, size_t in_stride,
                   const void* out, size_t out_stride) {
  const auto mask = [](size_t stride) { return (uintptr_t)(stride == 104 ? 7 : 15); };
  bool null = !out, misaligned = ((uintptr_t)out & mask(out_stride)) != 0;
  for (const void* h : host) null |= !h;
  for (const void* s : scalars) null |= !s, misaligned |= ((uintptr_t)s & 15) != 0;
  for (const void* p : points) null |= !p, misaligned |= ((uintptr_t)p & mask(in_stride)) != 0;
  if (null) return null_pointer(ctx);
  if (misaligned) {
    ctx->err = MC::MISALIGNED;
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

bool bm_base_canonical(const uint8_t base_xy[96]) {
  uint64_t lim[2][6];
  memcpy(lim, base_xy, 96);
  return !Fp64::geq_p(lim[0]) && !Fp64::geq_p(lim[1]);
}

int bmm_check_bases(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k) {
  for (uint32_t j = 0; j < k; j++)
    if (!bm_base_canonical(bases_xy + (size_t)j * 96)) {
      ctx->err = "a base has a coordinate that is not below p";
      return MSM377_EINVAL;
    }
  return MSM377_OK;
}

size_t point_stride(uint32_t form) { return form == MSM377_POINTS_MONT_FLAG ? 104 : 96; }
uint32_t scalars_mont(const msm377_ctx* ctx) { return ctx->scalar_form == MSM377_SCALARS_MONT ? 1u : 0u; }
dim3 bm_grid(uint64_t m) { return dim3((unsigned)((m + BM_THREADS - 1) / BM_THREADS)); }

// ---- the flow of a device call ----
// early: the verdict of the form and shape checks, which come first and hold for n == 0 too; then n == 0 (nothing to do,
// whatever the pointers); then check(): the pointers, and what is checked behind them (bases below p, a resident set).
// Only then the device: the scratch, prepare() (the call's tables, its width), and the passes of at most pass_len outputs
// -- pass(off, m) queues what leaves m points in the stash, the normalisation writes them as out_form records of
// out_stride bytes (and flags) at output `off`.  ONE host wait at the end; a failure in the flow is reported before what
// the wait says.
template <class MC, class Check, class Prepare, class Pass>
int batch_device_call(msm377_ctx* ctx, int early, uint64_t n, uint64_t pass_len, uint32_t out_form, void* d_out, size_t out_stride, uint8_t* d_out_inf, Check&& check, Prepare&& prepare,
                      Pass&& pass) {
  if (early || n == 0) return early;
  int rc = check();
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = bm_ensure_scratch(ctx);
  if (!rc) rc = prepare();
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  for (uint64_t off = 0; off < n && !rc; off += pass_len) {
    const uint64_t m = std::min<uint64_t>(pass_len, n - off);
    rc = pass(off, m);  // (notes what it launched: note_walk)
    if (!rc) rc = normalise<MC>(ctx, m, out_form, (uint8_t*)d_out + off * out_stride, d_out_inf ? d_out_inf + off : nullptr);
    WalkLayout& wl = ctx->last.walk;  // the pass just queued: the last one is what the stash holds at the end
    wl.info.n = n;
    wl.info.pass_offset = off;
    wl.info.m = m;
    wl.tables.m = m;
  }
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  HIP_TRY(ctx, e);
  ctx->last.walk.valid = true;
  return MSM377_OK;
}
const auto nothing_to_prepare = [] { return MSM377_OK; };

// ---- the staging of a host-buffer call ----
// The parts of one piece -- the inputs in the caller's order, then the records, then the flags -- at 16-byte aligned
// offsets of ONE device allocation that lives as long as this object.  rc: MSM377_ENOMEM (and ctx->err = oom) if there
// is no memory for it.
struct HostStage {
  msm377_ctx* ctx;
  uint8_t* d_io = nullptr;
  std::vector<size_t> offset;
  std::vector<uint8_t> rows;  // repack_rows' row-major copy of a piece
  int rc = MSM377_OK;
  HostStage(msm377_ctx* c, std::initializer_list<size_t> inputs, size_t record_bytes, size_t flag_bytes, const char* oom) : ctx(c) {
    size_t total = 0;
    const auto add = [&](size_t bytes) { offset.push_back(total), total += (bytes + 15) & ~(size_t)15; };
    for (size_t bytes : inputs) add(bytes);
    add(record_bytes), add(flag_bytes);
    if (hipMalloc((void**)&d_io, total) == hipSuccess) return;
    (void)hipGetLastError();
    d_io = nullptr;
    ctx->err = oom;
    rc = MSM377_ENOMEM;
  }
  ~HostStage() { (void)hipFree(d_io); }
  HostStage(const HostStage&) = delete;
  uint8_t* part(size_t i) const { return d_io + offset[i]; }
  uint8_t* records() const { return part(offset.size() - 2); }
  uint8_t* flags() const { return part(offset.size() - 1); }
  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* what) const { return hip_ok(ctx, hipMemcpy(dst, src, bytes, kind), what) ? MSM377_OK : MSM377_EHIP; }
  int up(size_t i, const uint8_t* src, size_t bytes, const char* what) const { return copy(part(i), src, bytes, hipMemcpyHostToDevice, what); }
  int down_records(uint8_t* dst, size_t bytes) const { return copy(dst, records(), bytes, hipMemcpyDeviceToHost, "hipMemcpy(records)"); }
  int down_flags(uint8_t* dst, size_t bytes) const { return copy(dst, flags(), bytes, hipMemcpyDeviceToHost, "hipMemcpy(flags)"); }
  // The loop over pieces of at most `piece` outputs: load(off, m) uploads the inputs of outputs off .. off + m and runs the
  // device call on them; their records of `stride` bytes and, where the caller wants them, their flags come down.
  template <class Load>
  int run(uint64_t n, uint64_t piece, uint8_t* out_points, size_t stride, uint8_t* out_inf, Load&& load) const {
    int rc = MSM377_OK;
    for (uint64_t off = 0; off < n && !rc; off += piece) {
      const uint64_t m = std::min<uint64_t>(piece, n - off);
      rc = load(off, m);
      if (!rc) rc = down_records(out_points + off * stride, m * stride);
      if (!rc && out_inf) rc = down_flags(out_inf + off, m);
    }
    if (rc) forget_walk(ctx);  // (a download that failed behind a device call that did not)
    return rc;
  }
  // Rows off .. off + m of the caller's k x n matrix (s_ij at scalars + i out_stride + j base_stride), row-major, into part i.
  int repack_rows(size_t i, const uint8_t* scalars, uint64_t off, uint64_t m, uint32_t k, uint64_t out_stride, uint64_t base_stride) {
    rows.resize((size_t)m * k * 32);
    for (uint64_t r = 0; r < m; r++)
      for (uint32_t j = 0; j < k; j++) memcpy(rows.data() + ((size_t)r * k + j) * 32, scalars + (off + r) * out_stride + (uint64_t)j * base_stride, 32);
    return up(i, rows.data(), rows.size(), "hipMemcpy(scalars)");
  }
};

// One width for the whole host-buffer call, whatever its pieces' sizes: the rule's value for the CALL's n stands in for a
// width that nobody forced, and what was there comes back on every way out.
struct OneWidth {
  int& window;
  const int forced;
  OneWidth(msm377_ctx* ctx, int by_rule) : window(ctx->bm.window), forced(window) {
    if (!forced) window = by_rule;
  }
  ~OneWidth() { window = forced; }
};

}  // namespace

// ---- fixed-base batch multiplication (include/msm377.h "fixed-base batch multiplication"; kernels/batch_mul.hpp) ----
int g1_batch_mul_device(msm377_ctx* ctx, const uint8_t base_xy[96], const void* d_scalars, uint64_t n, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf) {
  int c = 0;
  const size_t stride = point_stride(out_form);
  const auto check = [&]() -> int {
    const int rc = check_pointers<G1Mul>(ctx, {base_xy}, {d_scalars}, {}, 96, d_out_points, stride);
    if (rc || bm_base_canonical(base_xy)) return rc;
    ctx->err = "the base has a coordinate that is not below p";
    return MSM377_EINVAL;
  };
  const auto prepare = [&]() -> int {  // the table of (base, c): kept until either key changes
    BatchMulState& bm = ctx->bm;
    c = bm.window ? bm.window : batch_mul_rule(n);
    const int rc = ensure_mul_tables<G1Mul>(ctx, &bm.single, base_xy, 1, c, bm.row_bases, bm.base_wire, true, &bm.builds);
    if (!rc) bm.last_window = c;
    return rc;
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {
    hipLaunchKernelGGL(k_bm_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)ctx->bm.single.table, (const uint32_t*)d_scalars + off * 8, m, (uint32_t)c, scalars_mont(ctx),
                       reinterpret_cast<uint4*>(ctx->bm.stash));
    note_walk(ctx, MSM377_WALK_BATCH_MUL, MSM377_WALK_FORM_XYZZ, (uint32_t)c, 1);
    return MSM377_OK;
  };
  return batch_device_call<G1Mul>(ctx, bm_check_form(ctx, out_form), n, BM_CHUNK, out_form, d_out_points, stride, d_out_inf, check, prepare, pass);
}

// Host buffers: scalars up, records (and flags) down, in pieces of at most a chunk.
int g1_batch_mul(msm377_ctx* ctx, const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  int rc = bm_check_form(ctx, out_form);
  if (rc || n == 0) return rc;
  if (!base_xy || !scalars || !out_points) return null_pointer(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t stride = point_stride(out_form);
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK);
  HostStage io(ctx, {(size_t)piece * 32}, (size_t)piece * stride, piece, "out of device memory for the batch multiplication staging");
  if (io.rc) return io.rc;
  OneWidth width(ctx, batch_mul_rule(n));
  return io.run(n, piece, out_points, stride, out_inf, [&](uint64_t off, uint64_t m) -> int {
    const int up = io.up(0, scalars + off * 32, m * 32, "hipMemcpy(scalars)");
    return up ? up : g1_batch_mul_device(ctx, base_xy, io.part(0), m, out_form, io.records(), io.flags());
  });
}

// ---- multi-base batch multiplication (include/msm377.h "multi-base batch multiplication"; kernels/batch_mul_multi.hpp) ----
int g1_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                              void* d_out_points, uint8_t* d_out_inf) {
  int early = bm_check_form(ctx, out_form), c = 0;
  if (!early) early = check_shape(ctx, k, MSM377_MUL_MAX_BASES, "k is 1 to MSM377_MUL_MAX_BASES bases", out_stride, base_stride);
  BmmTables tables = {};
  const size_t stride = point_stride(out_form);
  const auto check = [&]() -> int {
    const int rc = check_pointers<G1Mul>(ctx, {bases_xy}, {d_scalars}, {}, 96, d_out_points, stride);
    return rc ? rc : bmm_check_bases(ctx, bases_xy, k);
  };
  const auto prepare = [&]() -> int {
    c = ctx->bm.window ? ctx->bm.window : batch_mul_multi_rule(n, k);
    const int rc = ensure_multi_tables<G1Mul>(ctx, ctx->bmm.slot, bases_xy, k, c, &ctx->bmm.builds);
    if (rc) return rc;
    ctx->bm.last_window = c;
    for (uint32_t j = 0; j < k; j++) tables.t[j] = ctx->bmm.slot[j].table;
    return MSM377_OK;
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {  // row `off` of the CALL's layout: the strides are the call's, whatever the pass's length
    hipLaunchKernelGGL(k_bmm_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, tables, (const uint8_t*)d_scalars + off * out_stride, m, k, out_stride, base_stride, (uint32_t)c,
                       scalars_mont(ctx), reinterpret_cast<uint4*>(ctx->bm.stash));
    note_walk(ctx, MSM377_WALK_BATCH_MUL_MULTI, MSM377_WALK_FORM_XYZZ, (uint32_t)c, k);
    return MSM377_OK;
  };
  return batch_device_call<G1Mul>(ctx, early, n, BM_CHUNK, out_form, d_out_points, stride, d_out_inf, check, prepare, pass);
}

// Host buffers: each piece of at most 2^20 scalars (2^20 / k outputs) repacked row-major on the host, up, records (and
// flags) down.
int g1_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                       uint8_t* out_points, uint8_t* out_inf) {
  int rc = bm_check_form(ctx, out_form);
  if (!rc) rc = check_shape(ctx, k, MSM377_MUL_MAX_BASES, "k is 1 to MSM377_MUL_MAX_BASES bases", out_stride, base_stride);
  if (rc || n == 0) return rc;
  if (!bases_xy || !scalars || !out_points) return null_pointer(ctx);
  rc = bmm_check_bases(ctx, bases_xy, k);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t stride = point_stride(out_form);
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK / k);
  HostStage io(ctx, {(size_t)piece * k * 32}, (size_t)piece * stride, piece, "out of device memory for the batch multiplication staging");
  if (io.rc) return io.rc;
  OneWidth width(ctx, batch_mul_multi_rule(n, k));
  return io.run(n, piece, out_points, stride, out_inf, [&](uint64_t off, uint64_t m) -> int {
    const int up = io.repack_rows(0, scalars, off, m, k, out_stride, base_stride);
    return up ? up : g1_batch_mul_multi_device(ctx, bases_xy, k, io.part(0), m, (uint64_t)k * 32, 32, out_form, io.records(), io.flags());
  });
}

// ---- Edwards-BLS12 batch multiplication (include/msm377.h "Edwards-BLS12 batch multiplication"; kernels/ed_batch_mul.hpp) ----
namespace {

int edbm_check_args(msm377_ctx* ctx, uint32_t k, uint64_t out_stride, uint64_t base_stride) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // as bm_check_form: both Edwards-BLS12 batch calls open here
  return check_shape(ctx, k, MSM377_MUL_MAX_BASES, "k is 1 to MSM377_MUL_MAX_BASES bases", out_stride, base_stride);
}

int edbm_check_bases(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k) {
  if (ed_batch_mul_bases_ok(bases_xy, k)) return MSM377_OK;
  ctx->err = "a base has a coordinate that is not below q or is not on the curve";
  return MSM377_EINVAL;
}

}  // namespace

int ed_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, void* d_out_points) {
  int c = 0;
  EdbmTables tables = {};
  const auto check = [&]() -> int {
    const int rc = check_pointers<EdMul>(ctx, {bases_xy}, {d_scalars}, {}, 64, d_out_points, 64);
    return rc ? rc : edbm_check_bases(ctx, bases_xy, k);
  };
  const auto prepare = [&]() -> int {
    c = ctx->bm.window ? ctx->bm.window : batch_mul_multi_rule(n, k);
    const int rc = ensure_multi_tables<EdMul>(ctx, ctx->edbm.slot, bases_xy, k, c, &ctx->edbm.builds);
    if (rc) return rc;
    ctx->bm.last_window = c;
    for (uint32_t j = 0; j < k; j++) tables.t[j] = ctx->edbm.slot[j].table;
    return MSM377_OK;
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {  // row `off` of the CALL's layout, as on G1
    hipLaunchKernelGGL(k_edbm_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, tables, (const uint8_t*)d_scalars + off * out_stride, m, k, out_stride, base_stride, (uint32_t)c,
                       reinterpret_cast<uint4*>(ctx->bm.stash));
    note_walk(ctx, MSM377_WALK_ED_BATCH_MUL_MULTI, MSM377_WALK_FORM_ED, (uint32_t)c, k);
    return MSM377_OK;
  };
  return batch_device_call<EdMul>(ctx, edbm_check_args(ctx, k, out_stride, base_stride), n, BM_CHUNK, EDBM_FORM_WIRE, d_out_points, 64, nullptr, check, prepare, pass);
}

// Host buffers: each piece of at most 2^20 scalars repacked row-major on the host, up, records down.
int ed_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  int rc = edbm_check_args(ctx, k, out_stride, base_stride);
  if (rc || n == 0) return rc;
  if (!bases_xy || !scalars || !out_points) return null_pointer(ctx);
  rc = edbm_check_bases(ctx, bases_xy, k);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK / k);
  HostStage io(ctx, {(size_t)piece * k * 32}, (size_t)piece * 64, 0, "out of device memory for the batch multiplication staging");
  if (io.rc) return io.rc;
  OneWidth width(ctx, batch_mul_multi_rule(n, k));
  return io.run(n, piece, out_points, 64, nullptr, [&](uint64_t off, uint64_t m) -> int {
    const int up = io.repack_rows(0, scalars, off, m, k, out_stride, base_stride);
    return up ? up : ed_batch_mul_multi_device(ctx, bases_xy, k, io.part(0), m, (uint64_t)k * 32, 32, io.records());
  });
}

// ---- row commitments (include/msm377.h "row commitments"; kernels/commit_rows.hpp, commit_rows_plan.hpp) ----
namespace {

void cr_drop_set(msm377_ctx* ctx) {
  GeneratorSet& gs = ctx->gens;
  gs.k = 0;
  gs.width = 0;
  ctx->own.release(gs.tables);
  gs.tables = nullptr;
}

int cr_check_set(msm377_ctx* ctx, uint32_t k) {
  if (!ctx->gens.valid()) {
    ctx->err = "no resident generator set: call msm377_g1_set_generators first";
    return MSM377_ESTATE;
  }
  if (k > ctx->gens.k) {
    ctx->err = "k is above the resident generator count";
    return MSM377_ESTATE;
  }
  return MSM377_OK;
}

}  // namespace

// The set is ONE allocation, table j at record j * bm_table_records(c): the builder writes every pass straight to its
// place, over row bases and wire bytes sized for k that live for the length of the build.
int g1_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy, uint32_t k, int window_bits) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // the build below goes through the stash
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  cr_drop_set(ctx);  // first, whatever follows: a call that fails leaves no set
  if (!gens_xy || k == 0) return MSM377_OK;
  const int c = window_bits ? window_bits : BM_NARROW_WIDTH;
  if (!batch_mul_width_supported(c)) {
    ctx->err = "window_bits is 8, 16 or 0 (= 8)";
    return MSM377_EINVAL;
  }
  if (k > MSM377_GEN_MAX || (c == BM_WIDE_WIDTH && k > MSM377_GEN_WIDE_MAX)) {
    ctx->err = "a set holds at most MSM377_GEN_MAX generators, MSM377_GEN_WIDE_MAX with 16-bit tables";
    return MSM377_EINVAL;
  }
  for (uint32_t j = 0; j < k; j++)
    if (!bm_base_canonical(gens_xy + (size_t)j * 96)) {
      ctx->err = "a generator has a coordinate that is not below p";
      return MSM377_EINVAL;
    }
  static_assert((uint64_t)MSM377_GEN_MAX * (bm_windows(8) + 1) <= BM_CHUNK && (uint64_t)MSM377_GEN_WIDE_MAX * (bm_windows(16) + 1) <= BM_CHUNK, "the row bases of a set are normalised in one chunk");
  GeneratorSet& gs = ctx->gens;
  uint32_t *row_bases = nullptr, *gens_wire = nullptr;
  int rc = bm_ensure_scratch(ctx);
  if (!rc) rc = bm_alloc(ctx, &gs.tables, (size_t)k * bm_table_records((uint32_t)c) * BM_REC_WORDS * 4);
  if (!rc) rc = bm_alloc(ctx, &row_bases, (size_t)k * (bm_windows(c) + 1) * BM_REC_WORDS * 4);
  if (!rc) rc = bm_alloc(ctx, &gens_wire, (size_t)k * 96);
  if (!rc) rc = build_mul_tables<G1Mul>(ctx, gens_xy, k, c, row_bases, gens_wire, gs.tables, nullptr);
  ctx->own.release(row_bases);  // (the build has waited for its launches)
  ctx->own.release(gens_wire);
  if (rc) {
    cr_drop_set(ctx);
    return rc;
  }
  gs.width = c;
  gs.k = k;
  return MSM377_OK;
}

int g1_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, void* d_out_points,
                          uint8_t* d_out_inf) {
  int early = bm_check_form(ctx, out_form);
  if (!early) early = check_shape(ctx, k, MSM377_GEN_MAX, "k is 1 to MSM377_GEN_MAX generators", out_stride, base_stride);
  const CommitRowsPlan plan = commit_rows_plan(early ? 1 : k);  // (a k that was refused is not planned for)
  const size_t stride = point_stride(out_form);
  const auto check = [&]() -> int {
    const int rc = check_pointers<G1Mul>(ctx, {}, {d_scalars}, {}, 96, d_out_points, stride);
    return rc ? rc : cr_check_set(ctx, k);
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {  // row `off` of the CALL's layout: the strides are the call's, whatever the pass's length
    const GeneratorSet& gs = ctx->gens;
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    const dim3 grid = bm_grid(m);
    const uint64_t part_stride = (uint64_t)grid.x * BM_THREADS;  // <= rows_per_pass, so segments * part_stride <= BM_CHUNK
    hipLaunchKernelGGL(k_cr_accumulate, dim3(grid.x, plan.segments), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)gs.tables, (const uint8_t*)d_scalars + off * out_stride, m, k,
                       plan.bases_per_segment, out_stride, base_stride, (uint32_t)gs.width, scalars_mont(ctx), part_stride, stash);
    if (plan.segments > 1) hipLaunchKernelGGL(k_cr_fold, grid, dim3(BM_THREADS), 0, ctx->stream, stash, m, plan.segments, part_stride);
    note_walk(ctx, MSM377_WALK_COMMIT_ROWS, MSM377_WALK_FORM_XYZZ, (uint32_t)gs.width, k, plan.segments, part_stride);
    return MSM377_OK;
  };
  return batch_device_call<G1Mul>(ctx, early, n, plan.rows_per_pass, out_form, d_out_points, stride, d_out_inf, check, nothing_to_prepare, pass);
}

// Host buffers: each piece of at most 2^20 scalars (2^20 / k rows) repacked row-major on the host, up, records (and
// flags) down.
int g1_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  int rc = bm_check_form(ctx, out_form);
  if (!rc) rc = check_shape(ctx, k, MSM377_GEN_MAX, "k is 1 to MSM377_GEN_MAX generators", out_stride, base_stride);
  if (rc || n == 0) return rc;
  if (!scalars || !out_points) return null_pointer(ctx);
  rc = cr_check_set(ctx, k);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t stride = point_stride(out_form);
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK / k);
  HostStage io(ctx, {(size_t)piece * k * 32}, (size_t)piece * stride, piece, "out of device memory for the row commitment staging");
  if (io.rc) return io.rc;
  return io.run(n, piece, out_points, stride, out_inf, [&](uint64_t off, uint64_t m) -> int {
    const int up = io.repack_rows(0, scalars, off, m, k, out_stride, base_stride);
    return up ? up : g1_commit_rows_device(ctx, io.part(0), m, k, (uint64_t)k * 32, 32, out_form, io.records(), io.flags());
  });
}

// ---- variable-base batch multiplication (include/msm377.h "variable-base batch multiplication"; kernels/batch_mul_var.hpp) ----
// Per pass of BMV_PASS points: the per-point tables through the stash and the normalisation, then the walk; the flow
// normalises again.  A pass reads its points before it writes its outputs, and passes cover disjoint index ranges:
// d_out_points == d_points is safe for records of equal size.
namespace {

bool bmv_stride_ok(uint32_t scalar_stride) { return scalar_stride == 0 || scalar_stride == 32; }

int bmv_check_args(msm377_ctx* ctx, uint32_t scalar_stride, uint32_t out_form) {
  const int rc = bm_check_form(ctx, out_form);
  if (rc) return rc;
  if (!bmv_stride_ok(scalar_stride)) {
    ctx->err = "scalar_stride is 32 (a scalar per point) or 0 (one scalar for all points)";
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

int bmv_ensure_table(msm377_ctx* ctx) { return bm_alloc(ctx, &ctx->bm.var_table, (size_t)BM_CHUNK * BM_REC_WORDS * 4); }

// [1..8] of m points of `form` into the stash at (e - 1) m + i.
void bmv_launch_table(msm377_ctx* ctx, uint32_t form, const uint8_t* pts, uint64_t m, uint4* stash) {
  const auto k = form == MSM377_POINTS_WIRE ? k_bmv_table<MSM377_POINTS_WIRE> : form == MSM377_POINTS_MONT ? k_bmv_table<MSM377_POINTS_MONT> : k_bmv_table<MSM377_POINTS_MONT_FLAG>;
  hipLaunchKernelGGL(k, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, pts, m, stash);
}

}  // namespace

int g1_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, void* d_out_points,
                            uint8_t* d_out_inf) {
  const int early = bmv_check_args(ctx, scalar_stride, out_form);
  const uint32_t form = early ? 0 : ctx->point_form, stride_words = scalar_stride / 4;
  const size_t in_stride = point_stride(form), out_stride = point_stride(out_form);
  const auto check = [&] { return check_pointers<G1Mul>(ctx, {}, {d_scalars}, {d_points}, in_stride, d_out_points, out_stride); };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    bmv_launch_table(ctx, form, (const uint8_t*)d_points + off * in_stride, m, stash);
    const int rc = normalise<G1Mul>(ctx, m * BMV_ENTRIES, BM_FORM_TABLE, ctx->bm.var_table, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bmv_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)ctx->bm.var_table, (const uint32_t*)d_scalars + off * stride_words, m, stride_words,
                       scalars_mont(ctx), stash);
    note_walk(ctx, MSM377_WALK_BATCH_MUL_VAR, MSM377_WALK_FORM_XYZZ, (uint32_t)BMV_WIDTH, 1, 1, 0, 1);
    return MSM377_OK;
  };
  return batch_device_call<G1Mul>(ctx, early, n, BMV_PASS, out_form, d_out_points, out_stride, d_out_inf, check, [&] { return bmv_ensure_table(ctx); }, pass);
}

// Host buffers: points and scalars up, records (and flags) down, in pieces of at most a chunk.  A stride-0 scalar is
// uploaded once.
int g1_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  int rc = bmv_check_args(ctx, scalar_stride, out_form);
  if (rc || n == 0) return rc;
  if (!points || !scalars || !out_points) return null_pointer(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t in_stride = point_stride(ctx->point_form), out_stride = point_stride(out_form);
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK);
  HostStage io(ctx, {(size_t)piece * 32, (size_t)piece * in_stride}, (size_t)piece * out_stride, piece, "out of device memory for the batch multiplication staging");
  if (io.rc) return io.rc;
  if (scalar_stride == 0) rc = io.up(0, scalars, 32, "hipMemcpy(scalar)");
  if (rc) return rc;
  return io.run(n, piece, out_points, out_stride, out_inf, [&](uint64_t off, uint64_t m) -> int {
    int up = scalar_stride ? io.up(0, scalars + off * 32, m * 32, "hipMemcpy(scalars)") : MSM377_OK;
    if (!up) up = io.up(1, points + off * in_stride, m * in_stride, "hipMemcpy(points)");
    return up ? up : g1_batch_mul_var_device(ctx, io.part(1), io.part(0), m, scalar_stride, out_form, io.records(), io.flags());
  });
}

// ---- Edwards-BLS12 variable-base batch multiplication (include/msm377.h; kernels/ed_batch_mul_var.hpp) ----
// The flow of the G1 call above on the Edwards kernels, behind ONE more step: the canonical + on-curve check of all n
// points, before anything is written.  The per-point tables are the G1 call's allocation (ctx->bm.var_table, never valid
// between calls); no slot, key or build count of any table is read or written from here.
namespace {

int edbmv_check_args(msm377_ctx* ctx, uint32_t scalar_stride) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // as edbm_check_args
  if (bmv_stride_ok(scalar_stride)) return MSM377_OK;
  ctx->err = "scalar_stride is 32 (a scalar per point) or 0 (one scalar for all points)";
  return MSM377_EINVAL;
}

int edbmv_refuse(msm377_ctx* ctx, uint64_t index, uint32_t reason) {
  ctx->err = ed_batch_mul_var_refusal(index, reason);
  return MSM377_EPOINT;
}

// k_check_curve<EdCheck> over the caller's points into counters of this call's own (ctx->edbm.point_check): no check
// call's scratch, report or list is touched.  One tiny clear, one launch, one wait.  first: the index of d_points[0] in the
// caller's array (a piece of a host-buffer call).
int edbmv_check_points(msm377_ctx* ctx, const void* d_points, uint64_t n, uint64_t first = 0) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = bm_alloc(ctx, &ctx->edbm.point_check, CHK_WORDS * 4);
  if (rc) return rc;
  uint32_t* scratch = ctx->edbm.point_check;
  hipLaunchKernelGGL(k_check_clear, dim3(1), dim3(64), 0, ctx->stream, scratch);
  hipLaunchKernelGGL(k_check_curve<EdCheck>, dim3((unsigned)((n + CHK_THREADS - 1) / CHK_THREADS)), dim3(CHK_THREADS), 0, ctx->stream, (const uint32_t*)d_points, n, 1u, scratch,
                     (uint32_t*)nullptr);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t h[CHK_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t key = (uint64_t)h[CHK_FIRST] | ((uint64_t)h[CHK_FIRST + 1] << 32);
  if (key == UINT64_MAX) return MSM377_OK;
  return edbmv_refuse(ctx, first + (key >> 2), (uint32_t)(key & 3) == CHK_CLASS_NONCANON ? MSM377_CHECK_CANONICAL : MSM377_CHECK_CURVE);
}

}  // namespace

int ed_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, void* d_out_points) {
  const uint32_t stride_words = scalar_stride / 4;
  const auto check = [&]() -> int {
    const int rc = check_pointers<EdMul>(ctx, {}, {d_scalars}, {d_points}, 64, d_out_points, 64);
    return rc ? rc : edbmv_check_points(ctx, d_points, n);
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    hipLaunchKernelGGL(k_edbmv_table, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, (const uint8_t*)d_points + off * 64, m, stash);
    const int rc = normalise<EdMul>(ctx, m * BMV_ENTRIES, EDBM_FORM_TABLE, ctx->bm.var_table, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_edbmv_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)ctx->bm.var_table, (const uint32_t*)d_scalars + off * stride_words, m, stride_words,
                       stash);
    note_walk(ctx, MSM377_WALK_ED_BATCH_MUL_VAR, MSM377_WALK_FORM_ED, (uint32_t)BMV_WIDTH, 1, 1, 0, 1);
    return MSM377_OK;
  };
  return batch_device_call<EdMul>(ctx, edbmv_check_args(ctx, scalar_stride), n, BMV_PASS, EDBM_FORM_WIRE, d_out_points, 64, nullptr, check, [&] { return bmv_ensure_table(ctx); }, pass);
}

// Host buffers: points and scalars up, records down, in pieces of at most a chunk; a stride-0 scalar is uploaded once.  A
// call of ONE piece leaves the check to its device call, which runs it before anything is written.  A call of several
// pieces checks all of them first, on the device, piece by piece through the staging -- a piece that has come down is not
// taken back -- and then uploads the points a second time (the host's own check, EdHostCheck, takes 11 us per point on
// one thread against 6 ms per 2^20 points of upload).
int ed_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points) {
  int rc = edbmv_check_args(ctx, scalar_stride);
  if (rc || n == 0) return rc;
  if (!points || !scalars || !out_points) return null_pointer(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK);
  HostStage io(ctx, {(size_t)piece * 32, (size_t)piece * 64}, (size_t)piece * 64, 0, "out of device memory for the batch multiplication staging");
  if (io.rc) return io.rc;
  for (uint64_t off = 0; n > piece && off < n && !rc; off += piece) {
    const uint64_t m = std::min<uint64_t>(piece, n - off);
    rc = io.up(1, points + off * 64, m * 64, "hipMemcpy(points)");
    if (!rc) rc = edbmv_check_points(ctx, io.part(1), m, off);
  }
  if (rc) return rc;
  if (scalar_stride == 0) rc = io.up(0, scalars, 32, "hipMemcpy(scalar)");
  if (rc) return rc;
  return io.run(n, piece, out_points, 64, nullptr, [&](uint64_t off, uint64_t m) -> int {
    int up = scalar_stride ? io.up(0, scalars + off * 32, m * 32, "hipMemcpy(scalars)") : MSM377_OK;
    if (!up) up = io.up(1, points + off * 64, m * 64, "hipMemcpy(points)");
    return up ? up : ed_batch_mul_var_device(ctx, io.part(1), io.part(0), m, scalar_stride, io.records());
  });
}

// ---- Edwards-BLS12 pairwise linear combination (include/msm377.h; kernels/ed_batch_lincomb2.hpp) ----
// The flow of the G1 call below on the Edwards kernels, behind the step of the Edwards variable-base call above: the
// canonical + on-curve check of BOTH arrays before anything is written.  Per pass of EDBL2_PASS pairs: both tables through
// the stash and ONE normalisation, then the joint walk; the flow normalises again.  A pass reads all of its inputs before it
// writes its outputs, and passes cover disjoint index ranges: d_out_points == d_p or == d_q is safe where that array has a
// record per pair, and so is the fold in place (q = p + h records, out = p, n = h).  The tables are ctx->bm.var_table, never
// valid between calls; no slot, key or build count of any table is read or written from here.
namespace {

int edbl2_check_args(msm377_ctx* ctx, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride, uint32_t b_stride) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // as edbm_check_args
  if (ed_batch_lincomb2_strides_ok(p_stride, q_stride, a_stride, b_stride)) return MSM377_OK;
  ctx->err = "a_stride and b_stride are each 32 or 0 (one scalar for all pairs), p_stride and q_stride each 64 or 0 (one point for all pairs)";
  return MSM377_EINVAL;
}

int edbl2_check_overlap(msm377_ctx* ctx, const void* p, const void* q, uint32_t p_stride, uint32_t q_stride, const void* out) {
  if ((p_stride || out != p) && (q_stride || out != q)) return MSM377_OK;
  ctx->err = "the outputs would overwrite the one point of a stride-0 array";
  return MSM377_EINVAL;
}

// k_check_curve<EdCheck> over np points of p and nq of q (a stride-0 array: ONE point) into two sets of counters of this
// call's own (ctx->edbm.pair_check): no check call's scratch, report or list is touched, nor the variable-base call's.  Two
// tiny clears, two launches, one wait.  first_p, first_q: the index of d_p[0] / d_q[0] in the caller's array (a piece of a
// host-buffer call; 0 for the one point of a stride-0 array).
int edbl2_check_points(msm377_ctx* ctx, const void* d_p, uint64_t np, const void* d_q, uint64_t nq, uint64_t first_p = 0, uint64_t first_q = 0) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = bm_alloc(ctx, &ctx->edbm.pair_check, 2 * CHK_WORDS * 4);
  if (rc) return rc;
  const void* pts[2] = {d_p, d_q};
  const uint64_t cnt[2] = {np, nq}, first[2] = {first_p, first_q};
  for (uint32_t t = 0; t < 2; t++) {
    uint32_t* scratch = ctx->edbm.pair_check + t * CHK_WORDS;
    hipLaunchKernelGGL(k_check_clear, dim3(1), dim3(64), 0, ctx->stream, scratch);
    if (cnt[t])
      hipLaunchKernelGGL(k_check_curve<EdCheck>, dim3((unsigned)((cnt[t] + CHK_THREADS - 1) / CHK_THREADS)), dim3(CHK_THREADS), 0, ctx->stream, (const uint32_t*)pts[t], cnt[t], 1u, scratch,
                         (uint32_t*)nullptr);
  }
  HIP_TRY(ctx, hipGetLastError());
  uint32_t h[2 * CHK_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->edbm.pair_check, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t key[2], bad[2];
  for (uint32_t t = 0; t < 2; t++) {
    key[t] = (uint64_t)h[t * CHK_WORDS + CHK_FIRST] | ((uint64_t)h[t * CHK_WORDS + CHK_FIRST + 1] << 32);
    bad[t] = key[t] == UINT64_MAX ? UINT64_MAX : first[t] + (key[t] >> 2);
  }
  if (bad[0] == UINT64_MAX && bad[1] == UINT64_MAX) return MSM377_OK;
  const uint32_t t = ed_batch_lincomb2_q_first(bad[0], bad[1]) ? 1u : 0u;
  ctx->err = ed_batch_lincomb2_refusal(t, bad[t], (uint32_t)(key[t] & 3) == CHK_CLASS_NONCANON ? MSM377_CHECK_CANONICAL : MSM377_CHECK_CURVE);
  return MSM377_EPOINT;
}

}  // namespace

int ed_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                             uint32_t b_stride, void* d_out_points) {
  const uint32_t a_words = a_stride / 4, b_words = b_stride / 4;
  const auto check = [&]() -> int {
    int rc = check_pointers<EdMul>(ctx, {}, {d_a, d_b}, {d_p, d_q}, 64, d_out_points, 64);
    if (!rc) rc = edbl2_check_overlap(ctx, d_p, d_q, p_stride, q_stride, d_out_points);
    return rc ? rc : edbl2_check_points(ctx, d_p, p_stride ? n : 1, d_q, q_stride ? n : 1);
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    hipLaunchKernelGGL(k_edbl2_table, dim3(bm_grid(m).x, EDBL2_TERMS), dim3(BM_THREADS), 0, ctx->stream, (const uint8_t*)d_p + off * p_stride, (const uint8_t*)d_q + off * q_stride, p_stride,
                       q_stride, m, stash);
    const int rc = normalise<EdMul>(ctx, m * EDBL2_TERMS * BMV_ENTRIES, EDBM_FORM_TABLE, ctx->bm.var_table, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_edbl2_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)ctx->bm.var_table, (const uint32_t*)d_a + off * a_words,
                       (const uint32_t*)d_b + off * b_words, m, a_words, b_words, stash);
    note_walk(ctx, MSM377_WALK_ED_BATCH_LINCOMB2, MSM377_WALK_FORM_ED, (uint32_t)BMV_WIDTH, EDBL2_TERMS, 1, 0, EDBL2_TERMS);
    return MSM377_OK;
  };
  return batch_device_call<EdMul>(ctx, edbl2_check_args(ctx, p_stride, q_stride, a_stride, b_stride), n, EDBL2_PASS, EDBM_FORM_WIRE, d_out_points, 64, nullptr, check,
                                  [&] { return bmv_ensure_table(ctx); }, pass);
}

// Host buffers: both scalar arrays and both point arrays up, records down, in pieces of at most a chunk; a stride-0 scalar
// or point is uploaded once.  A call of ONE piece leaves the check to its device call; a call of several pieces checks all
// pieces of both arrays first, on the device, piece by piece through the staging, as ed_batch_mul_var does, and then uploads
// the points a second time.  Pieces come in rising order, so the first piece with a finding holds the lowest index.
int ed_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                      uint32_t b_stride, uint8_t* out_points) {
  int rc = edbl2_check_args(ctx, p_stride, q_stride, a_stride, b_stride);
  if (rc || n == 0) return rc;
  if (!p || !q || !a || !b || !out_points) return null_pointer(ctx);
  rc = edbl2_check_overlap(ctx, p, q, p_stride, q_stride, out_points);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK);
  HostStage io(ctx, {(size_t)piece * 32, (size_t)piece * 32, (size_t)piece * 64, (size_t)piece * 64}, (size_t)piece * 64, 0,
               "out of device memory for the linear combination staging");  // a, b, p, q
  if (io.rc) return io.rc;
  if (a_stride == 0) rc = io.up(0, a, 32, "hipMemcpy(scalar a)");
  if (!rc && b_stride == 0) rc = io.up(1, b, 32, "hipMemcpy(scalar b)");
  if (!rc && p_stride == 0) rc = io.up(2, p, 64, "hipMemcpy(point p)");
  if (!rc && q_stride == 0) rc = io.up(3, q, 64, "hipMemcpy(point q)");
  for (uint64_t off = 0; n > piece && off < n && !rc; off += piece) {
    const uint64_t m = std::min<uint64_t>(piece, n - off);
    if (p_stride) rc = io.up(2, p + off * 64, m * 64, "hipMemcpy(points p)");
    if (!rc && q_stride) rc = io.up(3, q + off * 64, m * 64, "hipMemcpy(points q)");
    if (!rc) rc = edbl2_check_points(ctx, io.part(2), p_stride ? m : (off ? 0 : 1), io.part(3), q_stride ? m : (off ? 0 : 1), p_stride ? off : 0, q_stride ? off : 0);
  }
  if (rc) return rc;
  return io.run(n, piece, out_points, 64, nullptr, [&](uint64_t off, uint64_t m) -> int {
    int up = a_stride ? io.up(0, a + off * 32, m * 32, "hipMemcpy(scalars a)") : MSM377_OK;
    if (!up && b_stride) up = io.up(1, b + off * 32, m * 32, "hipMemcpy(scalars b)");
    if (!up && p_stride) up = io.up(2, p + off * 64, m * 64, "hipMemcpy(points p)");
    if (!up && q_stride) up = io.up(3, q + off * 64, m * 64, "hipMemcpy(points q)");
    return up ? up : ed_batch_lincomb2_device(ctx, io.part(2), io.part(3), io.part(0), io.part(1), m, p_stride, q_stride, a_stride, b_stride, io.records());
  });
}

// ---- Edwards-BLS12 k-term linear combination (include/msm377.h; kernels/ed_batch_lincomb.hpp) ----
// The flow of the pairwise call above with the number of terms a run-time value: the canonical + on-curve check of EVERY
// term's points before anything is written; per pass of EDBL_PASS outputs the k tables through the stash in ceil(k / 2)
// rounds of one table launch and ONE normalisation each (a chunk of the stash holds two tables of a full pass), round r
// into the records from r * 16 m on, then the joint walk; the flow normalises again.  A pass reads all of its inputs
// before it writes its outputs, and passes cover disjoint index ranges: d_out_points equal to the points of a term with a
// record per output is safe, and so is the fold in place.  The tables are the call's own allocation
// (ctx->edbm.lincomb_table), never valid between calls; ctx->bm.var_table and every slot, key and build count are left alone.
namespace {

int edbl_check_args(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // as edbm_check_args
  if (ed_batch_lincomb_shape_ok(terms, k)) return MSM377_OK;
  ctx->err = !terms ? "null pointer" : k < 1 || k > MSM377_LINCOMB_MAX_TERMS ? "k is 1 to MSM377_LINCOMB_MAX_TERMS terms"
                                      : "in every term scalar_stride is 32 or 0 (one scalar for all outputs) and point_stride 64 or 0 (one point for all outputs)";
  return MSM377_EINVAL;
}

// The pointers of the k terms and of the outputs: none null, all 16-byte aligned, the outputs not over a stride-0 point.
int edbl_check_pointers(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, const void* out, bool device) {
  bool null = !out, misaligned = device && ((uintptr_t)out & 15) != 0, over = false;
  for (uint32_t j = 0; j < k; j++) {
    null |= !terms[j].points || !terms[j].scalars;
    misaligned |= device && ((((uintptr_t)terms[j].points) | ((uintptr_t)terms[j].scalars)) & 15) != 0;
    over |= terms[j].point_stride == 0 && terms[j].points == out;
  }
  if (null) return null_pointer(ctx);
  if (misaligned) {
    ctx->err = EdMul::MISALIGNED;
    return MSM377_EINVAL;
  }
  if (over) {
    ctx->err = "the outputs would overwrite the one point of a stride-0 term";
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

// k_check_curve<EdCheck> over cnt[j] points of term j (a stride-0 term: ONE point; 0: nothing of it in this piece) into k
// sets of counters of this call's own (ctx->edbm.lincomb_check): no check call's scratch, report or list is touched, nor
// the other batch calls'.  k tiny clears, up to k launches, one wait.  first[j]: the index of d_points[j][0] in the
// caller's array (a piece of a host-buffer call; 0 for the one point of a stride-0 term).
int edbl_check_points(msm377_ctx* ctx, uint32_t k, const void* const* d_points, const uint64_t* cnt, const uint64_t* first) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = bm_alloc(ctx, &ctx->edbm.lincomb_check, (size_t)MSM377_LINCOMB_MAX_TERMS * CHK_WORDS * 4);
  if (rc) return rc;
  for (uint32_t j = 0; j < k; j++) {
    uint32_t* scratch = ctx->edbm.lincomb_check + j * CHK_WORDS;
    hipLaunchKernelGGL(k_check_clear, dim3(1), dim3(64), 0, ctx->stream, scratch);
    if (cnt[j])
      hipLaunchKernelGGL(k_check_curve<EdCheck>, dim3((unsigned)((cnt[j] + CHK_THREADS - 1) / CHK_THREADS)), dim3(CHK_THREADS), 0, ctx->stream, (const uint32_t*)d_points[j], cnt[j], 1u,
                         scratch, (uint32_t*)nullptr);
  }
  HIP_TRY(ctx, hipGetLastError());
  uint32_t h[MSM377_LINCOMB_MAX_TERMS * CHK_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->edbm.lincomb_check, (size_t)k * CHK_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t key[MSM377_LINCOMB_MAX_TERMS], bad[MSM377_LINCOMB_MAX_TERMS];
  for (uint32_t j = 0; j < k; j++) {
    key[j] = (uint64_t)h[j * CHK_WORDS + CHK_FIRST] | ((uint64_t)h[j * CHK_WORDS + CHK_FIRST + 1] << 32);
    bad[j] = key[j] == UINT64_MAX ? UINT64_MAX : first[j] + (key[j] >> 2);
  }
  const uint32_t t = ed_batch_lincomb_first_term(bad, k);
  if (t == k) return MSM377_OK;
  ctx->err = ed_batch_lincomb_refusal(t, bad[t], (uint32_t)(key[t] & 3) == CHK_CLASS_NONCANON ? MSM377_CHECK_CANONICAL : MSM377_CHECK_CURVE);
  return MSM377_EPOINT;
}

// The tables of a pass for k terms: ONE allocation, regrown for a larger k (the old one goes back first) and kept otherwise.
int edbl_ensure_table(msm377_ctx* ctx, uint32_t k) {
  EdBatchMulState& st = ctx->edbm;
  if (st.lincomb_table && st.lincomb_terms >= k) return MSM377_OK;
  ctx->own.release(st.lincomb_table);
  st.lincomb_table = nullptr;
  st.lincomb_terms = 0;
  const int rc = bm_alloc(ctx, &st.lincomb_table, (size_t)k * BMV_ENTRIES * EDBL_PASS * BM_REC_WORDS * 4);
  if (!rc) st.lincomb_terms = k;
  return rc;
}

}  // namespace

int ed_batch_lincomb_device(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, void* d_out_points) {
  const int early = edbl_check_args(ctx, terms, k);
  const auto check = [&]() -> int {
    const int rc = edbl_check_pointers(ctx, terms, k, d_out_points, true);
    if (rc) return rc;
    const void* pts[MSM377_LINCOMB_MAX_TERMS];
    uint64_t cnt[MSM377_LINCOMB_MAX_TERMS], first[MSM377_LINCOMB_MAX_TERMS];
    for (uint32_t j = 0; j < k; j++) pts[j] = terms[j].points, cnt[j] = terms[j].point_stride ? n : 1, first[j] = 0;
    return edbl_check_points(ctx, k, pts, cnt, first);
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    uint32_t* table = ctx->edbm.lincomb_table;
    EdblTerms of_pass = {};
    for (uint32_t j = 0; j < k; j++) {
      of_pass.points[j] = (const uint8_t*)terms[j].points + off * terms[j].point_stride;
      of_pass.scalars[j] = (const uint32_t*)terms[j].scalars + off * (terms[j].scalar_stride / 4);
      of_pass.point_stride[j] = terms[j].point_stride;
      of_pass.scalar_words[j] = terms[j].scalar_stride / 4;
    }
    for (uint32_t first = 0; first < k; first += EDBL_ROUND_TERMS) {  // (two tables of a full pass are one chunk of the stash)
      const uint32_t round_terms = std::min<uint32_t>(EDBL_ROUND_TERMS, k - first);
      hipLaunchKernelGGL(k_edbl_table, dim3(bm_grid(m).x, round_terms), dim3(BM_THREADS), 0, ctx->stream, of_pass, first, m, stash);
      const int rc = normalise<EdMul>(ctx, m * round_terms * BMV_ENTRIES, EDBM_FORM_TABLE, table + (size_t)first * BMV_ENTRIES * m * BM_REC_WORDS, nullptr);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(k_edbl_accumulate, bm_grid(m), dim3(BM_THREADS), (size_t)k * EDBL_TERM_LDS_WORDS * 4, ctx->stream, (const uint32_t*)table, of_pass, k, m, stash);
    note_walk(ctx, MSM377_WALK_ED_BATCH_LINCOMB, MSM377_WALK_FORM_ED, (uint32_t)BMV_WIDTH, k, 1, 0, k);
    ctx->last.walk.d_tables = table;
    return MSM377_OK;
  };
  return batch_device_call<EdMul>(ctx, early, n, EDBL_PASS, EDBM_FORM_WIRE, d_out_points, 64, nullptr, check, [&] { return edbl_ensure_table(ctx, k); }, pass);
}

// Host buffers: every term's scalars and points up, records down, in pieces of at most a chunk; a stride-0 scalar or point
// is uploaded once.  Parts 2j and 2j + 1 of the staging are term j's scalars and points.  A call of ONE piece leaves the
// check to its device call; a call of several pieces checks all pieces of all terms first, on the device, piece by piece
// through the staging, as ed_batch_lincomb2 does, and then uploads the points a second time.  Pieces come in rising
// order, so the first piece with a finding holds the lowest index.
int ed_batch_lincomb(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint8_t* out_points) {
  int rc = edbl_check_args(ctx, terms, k);
  if (rc || n == 0) return rc;
  rc = edbl_check_pointers(ctx, terms, k, out_points, false);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK);
  const auto s = [&](uint32_t j) { return j < k ? (size_t)piece * 32 : (size_t)0; };  // parts 2j, 2j + 1: the scalars and the points of term j
  const auto p = [&](uint32_t j) { return j < k ? (size_t)piece * 64 : (size_t)0; };
  HostStage io(ctx, {s(0), p(0), s(1), p(1), s(2), p(2), s(3), p(3), s(4), p(4), s(5), p(5), s(6), p(6), s(7), p(7)}, (size_t)piece * 64, 0,
               "out of device memory for the linear combination staging");
  static_assert(MSM377_LINCOMB_MAX_TERMS == 8, "the staging above lists eight terms");
  if (io.rc) return io.rc;
  const auto points_of = [&](uint32_t j) { return (const uint8_t*)terms[j].points; };
  const auto scalars_of = [&](uint32_t j) { return (const uint8_t*)terms[j].scalars; };
  for (uint32_t j = 0; j < k && !rc; j++) {
    if (terms[j].scalar_stride == 0) rc = io.up(2 * j, scalars_of(j), 32, "hipMemcpy(scalar)");
    if (!rc && terms[j].point_stride == 0) rc = io.up(2 * j + 1, points_of(j), 64, "hipMemcpy(point)");
  }
  const void* pts[MSM377_LINCOMB_MAX_TERMS];
  for (uint32_t j = 0; j < k; j++) pts[j] = io.part(2 * j + 1);
  for (uint64_t off = 0; n > piece && off < n && !rc; off += piece) {
    const uint64_t m = std::min<uint64_t>(piece, n - off);
    uint64_t cnt[MSM377_LINCOMB_MAX_TERMS], first[MSM377_LINCOMB_MAX_TERMS];
    for (uint32_t j = 0; j < k && !rc; j++) {
      if (terms[j].point_stride) rc = io.up(2 * j + 1, points_of(j) + off * 64, m * 64, "hipMemcpy(points)");
      cnt[j] = terms[j].point_stride ? m : (off ? 0 : 1);
      first[j] = terms[j].point_stride ? off : 0;
    }
    if (!rc) rc = edbl_check_points(ctx, k, pts, cnt, first);
  }
  if (rc) return rc;
  return io.run(n, piece, out_points, 64, nullptr, [&](uint64_t off, uint64_t m) -> int {
    int up = MSM377_OK;
    msm377_lincomb_term d_terms[MSM377_LINCOMB_MAX_TERMS];
    for (uint32_t j = 0; j < k && !up; j++) {
      if (terms[j].scalar_stride) up = io.up(2 * j, scalars_of(j) + off * 32, m * 32, "hipMemcpy(scalars)");
      if (!up && terms[j].point_stride) up = io.up(2 * j + 1, points_of(j) + off * 64, m * 64, "hipMemcpy(points)");
      d_terms[j] = msm377_lincomb_term{io.part(2 * j + 1), io.part(2 * j), terms[j].point_stride, terms[j].scalar_stride};
    }
    return up ? up : ed_batch_lincomb_device(ctx, d_terms, k, m, io.records());
  });
}

// ---- Edwards-BLS12 row commitments (include/msm377.h "Edwards-BLS12 row commitments"; kernels/ed_commit_rows.hpp) ----
// The G1 flow above on this curve's kernels, over a set of its own (ctx->ed_gens): the plan, the ONE allocation, the
// drop-first / install-last rule and the host staging are G1's.  What differs: the generators are checked on the DEVICE
// before anything is built (k_check_curve<EdCheck> into counters of the set's own: EdHostCheck takes 11 us per point on
// one thread, 45 ms at 4 096 generators), and the fold is grouped (k_edcr_fold, two levels at most).
namespace {

void edcr_drop_set(msm377_ctx* ctx) {
  GeneratorSet& gs = ctx->ed_gens;
  gs.k = 0;
  gs.width = 0;
  ctx->own.release(gs.tables);
  gs.tables = nullptr;
}

int edcr_check_args(msm377_ctx* ctx, uint32_t k, uint64_t out_stride, uint64_t base_stride) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // as edbm_check_args
  return check_shape(ctx, k, MSM377_GEN_MAX, "k is 1 to MSM377_GEN_MAX generators", out_stride, base_stride);
}

int edcr_check_set(msm377_ctx* ctx, uint32_t k) {
  if (!ctx->ed_gens.valid()) {
    ctx->err = "no resident Edwards-BLS12 generator set: call msm377_ed_set_generators first";
    return MSM377_ESTATE;
  }
  if (k > ctx->ed_gens.k) {
    ctx->err = "k is above the resident generator count";
    return MSM377_ESTATE;
  }
  return MSM377_OK;
}

// edbmv_check_points over the k generators at d_gens, into ctx->ed_gens.check: no check call's scratch, report or list
// and no other batch call's counters are touched.
int edcr_check_generators(msm377_ctx* ctx, const uint32_t* d_gens, uint32_t k) {
  const int rc = bm_alloc(ctx, &ctx->ed_gens.check, CHK_WORDS * 4);
  if (rc) return rc;
  uint32_t* scratch = ctx->ed_gens.check;
  hipLaunchKernelGGL(k_check_clear, dim3(1), dim3(64), 0, ctx->stream, scratch);
  hipLaunchKernelGGL(k_check_curve<EdCheck>, dim3((unsigned)((k + CHK_THREADS - 1) / CHK_THREADS)), dim3(CHK_THREADS), 0, ctx->stream, d_gens, (uint64_t)k, 1u, scratch, (uint32_t*)nullptr);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t h[CHK_WORDS];
  HIP_TRY(ctx, hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t key = (uint64_t)h[CHK_FIRST] | ((uint64_t)h[CHK_FIRST + 1] << 32);
  if (key == UINT64_MAX) return MSM377_OK;
  ctx->err = ed_commit_rows_refusal(key >> 2, (uint32_t)(key & 3) == CHK_CLASS_NONCANON ? MSM377_CHECK_CANONICAL : MSM377_CHECK_CURVE);
  return MSM377_EPOINT;
}

}  // namespace

// As g1_set_generators; the wire bytes go up once, are checked where they lie, and the builder reads them from there
// (its own upload writes the same bytes to the same place).
int ed_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy, uint32_t k, int window_bits) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  forget_walk(ctx);  // the build below goes through the stash
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  edcr_drop_set(ctx);  // first, whatever follows: a call that fails leaves no set
  if (!gens_xy || k == 0) return MSM377_OK;
  const int c = window_bits ? window_bits : BM_NARROW_WIDTH;
  if (!batch_mul_width_supported(c)) {
    ctx->err = "window_bits is 8, 16 or 0 (= 8)";
    return MSM377_EINVAL;
  }
  if (k > MSM377_GEN_MAX || (c == BM_WIDE_WIDTH && k > MSM377_GEN_WIDE_MAX)) {
    ctx->err = "a set holds at most MSM377_GEN_MAX generators, MSM377_GEN_WIDE_MAX with 16-bit tables";
    return MSM377_EINVAL;
  }
  GeneratorSet& gs = ctx->ed_gens;
  uint32_t *row_bases = nullptr, *gens_wire = nullptr;
  int rc = bm_ensure_scratch(ctx);
  if (!rc) rc = bm_alloc(ctx, &gens_wire, (size_t)k * 64);
  if (!rc && !hip_ok(ctx, hipMemcpyAsync(gens_wire, gens_xy, (size_t)k * 64, hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(generators)")) rc = MSM377_EHIP;
  if (!rc) rc = edcr_check_generators(ctx, gens_wire, k);
  if (!rc) rc = bm_alloc(ctx, &gs.tables, (size_t)k * bm_table_records((uint32_t)c) * BM_REC_WORDS * 4);
  if (!rc) rc = bm_alloc(ctx, &row_bases, (size_t)k * (bm_windows(c) + 1) * BM_REC_WORDS * 4);
  if (!rc) rc = build_mul_tables<EdMul>(ctx, gens_xy, k, c, row_bases, gens_wire, gs.tables, nullptr);
  if (rc) (void)hipStreamSynchronize(ctx->stream);  // (nothing in flight reads what goes back below)
  ctx->own.release(row_bases);  // (the build has waited for its launches)
  ctx->own.release(gens_wire);
  if (rc) {
    edcr_drop_set(ctx);
    return rc;
  }
  gs.width = c;
  gs.k = k;
  return MSM377_OK;
}

int ed_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, void* d_out_points) {
  const int early = edcr_check_args(ctx, k, out_stride, base_stride);
  const CommitRowsPlan plan = commit_rows_plan(early ? 1 : k);  // (a k that was refused is not planned for)
  const auto check = [&]() -> int {
    const int rc = check_pointers<EdMul>(ctx, {}, {d_scalars}, {}, 64, d_out_points, 64);
    return rc ? rc : edcr_check_set(ctx, k);
  };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {  // row `off` of the CALL's layout, as on G1
    const GeneratorSet& gs = ctx->ed_gens;
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    const dim3 grid = bm_grid(m);
    const uint64_t part_stride = (uint64_t)grid.x * BM_THREADS;  // <= rows_per_pass, so segments * part_stride <= BM_CHUNK
    const uint32_t S = plan.segments, groups = (S + CR_FOLD_GROUP - 1) / CR_FOLD_GROUP;
    hipLaunchKernelGGL(k_edcr_accumulate, dim3(grid.x, S), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)gs.tables, (const uint8_t*)d_scalars + off * out_stride, m, k, plan.bases_per_segment,
                       out_stride, base_stride, (uint32_t)gs.width, part_stride, stash);
    if (S > 1) hipLaunchKernelGGL(k_edcr_fold, dim3(grid.x, groups), dim3(BM_THREADS), 0, ctx->stream, stash, m, S, 1u, part_stride);
    if (groups > 1) hipLaunchKernelGGL(k_edcr_fold, dim3(grid.x, 1), dim3(BM_THREADS), 0, ctx->stream, stash, m, S, CR_FOLD_GROUP, part_stride);
    note_walk(ctx, MSM377_WALK_ED_COMMIT_ROWS, MSM377_WALK_FORM_ED, (uint32_t)gs.width, k, S, part_stride);
    return MSM377_OK;
  };
  return batch_device_call<EdMul>(ctx, early, n, plan.rows_per_pass, EDBM_FORM_WIRE, d_out_points, 64, nullptr, check, nothing_to_prepare, pass);
}

// Host buffers: each piece of at most 2^20 scalars (2^20 / k rows) repacked row-major on the host, up, records down.
int ed_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  int rc = edcr_check_args(ctx, k, out_stride, base_stride);
  if (rc || n == 0) return rc;
  if (!scalars || !out_points) return null_pointer(ctx);
  rc = edcr_check_set(ctx, k);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK / k);
  HostStage io(ctx, {(size_t)piece * k * 32}, (size_t)piece * 64, 0, "out of device memory for the row commitment staging");
  if (io.rc) return io.rc;
  return io.run(n, piece, out_points, 64, nullptr, [&](uint64_t off, uint64_t m) -> int {
    const int up = io.repack_rows(0, scalars, off, m, k, out_stride, base_stride);
    return up ? up : ed_commit_rows_device(ctx, io.part(0), m, k, (uint64_t)k * 32, 32, io.records());
  });
}

// ---- pairwise linear combination (include/msm377.h "pairwise linear combination"; kernels/batch_lincomb2.hpp) ----
// Per pass of BL2_PASS pairs: both tables through the stash and ONE normalisation, then the joint walk; the flow
// normalises again.  A pass reads all of its inputs before it writes its outputs, and passes cover disjoint index
// ranges: d_out_points == d_p or == d_q is safe for records of equal size, and so is the fold in place (q = p + h
// records, out = p, n = h).
namespace {

int bl2_check_args(msm377_ctx* ctx, uint32_t a_stride, uint32_t b_stride, uint32_t out_form) {
  const int rc = bm_check_form(ctx, out_form);
  if (rc) return rc;
  if (!bmv_stride_ok(a_stride) || !bmv_stride_ok(b_stride)) {
    ctx->err = "a_stride and b_stride are each 32 (a scalar per pair) or 0 (one scalar for all pairs)";
    return MSM377_EINVAL;
  }
  return MSM377_OK;
}

}  // namespace

int g1_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t a_stride, uint32_t b_stride,
                             uint32_t out_form, void* d_out_points, uint8_t* d_out_inf) {
  const int early = bl2_check_args(ctx, a_stride, b_stride, out_form);
  const uint32_t form = early ? 0 : ctx->point_form, a_words = a_stride / 4, b_words = b_stride / 4;
  const size_t in_stride = point_stride(form), out_stride = point_stride(out_form);
  const auto check = [&] { return check_pointers<G1Mul>(ctx, {}, {d_a, d_b}, {d_p, d_q}, in_stride, d_out_points, out_stride); };
  const auto pass = [&](uint64_t off, uint64_t m) -> int {
    uint4* stash = reinterpret_cast<uint4*>(ctx->bm.stash);
    bmv_launch_table(ctx, form, (const uint8_t*)d_p + off * in_stride, m, stash);
    bmv_launch_table(ctx, form, (const uint8_t*)d_q + off * in_stride, m, stash + BMV_ENTRIES * m);
    const int rc = normalise<G1Mul>(ctx, m * BL2_TERMS * BMV_ENTRIES, BM_FORM_TABLE, ctx->bm.var_table, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bl2_accumulate, bm_grid(m), dim3(BM_THREADS), 0, ctx->stream, (const uint32_t*)ctx->bm.var_table, (const uint32_t*)d_a + off * a_words,
                       (const uint32_t*)d_b + off * b_words, m, a_words, b_words, scalars_mont(ctx), stash);
    note_walk(ctx, MSM377_WALK_BATCH_LINCOMB2, MSM377_WALK_FORM_XYZZ, (uint32_t)BMV_WIDTH, BL2_TERMS, 1, 0, BL2_TERMS);
    return MSM377_OK;
  };
  return batch_device_call<G1Mul>(ctx, early, n, BL2_PASS, out_form, d_out_points, out_stride, d_out_inf, check, [&] { return bmv_ensure_table(ctx); }, pass);
}

// Host buffers: both scalar arrays and both point arrays up, records (and flags) down, in pieces of at most a chunk.  A
// stride-0 scalar is uploaded once.
int g1_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t a_stride, uint32_t b_stride, uint32_t out_form,
                      uint8_t* out_points, uint8_t* out_inf) {
  int rc = bl2_check_args(ctx, a_stride, b_stride, out_form);
  if (rc || n == 0) return rc;
  if (!p || !q || !a || !b || !out_points) return null_pointer(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t in_stride = point_stride(ctx->point_form), out_stride = point_stride(out_form);
  const uint64_t piece = std::min<uint64_t>(n, BM_CHUNK);
  HostStage io(ctx, {(size_t)piece * 32, (size_t)piece * 32, (size_t)piece * in_stride, (size_t)piece * in_stride}, (size_t)piece * out_stride, piece,
               "out of device memory for the linear combination staging");  // a, b, p, q
  if (io.rc) return io.rc;
  if (a_stride == 0) rc = io.up(0, a, 32, "hipMemcpy(scalar a)");
  if (!rc && b_stride == 0) rc = io.up(1, b, 32, "hipMemcpy(scalar b)");
  if (rc) return rc;
  return io.run(n, piece, out_points, out_stride, out_inf, [&](uint64_t off, uint64_t m) -> int {
    int up = a_stride ? io.up(0, a + off * 32, m * 32, "hipMemcpy(scalars a)") : MSM377_OK;
    if (!up && b_stride) up = io.up(1, b + off * 32, m * 32, "hipMemcpy(scalars b)");
    if (!up) up = io.up(2, p + off * in_stride, m * in_stride, "hipMemcpy(points p)");
    if (!up) up = io.up(3, q + off * in_stride, m * in_stride, "hipMemcpy(points q)");
    return up ? up : g1_batch_lincomb2_device(ctx, io.part(2), io.part(3), io.part(0), io.part(1), m, a_stride, b_stride, out_form, io.records(), io.flags());
  });
}

int g1_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out) {
  if (!ctx || (n && !d_points_out) || ((uintptr_t)d_points_out & 15)) return MSM377_EINVAL;
  if (n == 0) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_generate_bases, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, seed, n, (uint32_t*)d_points_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MSM377_OK;
}

// ---- table read-backs (msm377_g1_read_mul_table, msm377_ed_read_mul_table) ----
// A copy of records the batch calls keep between calls, and what the host knows about them.  table: null if there is no
// valid table at that place; key: the slot's 96 bytes (Edwards-BLS12: 64 base bytes, then zeros), null for a generator's.
static int read_mul_table(msm377_ctx* ctx, const uint32_t* table, int c, const uint8_t* key, const char* not_valid, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  if (!table) {
    ctx->err = not_valid;
    return MSM377_ESTATE;
  }
  const uint64_t records = bm_table_records((uint32_t)c);
  if (first > records || count > records - first || (count && !words)) {
    ctx->err = "record range outside the table";
    return MSM377_EINVAL;
  }
  if (info) {
    memset(info, 0, sizeof *info);
    info->width = (uint32_t)c;
    info->rows = (uint32_t)bm_windows(c) + 1;
    info->records = records;
    if (key) memcpy(info->key, key, 96);
  }
  if (words && count) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(words, table + first * BM_REC_WORDS, (size_t)count * BM_REC_WORDS * 4, hipMemcpyDeviceToHost));
  }
  return MSM377_OK;
}
static int read_mul_slot(msm377_ctx* ctx, const MulTableSlot& sl, const char* not_valid, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  return read_mul_table(ctx, sl.valid ? sl.table : nullptr, sl.width, sl.key, not_valid, info, first, count, words);
}

int g1_read_mul_table(msm377_ctx* ctx, uint32_t which, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  const char* not_valid = "that window table is not valid: never built, dropped, or left by a build that failed";
  if (which == MSM377_MUL_TABLE_SINGLE && index == 0) return read_mul_slot(ctx, ctx->bm.single, not_valid, info, first, count, words);
  if (which == MSM377_MUL_TABLE_MULTI && index < MSM377_MUL_MAX_BASES) return read_mul_slot(ctx, ctx->bmm.slot[index], not_valid, info, first, count, words);
  if (which > MSM377_MUL_TABLE_GENERATOR) {
    ctx->err = "unknown window table";
    return MSM377_EINVAL;
  }
  const GeneratorSet& gs = ctx->gens;
  const bool there = which == MSM377_MUL_TABLE_GENERATOR && index < gs.k;
  return read_mul_table(ctx, there ? gs.tables + (size_t)index * bm_table_records((uint32_t)gs.width) * BM_REC_WORDS : nullptr, gs.width, nullptr, not_valid, info, first, count, words);
}

// Slot `index` of ctx->edbm as it stands.
int ed_read_mul_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  if (index >= MSM377_MUL_MAX_BASES) {
    ctx->err = "unknown window table";
    return MSM377_EINVAL;
  }
  return read_mul_slot(ctx, ctx->edbm.slot[index], "that window table is not valid: never built, or left by a build that failed", info, first, count, words);
}

// Generator `index` of ctx->ed_gens as it stands: as ed_read_mul_table reads a slot, with a zero key.
int ed_read_generator_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  const GeneratorSet& gs = ctx->ed_gens;
  const uint32_t* table = index < gs.k ? gs.tables + (size_t)index * bm_table_records((uint32_t)gs.width) * BM_REC_WORDS : nullptr;
  return read_mul_table(ctx, table, gs.width, nullptr, "no resident Edwards-BLS12 generator set, or the index is beyond it", info, first, count, words);
}

// ---- stash read-backs (msm377_read_walk_stash, msm377_g1_read_walk_tables, msm377_ed_read_walk_table[s]) ----
// Copies of what the last pass of the last batch call left (context.hpp WalkLayout), gathered from the piece-major stash
// into point-major words: piece k of stash point j is at piece index k * BM_CHUNK + j.  No launch; every batch call has
// waited for its stream before it returned.
static int walk_not_valid(msm377_ctx* ctx) {
  ctx->err = "no batch pass to read: no batch call has completed a pass on this context, the last one failed, or the stash was written since";
  return MSM377_ESTATE;
}

// `pieces` 16-byte pieces from piece `first_piece` on, of stash points [at, at + count), into `words` (count x take u32,
// take <= 4 pieces: the words of a point that are wanted).
static int gather_pieces(msm377_ctx* ctx, uint32_t first_piece, uint32_t pieces, uint64_t at, uint64_t count, uint32_t take, uint32_t* words) {
  std::vector<uint32_t> piece((size_t)count * 4);
  for (uint32_t k = 0; k < pieces; k++) {
    HIP_TRY(ctx, hipMemcpy(piece.data(), ctx->bm.stash + ((size_t)(first_piece + k) * BM_CHUNK + at) * 4, (size_t)count * 16, hipMemcpyDeviceToHost));
    for (uint64_t j = 0; j < count; j++)
      for (uint32_t q = 0; q < 4 && 4 * k + q < take; q++) words[(size_t)j * take + 4 * k + q] = piece[(size_t)j * 4 + q];
  }
  return MSM377_OK;
}

int read_walk_stash(msm377_ctx* ctx, msm377_walk_stash_info* info, uint32_t segment, uint64_t first, uint64_t count, uint32_t* point_words, uint32_t* product_words) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  const WalkLayout& wl = ctx->last.walk;
  if (!wl.valid || !ctx->bm.stash) return walk_not_valid(ctx);
  const msm377_walk_stash_info& wi = wl.info;
  if (segment >= wi.segments || first > wi.m || count > wi.m - first || (count && !point_words && !product_words) || (product_words && segment != 0)) {
    ctx->err = "point range or segment outside the pass (running products: segment 0 only)";
    return MSM377_EINVAL;
  }
  if (info) *info = wi;
  if (!count) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool ed = wi.form == MSM377_WALK_FORM_ED;
  const uint32_t point_pieces = ed ? EDBM_POINT_PIECES : BM_POINT_PIECES, all_pieces = ed ? EDBM_PIECES : BM_PIECES;
  const uint64_t at = (uint64_t)segment * wi.stride + first;  // < segments * stride <= BM_CHUNK by the plan; first + count <= m <= stride
  int rc = MSM377_OK;
  if (point_words) rc = gather_pieces(ctx, 0, point_pieces, at, count, wi.point_words, point_words);
  if (!rc && product_words) rc = gather_pieces(ctx, point_pieces, all_pieces - point_pieces, at, count, wi.product_words + wi.product_pad, product_words);
  return rc;
}

// form: the curve whose call asks; the tables of the other curve's pass are not its to read.
static int read_walk_tables(msm377_ctx* ctx, uint32_t form, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words) {
  if (!ctx) return MSM377_EINVAL;
  ctx->err.clear();
  const WalkLayout& wl = ctx->last.walk;
  if (!wl.valid || !wl.tables.tables || wl.info.form != form || !wl.d_tables) return walk_not_valid(ctx);
  const msm377_walk_tables_info& ti = wl.tables;
  if (table >= ti.tables || first > ti.m || count > ti.m - first || (count && !words)) {
    ctx->err = "point range or table outside the pass";
    return MSM377_EINVAL;
  }
  if (info) *info = ti;
  if (!count) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (uint32_t e = 0; e < ti.entries; e++)  // entry e + 1 of point i of table t: record ((t * entries) + e) * m + i
    HIP_TRY(ctx, hipMemcpy(words + ((size_t)e * count) * BM_REC_WORDS, wl.d_tables + (((size_t)table * ti.entries + e) * ti.m + first) * BM_REC_WORDS,
                           (size_t)count * BM_REC_WORDS * 4, hipMemcpyDeviceToHost));
  return MSM377_OK;
}

int g1_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words) {
  return read_walk_tables(ctx, MSM377_WALK_FORM_XYZZ, info, table, first, count, words);
}
int ed_read_walk_table(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words) {
  return read_walk_tables(ctx, MSM377_WALK_FORM_ED, info, table, first, count, words);
}
int ed_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  return ed_read_walk_table(ctx, info, 0, first, count, words);
}

}  // namespace eng
}  // namespace msm377
