// The C ABI of include/msm377.h: settings, the host-only combine functions, the stage read-back, and one forwarding line
// per entry point that enqueues GPU work (those live in sequencer.hip under the same name without the msm377_ prefix)
// or belongs to the context's life cycle (context.hip).  No kernels in this translation unit.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "context.hpp"
#include "host_tail.hpp"
#include "sequencer.hpp"
#include "batch_mul_host.hpp"
#include "batch_mul_multi_host.hpp"
#include "ed_batch_mul_host.hpp"
#include "ed_batch_mul_var_host.hpp"
#include "ed_batch_lincomb2_host.hpp"
#include "ed_batch_lincomb_host.hpp"
#include "ed_commit_rows_host.hpp"
#include "commit_rows_host.hpp"
#include "commit_rows_plan.hpp"
#include "batch_lincomb2_host.hpp"
#include "batch_mul_var_host.hpp"
#include "import_host.hpp"
#include "validate_host.hpp"

using namespace msm377;

// --------------------------------------------------------------------------- C ABI ----

extern "C" {

const char* msm377_version(void) { return "msm377 0.1 gfx950"; }

const char* msm377_strerror(int code) {
  switch (code) {
    case MSM377_OK: return "ok";
    case MSM377_EINVAL: return "invalid argument";
    case MSM377_EHIP: return "HIP runtime error";
    case MSM377_ESCALAR: return "scalar out of range for the signed window recode";
    case MSM377_ENOMEM: return "out of memory";
    case MSM377_ESTATE: return "call sequence error";
    case MSM377_EGLVRANGE: return "scalar outside the GLV range";
    case MSM377_EEXCEPTIONAL: return "exceptional case of the twisted Edwards law while combining partial records";
    case MSM377_EPOINT: return "an input point failed a requested check (canonical / on the curve / in the subgroup)";
    default: return "unknown error";
  }
}

// ---- the context's life cycle: context.hip ----
int msm377_ctx_create(int device, uint64_t max_points, msm377_ctx** out) { return eng::ctx_create(device, max_points, Knobs::from_env(), false, out); }
void msm377_ctx_destroy(msm377_ctx* ctx) { eng::ctx_destroy(ctx); }
int msm377_ctx_set_stage_capture(msm377_ctx* ctx, int enabled) { return eng::set_stage_capture(ctx, enabled); }

// An entry point that converts bases: after an error the base records are not described (msm377_g1_read_bases).
static int converted(msm377_ctx* ctx, int rc) {
  if (ctx && rc != MSM377_OK) ctx->last.bases.valid = false;
  return rc;
}

const char* msm377_last_error(const msm377_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int msm377_g1_window_partials_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin,
                                     uint32_t win_count, uint8_t* partials_out) {
  if (!partials_out) return MSM377_EINVAL;
  return converted(ctx, eng::window_partials(ctx, d_points, d_scalars, n, win_begin, win_count, partials_out, nullptr));
}

int msm377_g1_window_partials_resident(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin,
                                       uint32_t win_count, void* d_partials_out) {
  if (!d_partials_out) return MSM377_EINVAL;
  return converted(ctx, eng::window_partials(ctx, d_points, d_scalars, n, win_begin, win_count, nullptr, d_partials_out));
}


int msm377_g1_combine_window_partials(const uint8_t* partials, uint32_t num_windows, uint8_t out_xy[96]) {
  if (!partials || !out_xy || ((uintptr_t)partials & 3) || num_windows == 0 || num_windows > MSM377_NUM_WINDOWS) return MSM377_EINVAL;
  return g1_combine_tagged(reinterpret_cast<const uint32_t*>(partials), (int)num_windows, out_xy) ? MSM377_EEXCEPTIONAL : MSM377_OK;
}

int msm377_g1_combine_partials_ctx(msm377_ctx* ctx, const uint8_t* partials, uint8_t out_xy[96]) {
  if (!ctx || !partials || !out_xy || ((uintptr_t)partials & 3)) return MSM377_EINVAL;
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(partials);
  bool all_te = true, all_w = true;
  for (int w = 0; w < MSM377_NUM_WINDOWS; w++) {
    const bool te = window_record_is_te(rec + (size_t)w * MSM377_G1_PARTIAL_POINTS * MSM377_G1_POINT_WORDS);
    all_te = all_te && te;
    all_w = all_w && !te;
  }
  int rc = MSM377_OK;
  // (The workers are not pre-woken for this call: between a rank's window_partials call and this combine lie the
  // all-gather and a D2H copy, longer than any spin deadline -- round 2 armed them from window_partials and they spun
  // for nothing, on every rank of the host.)
  if (all_te)
    {
    const int tr = eng::te_tail(ctx, rec, out_xy);
    rc = tr == eng::TAIL_EXCEPTIONAL ? MSM377_EEXCEPTIONAL : tr;
  }
  else if (all_w)
    rc = eng::xyzz_tail(ctx, rec, out_xy);
  else
    rc = g1_combine_tagged(rec, MSM377_NUM_WINDOWS, out_xy) ? MSM377_EEXCEPTIONAL : MSM377_OK;
  if (rc == MSM377_EEXCEPTIONAL) ctx->err = "the partial records add up to an exceptional case of the twisted Edwards law (points outside the prime-order subgroup): recompute them in form 0";
  return rc;
}

int msm377_g1_fold_window_partials(uint8_t* partials, uint32_t win_count) {
  if (!partials || ((uintptr_t)partials & 3) || win_count > MSM377_NUM_WINDOWS) return MSM377_EINVAL;
  g1_fold_tagged(reinterpret_cast<uint32_t*>(partials), (int)win_count);
  return MSM377_OK;
}

int msm377_g1_combine_partials(const uint8_t* partials, uint8_t out_xy[96]) {
  if (!partials || !out_xy || ((uintptr_t)partials & 3)) return MSM377_EINVAL;
  return g1_combine_tagged(reinterpret_cast<const uint32_t*>(partials), MSM377_NUM_WINDOWS, out_xy) ? MSM377_EEXCEPTIONAL : MSM377_OK;
}

int msm377_g1_add_points(const uint8_t* points_xy, uint32_t count, uint8_t out_xy[96]) {
  if (!out_xy || (count && !points_xy)) return MSM377_EINVAL;
  return g1h_add_wire_points(points_xy, count, out_xy) ? MSM377_OK : MSM377_EINVAL;
}

int msm377_g1_combine_partials_split(const uint8_t* partials, uint32_t pieces, uint8_t out_xy[96]) {
  if (!partials || !out_xy || ((uintptr_t)partials & 3) || pieces < 1 || pieces > 64) return MSM377_EINVAL;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(partials);
  for (int w = 0; w < MSM377_NUM_WINDOWS; w++)
    if (!window_record_is_te(p + (size_t)w * 16 * 48)) return MSM377_EINVAL;  // the decomposition of the Edwards tail only
  return teh_combine_split(p, MSM377_NUM_WINDOWS, out_xy, (int)pieces) ? MSM377_EEXCEPTIONAL : MSM377_OK;
}


// The fixed-size read-back and msm377_ctx_get_stage_form describe G1 records only (52 words); Edwards-BLS12 records are read as run.
static bool is_g1_form(int form) { return form == MSM377_STAGE_FORM_XYZZ || form == MSM377_STAGE_FORM_TE; }

int msm377_g1_read_stage(msm377_ctx* ctx, uint32_t slot, uint16_t* digits, uint32_t* row_ptr, uint32_t* val_idx, uint32_t* buckets) {
  if (!ctx) return MSM377_EINVAL;
  // capture mode 1 only: the sizes below are those of its route; under mode 2 a call lays its stages out as it runs
  if (ctx->capture != 1 || ctx->last.n == 0 || slot >= ctx->last.geom_windows || !is_g1_form(ctx->last.form) || ctx->last.glv) {
    ctx->err = "no captured stage data for that window slot (capture mode 2 is read with msm377_g1_read_stage_ex)";
    return MSM377_ESTATE;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t n = ctx->last.n;
  if (digits) HIP_TRY(ctx, hipMemcpy(digits, ctx->d_digits + (size_t)slot * n, n * 2, hipMemcpyDeviceToHost));
  if (row_ptr) HIP_TRY(ctx, hipMemcpy(row_ptr, ctx->d_row_ptr + (size_t)slot * RP, RP * 4, hipMemcpyDeviceToHost));
  if (val_idx) HIP_TRY(ctx, hipMemcpy(val_idx, ctx->d_val_idx + (size_t)slot * n, n * 4, hipMemcpyDeviceToHost));
  if (buckets) {
    uint32_t* tmp = (uint32_t*)malloc((size_t)BKT_WORDS * NB * 4);
    if (!tmp) return MSM377_ENOMEM;
    hipError_t e = hipMemcpy(tmp, ctx->d_buckets_snap + (size_t)slot * BKT_WORDS * NB, (size_t)BKT_WORDS * NB * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess)  // 64-word records (four 16-word coordinate slots) -> the 52 packed words of the ABI
      for (uint32_t t = 0; t < NB; t++)
        for (uint32_t c = 0; c < 4; c++)
          for (uint32_t j = 0; j < 13; j++) buckets[(size_t)t * PT_WORDS + c * 13 + j] = tmp[(size_t)t * BKT_WORDS + c * 16 + j];
    free(tmp);
    HIP_TRY(ctx, e);
  }
  return MSM377_OK;
}

// The as-run read-back: sizes, biases and pointers are those enqueue_decompose recorded at its launch (StageLayout);
// nothing about the geometry is worked out here.
int msm377_g1_read_stage_ex(msm377_ctx* ctx, uint32_t slot, msm377_stage_info* info, void* digits, uint32_t* row_ptr, uint32_t* val_idx, uint32_t* buckets) {
  if (!ctx) return MSM377_EINVAL;
  const StageLayout& sl = ctx->last.stage;
  if (!ctx->capture || !sl.valid || !ctx->d_buckets_snap) {
    ctx->err = "no captured stage data: stage capture is off, or the last call is not one the capture mode describes";
    return MSM377_ESTATE;
  }
  if (slot >= sl.info.slots) {
    ctx->err = "no captured stage data for that window slot";
    return MSM377_ESTATE;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  msm377_stage_info out = sl.info;
  if (sl.d_key_max) {
    uint32_t words[MSM377_NUM_WINDOWS] = {};
    HIP_TRY(ctx, hipMemcpy(words, sl.d_key_max, sizeof words, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < out.slots && s < MSM377_NUM_WINDOWS; s++) out.key_max[s] = words[s];
  }
  if (info) *info = out;
  const uint64_t cols = out.columns;
  const size_t records = out.bucket_records;
  if (digits) HIP_TRY(ctx, hipMemcpy(digits, (const uint8_t*)sl.d_digits + (size_t)slot * cols * out.digit_bytes, cols * out.digit_bytes, hipMemcpyDeviceToHost));
  if (row_ptr) HIP_TRY(ctx, hipMemcpy(row_ptr, ctx->d_row_ptr + (size_t)slot * out.row_ptr_len, (size_t)out.row_ptr_len * 4, hipMemcpyDeviceToHost));
  if (val_idx) HIP_TRY(ctx, hipMemcpy(val_idx, ctx->d_val_idx + (size_t)slot * cols, cols * 4, hipMemcpyDeviceToHost));
  if (buckets) {
    // records as the pass stored them (four coordinate slots of coord_words words) -> 4 x limbs packed words: 52 for G1, 36 for Edwards-BLS12
    const size_t cw = sl.coord_words, nl = sl.limbs, bw = 4 * cw;
    uint32_t* tmp = (uint32_t*)malloc(records * bw * 4);
    if (!tmp) return MSM377_ENOMEM;
    hipError_t e = hipMemcpy(tmp, ctx->d_buckets_snap + (size_t)slot * records * bw, records * bw * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      for (size_t t = 0; t < records; t++)
        for (size_t c = 0; c < 4; c++)
          for (size_t j = 0; j < nl; j++) buckets[(t * 4 + c) * nl + j] = tmp[t * bw + c * cw + j];
    free(tmp);
    HIP_TRY(ctx, e);
  }
  return MSM377_OK;
}

// The window records of the last pass: layout and pointer are those enqueue_reduce wrote down beside the gather launch.
int msm377_g1_read_partials(msm377_ctx* ctx, msm377_partials_info* info, uint32_t* words) {
  if (!ctx) return MSM377_EINVAL;
  const StageLayout& sl = ctx->last.stage;
  if (!ctx->capture || !sl.valid || !ctx->d_buckets_snap || !sl.d_partials) {
    ctx->err = "no captured window records: stage capture is off, or the last call is not one the capture mode describes";
    return MSM377_ESTATE;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // a zero-copy call returns while k_gather_partials is still finishing (kernels/reduce.hpp publish_to_host, INVARIANT)
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (info) *info = sl.partials;
  if (words) {
    const size_t count = (size_t)sl.partials.records * sl.partials.points * 4 * sl.partials.coord_words;
    HIP_TRY(ctx, hipMemcpy(words, sl.d_partials, count * 4, hipMemcpyDeviceToHost));
  }
  return MSM377_OK;
}

// The accumulation work list of the last pass: the host's half of `info` and the pointers are those enqueue_accumulate
// wrote down beside its launches (WorkListLayout); the counters are read where the kernels left them.
int msm377_g1_read_work_list(msm377_ctx* ctx, msm377_work_list_info* info, uint32_t* items_out, uint32_t* split_rows_out, uint32_t* row_ovf_base_out, uint64_t ovf_first,
                             uint64_t ovf_count, uint32_t* ovf_out) {
  if (!ctx) return MSM377_EINVAL;
  const WorkListLayout& wl = ctx->last.work;
  if (!ctx->capture || !ctx->last.stage.valid || !ctx->d_buckets_snap || !wl.valid) {
    ctx->err = "no captured work list: stage capture is off, the last call is not one the capture mode describes, or a check call has used the work-list counters since";
    return MSM377_ESTATE;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  msm377_work_list_info out = wl.info;
  static_assert(MSM377_WORK_HIST_BINS == SEG_BINS, "the histogram of the ABI is the kernels'");
  uint32_t counters[2] = {};
  HIP_TRY(ctx, hipMemcpy(out.hist, wl.d_hist, sizeof out.hist, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(&out.items, wl.d_total, 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(counters, wl.d_counters, sizeof counters, hipMemcpyDeviceToHost));
  out.split_rows = counters[0], out.overflow_slots = counters[1];
  // what the kernels counted must fit what the launches were sized for before anything is copied by those counts
  if (out.items > out.max_items || out.split_rows > out.rows || out.overflow_slots > out.max_items - out.rows) {
    ctx->err = "the work-list counters exceed the bounds of their launches";
    return MSM377_ESTATE;
  }
  if (ovf_out && (ovf_first > out.overflow_slots || ovf_count > out.overflow_slots - ovf_first)) {
    ctx->err = "record range outside the overflow records";
    return MSM377_EINVAL;
  }
  if (info) *info = out;
  if (items_out && out.items) HIP_TRY(ctx, hipMemcpy(items_out, ctx->d_work, (size_t)out.items * sizeof(WorkItem), hipMemcpyDeviceToHost));
  if (split_rows_out && out.split_rows) HIP_TRY(ctx, hipMemcpy(split_rows_out, ctx->d_split_rows, (size_t)out.split_rows * 4, hipMemcpyDeviceToHost));
  if (row_ovf_base_out) HIP_TRY(ctx, hipMemcpy(row_ovf_base_out, ctx->d_row_ovf_base, (size_t)out.rows * 4, hipMemcpyDeviceToHost));
  if (ovf_out && ovf_count) {
    // records as the pass stored them (four coordinate slots of coord_words words) -> 4 x limbs packed words, as msm377_g1_read_stage_ex packs a bucket
    const size_t cw = wl.coord_words, nl = wl.limbs, bw = wl.bkt_words;
    uint32_t* tmp = (uint32_t*)malloc((size_t)ovf_count * bw * 4);
    if (!tmp) return MSM377_ENOMEM;
    hipError_t e = hipMemcpy(tmp, ctx->d_ovf + (size_t)ovf_first * bw, (size_t)ovf_count * bw * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      for (size_t t = 0; t < ovf_count; t++)
        for (size_t c = 0; c < 4; c++)
          for (size_t j = 0; j < nl; j++) ovf_out[(t * 4 + c) * nl + j] = tmp[t * bw + c * cw + j];
    free(tmp);
    HIP_TRY(ctx, e);
  }
  return MSM377_OK;
}

// The base records of the last conversion: layout and pointer are those note_bases (sequencer.hip) wrote down beside the
// launch; this is a copy.
int msm377_g1_read_bases(msm377_ctx* ctx, msm377_bases_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  if (!ctx) return MSM377_EINVAL;
  const BasesLayout& bl = ctx->last.bases;
  if (!bl.valid || !bl.d_records) {
    ctx->err = "no base records to read: no conversion has run on this context yet, or the last one failed";
    return MSM377_ESTATE;
  }
  if (first > bl.info.records || count > bl.info.records - first || (count && !words && !info)) {
    ctx->err = "record range outside the base records";
    return MSM377_EINVAL;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  msm377_bases_info out = bl.info;
  if (bl.d_flagged) HIP_TRY(ctx, hipMemcpy(&out.flagged, bl.d_flagged, 4, hipMemcpyDeviceToHost));
  if (info) *info = out;
  if (words && count) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));  // (every entry point has waited for its conversion already)
    HIP_TRY(ctx, hipMemcpy(words, bl.d_records + first * out.record_words, (size_t)count * out.record_words * 4, hipMemcpyDeviceToHost));
  }
  return MSM377_OK;
}

int msm377_g1_read_mul_table(msm377_ctx* ctx, uint32_t which, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  return eng::g1_read_mul_table(ctx, which, index, info, first, count, words);
}

int msm377_read_walk_stash(msm377_ctx* ctx, msm377_walk_stash_info* info, uint32_t segment, uint64_t first, uint64_t count, uint32_t* point_words, uint32_t* product_words) {
  return eng::read_walk_stash(ctx, info, segment, first, count, point_words, product_words);
}

int msm377_g1_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words) {
  return eng::g1_read_walk_tables(ctx, info, table, first, count, words);
}

int msm377_ctx_get_stage_form(const msm377_ctx* ctx) { return (ctx && ctx->capture && ctx->last.n && is_g1_form(ctx->last.form)) ? ctx->last.form : -1; }

int msm377_g1_xyzz_to_affine(const uint32_t xyzz[52], uint8_t out_xy[96]) {
  if (!xyzz || !out_xy) return MSM377_EINVAL;
  g1h_to_wire(g1h_from_device_words(xyzz), out_xy);
  return MSM377_OK;
}

int msm377_ctx_set_glv(msm377_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return MSM377_EINVAL;
  ctx->knobs.glv_mode = mode == 1 ? 1 : 0;  // 2 ("the library's choice") is off: see Knobs::glv_mode
  return MSM377_OK;
}

int msm377_ctx_set_g1_form(msm377_ctx* ctx, int form) {
  if (!ctx || form < 0 || form > 1) return MSM377_EINVAL;
  ctx->knobs.g1_form = form;
  return MSM377_OK;
}

int msm377_ctx_get_products_per_addition(const msm377_ctx* ctx) { return ctx ? ctx->last.products : 0; }

int msm377_ctx_get_fallback_info(const msm377_ctx* ctx, uint64_t* count, uint32_t* last_mask) {
  if (!ctx) return MSM377_EINVAL;
  if (count) *count = ctx->fallback.count;
  if (last_mask) *last_mask = ctx->fallback.mask;
  return MSM377_OK;
}

int msm377_ctx_set_precompute_window(msm377_ctx* ctx, int window_bits) {
  if (!ctx || (window_bits != MSM377_WINDOW_BITS && window_bits != MSM377_WIDE_WINDOW_BITS)) return MSM377_EINVAL;
  ctx->knobs.precomp_bits = window_bits;
  return MSM377_OK;
}

int msm377_ctx_set_base_checks(msm377_ctx* ctx, uint32_t flags) {
  if (!ctx || (flags && !check_flags_normal(flags))) return MSM377_EINVAL;
  ctx->knobs.base_checks = check_flags_normal(flags);
  return MSM377_OK;
}

int msm377_ctx_set_input_format(msm377_ctx* ctx, uint32_t point_form, uint32_t scalar_form) {
  if (!ctx || point_form > MSM377_POINTS_MONT_FLAG || scalar_form > MSM377_SCALARS_MONT) return MSM377_EINVAL;
  ctx->point_form = point_form;
  ctx->scalar_form = scalar_form;
  return MSM377_OK;
}

int msm377_ctx_get_input_format(const msm377_ctx* ctx, uint32_t* point_form, uint32_t* scalar_form) {
  if (!ctx) return MSM377_EINVAL;
  if (point_form) *point_form = ctx->point_form;
  if (scalar_form) *scalar_form = ctx->scalar_form;
  return MSM377_OK;
}

// ---- native input forms: the host-only parts (import_host.hpp) ----
int msm377_g1_import_points_host(const uint8_t* in, uint64_t n, uint32_t point_form, uint8_t* out_wire, uint32_t* out_inf_mask) {
  if (point_form > MSM377_POINTS_MONT_FLAG || (n && (!in || !out_wire))) return MSM377_EINVAL;
  import_points_host(in, n, point_form, out_wire, out_inf_mask);
  return MSM377_OK;
}

int msm377_import_scalars_host(const uint8_t* in, uint64_t n, uint32_t scalar_form, uint8_t* out_wire) {
  if (scalar_form > MSM377_SCALARS_MONT || (n && (!in || !out_wire))) return MSM377_EINVAL;
  import_scalars_host(in, n, scalar_form, out_wire);
  return MSM377_OK;
}

int msm377_g1_result_to_native(const uint8_t xy[96], uint8_t out[104]) {
  if (!xy || !out) return MSM377_EINVAL;
  return result_to_native_host(xy, out) ? MSM377_OK : MSM377_EINVAL;
}

// ---- fixed-base batch multiplication: the host-only parts (batch_mul_host.hpp) and the settings ----
int msm377_g1_batch_mul_host(const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  return batch_mul_host(base_xy, scalars, n, MSM377_SCALARS_WIRE, out_form, out_points, out_inf);
}

int msm377_g1_batch_mul_multi_host(const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                                   uint8_t* out_points, uint8_t* out_inf) {
  return batch_mul_multi_host(bases_xy, k, scalars, n, out_stride, base_stride, MSM377_SCALARS_WIRE, out_form, out_points, out_inf);
}

int msm377_g1_commit_rows_host(const uint8_t* gens_xy, uint32_t k, const uint8_t* scalars, uint32_t scalar_form, uint64_t n, uint64_t out_stride, uint64_t base_stride,
                               uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  return commit_rows_host(gens_xy, k, scalars, scalar_form, n, out_stride, base_stride, out_form, out_points, out_inf);
}

void msm377_commit_rows_plan(uint32_t k, uint32_t* segments, uint32_t* bases_per_segment, uint64_t* rows_per_pass) {
  const CommitRowsPlan p = commit_rows_plan(k);
  if (segments) *segments = p.segments;
  if (bases_per_segment) *bases_per_segment = p.bases_per_segment;
  if (rows_per_pass) *rows_per_pass = p.rows_per_pass;
}

int msm377_ctx_get_generators(const msm377_ctx* ctx, uint32_t* k, int* window_bits) {
  if (!ctx) return MSM377_EINVAL;
  if (k) *k = ctx->gens.k;
  if (window_bits) *window_bits = ctx->gens.width;
  return MSM377_OK;
}

int msm377_g1_batch_mul_var_host(const uint8_t* points, uint32_t point_form, const uint8_t* scalars, uint32_t scalar_form, uint64_t n, uint32_t scalar_stride, uint32_t out_form,
                                 uint8_t* out_points, uint8_t* out_inf) {
  return batch_mul_var_host(points, point_form, scalars, scalar_form, n, scalar_stride, out_form, out_points, out_inf);
}

int msm377_g1_batch_lincomb2_host(const uint8_t* p, const uint8_t* q, uint32_t point_form, const uint8_t* a, const uint8_t* b, uint32_t scalar_form, uint64_t n, uint32_t a_stride,
                                  uint32_t b_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  return batch_lincomb2_host(p, q, point_form, a, b, scalar_form, n, a_stride, b_stride, out_form, out_points, out_inf);
}

int msm377_ctx_set_mul_window(msm377_ctx* ctx, int window_bits) {
  if (!ctx || (window_bits != 0 && !batch_mul_width_supported(window_bits))) return MSM377_EINVAL;
  ctx->bm.window = window_bits;
  return MSM377_OK;
}

int msm377_ctx_get_last_mul_window(const msm377_ctx* ctx) { return ctx ? ctx->bm.last_window : 0; }

uint64_t msm377_ctx_get_mul_table_builds(const msm377_ctx* ctx) { return ctx ? ctx->bm.builds : 0; }

uint64_t msm377_ctx_get_mul_multi_table_builds(const msm377_ctx* ctx) { return ctx ? ctx->bmm.builds : 0; }

// ---- Edwards-BLS12 batch multiplication: the host-only parts (ed_batch_mul_host.hpp) ----
int msm377_ed_batch_mul_multi_host(const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  return ed_batch_mul_multi_host(bases_xy, k, scalars, n, out_stride, base_stride, out_points);
}
int msm377_ed_batch_mul_var_host(const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points) {
  return ed_batch_mul_var_host(points, scalars, n, scalar_stride, out_points);
}
int msm377_ed_commit_rows_host(const uint8_t* gens_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  return ed_commit_rows_host(gens_xy, k, scalars, n, out_stride, base_stride, out_points);
}
int msm377_ed_ctx_get_generators(const msm377_ctx* ctx, uint32_t* k, int* window_bits) {
  if (!ctx) return MSM377_EINVAL;
  if (k) *k = ctx->ed_gens.k;
  if (window_bits) *window_bits = ctx->ed_gens.width;
  return MSM377_OK;
}
int msm377_ed_batch_lincomb2_host(const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                                  uint32_t b_stride, uint8_t* out_points) {
  return ed_batch_lincomb2_host(p, q, a, b, n, p_stride, q_stride, a_stride, b_stride, out_points);
}

int msm377_ed_batch_lincomb_host(const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint8_t* out_points) { return ed_batch_lincomb_host(terms, k, n, out_points); }

uint64_t msm377_ed_ctx_get_mul_table_builds(const msm377_ctx* ctx) { return ctx ? ctx->edbm.builds : 0; }

int msm377_ctx_get_last_check(const msm377_ctx* ctx, msm377_check_report* out) {
  if (!ctx || !out) return MSM377_EINVAL;
  *out = ctx->last_check;
  return MSM377_OK;
}

static int check_host_args(const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  return (!out || !check_flags_normal(flags) || (n && !points)) ? MSM377_EINVAL : MSM377_OK;
}
int msm377_g1_check_points_host(const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  if (check_host_args(points, n, flags, out)) return MSM377_EINVAL;
  check_points_host<G1HostCheck>(points, n, check_flags_normal(flags), out);
  return MSM377_OK;
}
int msm377_ed_check_points_host(const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) {
  if (check_host_args(points, n, flags, out)) return MSM377_EINVAL;
  check_points_host<EdHostCheck>(points, n, check_flags_normal(flags), out);
  return MSM377_OK;
}

// ---- short scalars: the host-only parts ----
uint32_t msm377_short_windows(uint32_t scalar_bits, uint32_t bucket_log) {
  if (scalar_bits < 1 || scalar_bits > 253 || bucket_log < 1 || bucket_log > 15) return 0;
  return short_windows(scalar_bits, bucket_log);
}

int msm377_scalars_width_host(const uint8_t* scalars, uint64_t n, uint32_t scalar_bytes, uint32_t* bits_out) {
  if (!bits_out || (n && !scalars) || (scalar_bytes != 4 && scalar_bytes != 8 && scalar_bytes != 16 && scalar_bytes != 32)) return MSM377_EINVAL;
  uint32_t best = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* k = scalars + i * scalar_bytes;
    for (uint32_t j = scalar_bytes; j-- > 0;) {
      if (!k[j]) continue;
      const uint32_t len = 8 * j + 32 - (uint32_t)__builtin_clz((uint32_t)k[j]);
      best = std::max(best, len);
      break;
    }
  }
  *bits_out = best;
  return MSM377_OK;
}

int msm377_ctx_get_last_geometry(const msm377_ctx* ctx, uint32_t* windows, uint32_t* bucket_log) {
  if (!ctx) return MSM377_EINVAL;
  if (windows) *windows = ctx->last.geom_windows;
  if (bucket_log) *bucket_log = ctx->last.geom_log;
  return MSM377_OK;
}

uint32_t msm377_ctx_get_last_sort_elem_bytes(const msm377_ctx* ctx) { return ctx ? ctx->last.sort_elem : 0u; }

int msm377_ctx_set_narrow_max(msm377_ctx* ctx, uint64_t max_points) {
  if (!ctx) return MSM377_EINVAL;
  ctx->knobs.narrow_max_points = max_points;
  return MSM377_OK;
}

int msm377_ctx_set_timing(msm377_ctx* ctx, int enabled) {
  if (!ctx) return MSM377_EINVAL;
  ctx->timing = enabled == 2 ? 2 : (enabled != 0);
  return MSM377_OK;
}

int msm377_ctx_get_stage_ms(msm377_ctx* ctx, double* ms_out) {
  if (!ctx || !ms_out) return MSM377_EINVAL;
  for (int s = 0; s < MSM377_NUM_STAGES; s++) ms_out[s] = ctx->last.stage_ms[s];
  return MSM377_OK;
}

// ---- entry points that enqueue GPU work: sequencer.hip ----
// Edwards-BLS12 is not covered by the native input forms (include/msm377.h): its calls refuse while one is set.
static int ed_wire_only(msm377_ctx* ctx) {
  if (!ctx || (ctx->point_form == MSM377_POINTS_WIRE && ctx->scalar_form == MSM377_SCALARS_WIRE)) return MSM377_OK;
  ctx->err = "the Edwards-BLS12 calls take the wire format only (msm377_ctx_set_input_format)";
  return MSM377_EINVAL;
}
int msm377_ctx_reserve_host_staging(msm377_ctx* ctx) { return eng::reserve_host_staging(ctx); }
int msm377_g1_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[96]) { return converted(ctx, eng::g1_msm_device(ctx, d_points, d_scalars, n, out_xy)); }
int msm377_g1_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]) { return converted(ctx, eng::g1_msm(ctx, points, scalars, n, out_xy)); }
int msm377_g1_msm_short_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t scalar_bits, uint8_t out_xy[96]) { return converted(ctx, eng::g1_msm_short_device(ctx, d_points, d_scalars, n, scalar_bytes, scalar_bits, out_xy)); }
int msm377_g1_msm_short(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_bytes, uint32_t scalar_bits, uint8_t out_xy[96]) { return converted(ctx, eng::g1_msm_short(ctx, points, scalars, n, scalar_bytes, scalar_bits, out_xy)); }
int msm377_g1_msm_fixed_base_short_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t scalar_bits, uint8_t out_xy[96]) { return eng::g1_msm_fixed_base_short_device(ctx, d_scalars, n, scalar_bytes, scalar_bits, out_xy); }
int msm377_scalars_width_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t* bits_out) { return eng::scalars_width_device(ctx, d_scalars, n, scalar_bytes, bits_out); }
int msm377_ed_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[64]) { return converted(ctx, ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_msm_device(ctx, d_points, d_scalars, n, out_xy)); }
int msm377_ed_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[64]) { return converted(ctx, ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_msm(ctx, points, scalars, n, out_xy)); }
int msm377_ed_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out) { return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_generate_bases_device(ctx, seed, n, d_points_out); }
int msm377_ed_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride,
                                     void* d_out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_mul_multi_device(ctx, bases_xy, k, d_scalars, n, out_stride, base_stride, d_out_points);
}
int msm377_ed_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_mul_multi(ctx, bases_xy, k, scalars, n, out_stride, base_stride, out_points);
}
int msm377_ed_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, void* d_out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_mul_var_device(ctx, d_points, d_scalars, n, scalar_stride, d_out_points);
}
int msm377_ed_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_mul_var(ctx, points, scalars, n, scalar_stride, out_points);
}
int msm377_ed_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  return eng::ed_read_walk_tables(ctx, info, first, count, words);
}
int msm377_ed_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t p_stride, uint32_t q_stride,
                                    uint32_t a_stride, uint32_t b_stride, void* d_out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_lincomb2_device(ctx, d_p, d_q, d_a, d_b, n, p_stride, q_stride, a_stride, b_stride, d_out_points);
}
int msm377_ed_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                             uint32_t b_stride, uint8_t* out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_lincomb2(ctx, p, q, a, b, n, p_stride, q_stride, a_stride, b_stride, out_points);
}
int msm377_ed_batch_lincomb_device(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, void* d_out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_lincomb_device(ctx, terms, k, n, d_out_points);
}
int msm377_ed_batch_lincomb(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint8_t* out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_batch_lincomb(ctx, terms, k, n, out_points);
}
int msm377_ed_read_walk_table(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words) {
  return eng::ed_read_walk_table(ctx, info, table, first, count, words);
}
int msm377_ed_read_mul_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  return eng::ed_read_mul_table(ctx, index, info, first, count, words);
}
int msm377_ed_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy, uint32_t k, int window_bits) { return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_set_generators(ctx, gens_xy, k, window_bits); }
int msm377_ed_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, void* d_out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_commit_rows_device(ctx, d_scalars, n, k, out_stride, base_stride, d_out_points);
}
int msm377_ed_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points) {
  return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_commit_rows(ctx, scalars, n, k, out_stride, base_stride, out_points);
}
int msm377_ed_read_generator_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words) {
  return eng::ed_read_generator_table(ctx, index, info, first, count, words);
}
int msm377_g1_set_bases_device(msm377_ctx* ctx, const void* d_points, uint64_t n) { return converted(ctx, eng::g1_set_bases_device(ctx, d_points, n)); }
int msm377_g1_set_bases(msm377_ctx* ctx, const uint8_t* points, uint64_t n) { return converted(ctx, eng::g1_set_bases(ctx, points, n)); }
int msm377_g1_set_bases_precomputed_device(msm377_ctx* ctx, const void* d_points, uint64_t n) { return converted(ctx, eng::g1_set_bases_precomputed_device(ctx, d_points, n)); }
int msm377_g1_set_bases_precomputed(msm377_ctx* ctx, const uint8_t* points, uint64_t n) { return converted(ctx, eng::g1_set_bases_precomputed(ctx, points, n)); }
int msm377_g1_msm_fixed_base_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint8_t out_xy[96]) { return eng::g1_msm_fixed_base_device(ctx, d_scalars, n, out_xy); }
int msm377_g1_msm_fixed_base_batch_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t batch, uint8_t* out_xy) { return eng::g1_msm_fixed_base_batch_device(ctx, d_scalars, n, batch, out_xy); }
int msm377_g1_msm_fixed_base(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]) { return eng::g1_msm_fixed_base(ctx, scalars, n, out_xy); }
int msm377_g1_glv_window_partials_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin, uint32_t win_count, uint8_t* partials_out) { return converted(ctx, eng::g1_glv_window_partials_device(ctx, d_points, d_scalars, n, win_begin, win_count, partials_out)); }
int msm377_g1_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out) { return eng::g1_generate_bases_device(ctx, seed, n, d_points_out); }
int msm377_g1_batch_mul_device(msm377_ctx* ctx, const uint8_t base_xy[96], const void* d_scalars, uint64_t n, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf) { return eng::g1_batch_mul_device(ctx, base_xy, d_scalars, n, out_form, d_out_points, d_out_inf); }
int msm377_g1_batch_mul(msm377_ctx* ctx, const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) { return eng::g1_batch_mul(ctx, base_xy, scalars, n, out_form, out_points, out_inf); }
int msm377_g1_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride,
                                     uint32_t out_form, void* d_out_points, uint8_t* d_out_inf) {
  return eng::g1_batch_mul_multi_device(ctx, bases_xy, k, d_scalars, n, out_stride, base_stride, out_form, d_out_points, d_out_inf);
}
int msm377_g1_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                              uint8_t* out_points, uint8_t* out_inf) {
  return eng::g1_batch_mul_multi(ctx, bases_xy, k, scalars, n, out_stride, base_stride, out_form, out_points, out_inf);
}
int msm377_g1_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy, uint32_t k, int window_bits) { return eng::g1_set_generators(ctx, gens_xy, k, window_bits); }
int msm377_g1_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, void* d_out_points,
                                 uint8_t* d_out_inf) {
  return eng::g1_commit_rows_device(ctx, d_scalars, n, k, out_stride, base_stride, out_form, d_out_points, d_out_inf);
}
int msm377_g1_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, uint8_t* out_points,
                          uint8_t* out_inf) {
  return eng::g1_commit_rows(ctx, scalars, n, k, out_stride, base_stride, out_form, out_points, out_inf);
}
int msm377_g1_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf) {
  return eng::g1_batch_mul_var_device(ctx, d_points, d_scalars, n, scalar_stride, out_form, d_out_points, d_out_inf);
}
int msm377_g1_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  return eng::g1_batch_mul_var(ctx, points, scalars, n, scalar_stride, out_form, out_points, out_inf);
}
int msm377_g1_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t a_stride, uint32_t b_stride,
                                    uint32_t out_form, void* d_out_points, uint8_t* d_out_inf) {
  return eng::g1_batch_lincomb2_device(ctx, d_p, d_q, d_a, d_b, n, a_stride, b_stride, out_form, d_out_points, d_out_inf);
}
int msm377_g1_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t a_stride, uint32_t b_stride,
                             uint32_t out_form, uint8_t* out_points, uint8_t* out_inf) {
  return eng::g1_batch_lincomb2(ctx, p, q, a, b, n, a_stride, b_stride, out_form, out_points, out_inf);
}
int msm377_g1_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out) { return eng::g1_check_points_device(ctx, d_points, n, flags, out); }
int msm377_g1_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) { return eng::g1_check_points(ctx, points, n, flags, out); }
int msm377_ed_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out) { return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_check_points_device(ctx, d_points, n, flags, out); }
int msm377_ed_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out) { return ed_wire_only(ctx) ? MSM377_EINVAL : eng::ed_check_points(ctx, points, n, flags, out); }

}  // extern "C"

