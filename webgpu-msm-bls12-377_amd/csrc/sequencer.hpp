// Stage sequencer: everything that enqueues GPU work for an entry point of include/msm377.h.  capi.hip validates nothing
// and forwards here; the functions below carry the entry point's name without its msm377_ prefix and its exact
// arguments and return codes.  Kernels: kernels/*.hpp (compiled into sequencer.hip only); host tail: host_tail.hpp.
#pragma once
#include <stdint.h>

#include "../../include/msm377.h"

struct msm377_ctx;

namespace msm377 {
namespace eng {

int g1_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[96]);
int g1_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]);
int ed_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[64]);
int ed_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[64]);
int ed_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out);
// Short scalars: n x scalar_bytes little-endian bytes, every scalar below 2^scalar_bits.
int g1_msm_short_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t scalar_bits, uint8_t out_xy[96]);
int g1_msm_short(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_bytes, uint32_t scalar_bits, uint8_t out_xy[96]);
int g1_msm_fixed_base_short_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t scalar_bits, uint8_t out_xy[96]);
int scalars_width_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t* bits_out);
int g1_set_bases_device(msm377_ctx* ctx, const void* d_points, uint64_t n);
int g1_set_bases(msm377_ctx* ctx, const uint8_t* points, uint64_t n);
int g1_set_bases_precomputed_device(msm377_ctx* ctx, const void* d_points, uint64_t n);
int g1_set_bases_precomputed(msm377_ctx* ctx, const uint8_t* points, uint64_t n);
int g1_msm_fixed_base_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint8_t out_xy[96]);
int g1_msm_fixed_base_batch_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t batch, uint8_t* out_xy);
int g1_msm_fixed_base(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]);
int window_partials(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin, uint32_t win_count, uint8_t* host_out, void* dev_out);
int g1_glv_window_partials_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t win_begin, uint32_t win_count, uint8_t* partials_out);
int g1_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out);

// Input validation (kernels/validate.hpp).  flags: any valid MSM377_CHECK_* mask (normalised inside).
int g1_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out);
int g1_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out);
int ed_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out);
int ed_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out);

// Fixed-base batch multiplication (kernels/batch_mul.hpp): out[i] = [s_i]B, every output its own affine point.
int g1_batch_mul_device(msm377_ctx* ctx, const uint8_t base_xy[96], const void* d_scalars, uint64_t n, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf);
int g1_batch_mul(msm377_ctx* ctx, const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
// Multi-base batch multiplication (kernels/batch_mul_multi.hpp): out[i] = sum_j [s_ij]B_j over k fixed bases.
int g1_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                              void* d_out_points, uint8_t* d_out_inf);
int g1_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                       uint8_t* out_points, uint8_t* out_inf);
// Row commitments (kernels/commit_rows.hpp): out[i] = sum_j [s_ij]G_j over the first k generators of the resident set.
int g1_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy, uint32_t k, int window_bits);
int g1_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, void* d_out_points,
                          uint8_t* d_out_inf);
int g1_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
// Variable-base batch multiplication (kernels/batch_mul_var.hpp): out[i] = [s_i]P_i.
int g1_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf);
int g1_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
// Pairwise linear combination (kernels/batch_lincomb2.hpp): out[i] = [a_i]P_i + [b_i]Q_i.
int g1_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t a_stride, uint32_t b_stride,
                             uint32_t out_form, void* d_out_points, uint8_t* d_out_inf);
int g1_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t a_stride, uint32_t b_stride, uint32_t out_form,
                      uint8_t* out_points, uint8_t* out_inf);

// Edwards-BLS12 batch multiplication (kernels/ed_batch_mul.hpp): out[i] = sum_j [s_ij]B_j, 64-byte wire outputs.
int ed_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, void* d_out_points);
int ed_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points);
// Edwards-BLS12 variable-base batch multiplication (kernels/ed_batch_mul_var.hpp): out[i] = [s_i]P_i.
int ed_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, void* d_out_points);
int ed_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points);
// Edwards-BLS12 pairwise linear combination (kernels/ed_batch_lincomb2.hpp): out[i] = [a_i]P_i + [b_i]Q_i.
int ed_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                             uint32_t b_stride, void* d_out_points);
int ed_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                      uint32_t b_stride, uint8_t* out_points);
// Edwards-BLS12 k-term linear combination (kernels/ed_batch_lincomb.hpp): out[i] = sum_j [s_ij]P_ij, 1 <= k <= 8 terms.
int ed_batch_lincomb_device(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, void* d_out_points);
int ed_batch_lincomb(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint8_t* out_points);

// Edwards-BLS12 row commitments (kernels/ed_commit_rows.hpp): out[i] = sum_j [s_ij]G_j over the first k generators of that curve's resident set.
int ed_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy, uint32_t k, int window_bits);
int ed_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, void* d_out_points);
int ed_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points);

// The window table of a batch operation as it stands (no launch): msm377_g1_read_mul_table, msm377_ed_read_mul_table,
// msm377_ed_read_generator_table.
int ed_read_generator_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words);
int g1_read_mul_table(msm377_ctx* ctx, uint32_t which, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words);
int ed_read_mul_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words);

// What the last pass of the last batch call left in the stash, and the per-point tables it walked (no launch):
// msm377_read_walk_stash, msm377_g1_read_walk_tables, msm377_ed_read_walk_tables, msm377_ed_read_walk_table.
int read_walk_stash(msm377_ctx* ctx, msm377_walk_stash_info* info, uint32_t segment, uint64_t first, uint64_t count, uint32_t* point_words, uint32_t* product_words);
int g1_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words);
int ed_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint64_t first, uint64_t count, uint32_t* words);
int ed_read_walk_table(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words);

void twin_return(msm377_ctx* ctx);  // takes back the resident bases a batch call lent to the twin of ctx

// Shared with capi.hip (argument checks of the host-only entry points, the stage read-back).
bool hip_ok(msm377_ctx* ctx, int hip_error, const char* what);
#define HIP_TRY(ctx, call)                                                   \
  do {                                                                       \
    if (!msm377::eng::hip_ok((ctx), (int)(call), #call)) return MSM377_EHIP; \
  } while (0)

}  // namespace eng
}  // namespace msm377
