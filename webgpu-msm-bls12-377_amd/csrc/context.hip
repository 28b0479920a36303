// The life cycle of a context (context.hpp): create and destroy, the buffers that are allocated on demand, and the
// Resources value through which every one of them is taken from the HIP runtime and given back.  Host code only: no
// kernel header is included here, sizes that belong to a kernel's geometry arrive as arguments.
#include "context.hpp"

#include <string.h>

#include <algorithm>
#include <new>

#include "sequencer.hpp"

using namespace msm377;

// ---- Resources ----
hipError_t Resources::alloc(void** p, size_t bytes) {
  const hipError_t rc = hipMalloc(p, bytes);
  if (rc == hipSuccess) device.push_back(*p);
  else *p = nullptr;
  return rc;
}
hipError_t Resources::alloc_pinned(void** p, size_t bytes, unsigned flags) {
  const hipError_t rc = hipHostMalloc(p, bytes, flags);
  if (rc == hipSuccess) pinned.push_back(*p);
  else *p = nullptr;
  return rc;
}
hipError_t Resources::event(hipEvent_t* e, unsigned flags) {
  const hipError_t rc = hipEventCreateWithFlags(e, flags);
  if (rc == hipSuccess) events.push_back(*e);
  else *e = nullptr;
  return rc;
}
hipError_t Resources::stream(hipStream_t* s, const int* priority) {
  const hipError_t rc = priority ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, *priority) : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  if (rc == hipSuccess) streams.push_back(*s);
  else *s = nullptr;
  return rc;
}
void Resources::release(void* p) {
  const auto it = std::find(device.begin(), device.end(), p);
  if (!p || it == device.end()) return;
  (void)hipFree(p);
  device.erase(it);
}
void Resources::release_all() {
  for (void* p : device) (void)hipFree(p);
  for (void* p : pinned) (void)hipHostFree(p);
  for (hipEvent_t e : events) (void)hipEventDestroy(e);
  for (auto s = streams.rbegin(); s != streams.rend(); ++s) (void)hipStreamDestroy(*s);  // the main stream last
  *this = Resources();
}

bool WideBuffers::ensure(Resources& own, uint64_t n, size_t counts_words) {
  if (cap >= n) return true;
  release(own);
  if (own.alloc((void**)&digits, (size_t)WIDE_WINDOWS * n * 4) == hipSuccess && own.alloc((void**)&temp, (size_t)WIDE_WINDOWS * n * sizeof(SortElem)) == hipSuccess &&
      own.alloc((void**)&counts, counts_words * 4) == hipSuccess) {
    cap = n;
    return true;
  }
  release(own);
  (void)hipGetLastError();
  return false;
}
void WideBuffers::release(Resources& own) {
  for (void* p : {(void*)digits, (void*)temp, (void*)counts}) own.release(p);
  *this = WideBuffers();
}

namespace msm377 {
namespace eng {

int ctx_create(int device, uint64_t max_points, const Knobs& knobs, bool borrows_bases, msm377_ctx** out) {
  if (!out || max_points == 0 || max_points > (1ull << 30)) return MSM377_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return MSM377_EHIP;
  msm377_ctx* ctx = new (std::nothrow) msm377_ctx();
  if (!ctx) return MSM377_ENOMEM;
  ctx->device = device;
  ctx->cap = ctx->native.cap = max_points;
  ctx->knobs = knobs;
  ctx->tail_pool.wait_limit_ns = (int64_t)knobs.tail_wait_ms * 1000000ll;
  ctx->tail_pool.numa_local = knobs.tail_numa;
  Resources& own = ctx->own;
  const uint64_t cap = max_points;
  // The main stream outranks the side stream: the base conversion (VALU-heavy, ~0.2 ms) only has to finish before
  // the accumulation starts, decompose + sort on the main stream are the critical path (k_decompose: 16 us alone,
  // ~100 us when it competes with the conversion at equal priority).
  int prio_least = 0, prio_greatest = 0;
  bool ok = hipSetDevice(device) == hipSuccess;
  if (ok && hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_least = prio_greatest = 0;
  // (Round 3 re-measured the priorities with the faster sort, now that the conversion chain is the front end's critical
  // path: main stream high 2.554 ms, side stream high 2.583, equal 2.603 at 2^20 -- profiles/r03_final/ab_prio_prewake.txt.)
  ok = ok && own.stream(&ctx->stream, &prio_greatest) == hipSuccess && own.stream(&ctx->stream2, &prio_least) == hipSuccess &&
       own.event(&ctx->bases_ready, hipEventDisableTiming) == hipSuccess;
  auto dalloc = [&](void** p, size_t bytes) { ok = ok && own.alloc(p, bytes) == hipSuccess; };
  if (!borrows_bases) dalloc((void**)&ctx->d_raw_points, cap * 96);
  dalloc((void**)&ctx->d_raw_scalars, cap * 32);
  if (!borrows_bases) dalloc((void**)&ctx->d_bases, 2 * cap * G1_REC_WORDS * 4);  // 128-byte records of P_i and phi(P_i) (GLV front end), or 256-byte twisted Edwards records of P_i
  // (window, point) entries the window-indexed buffers hold: 16 windows of `cap` points, or the 22 windows of the
  // narrow path over a small input when that is more (small contexts)
  const uint64_t wcap = std::max<uint64_t>((uint64_t)MSM377_NUM_WINDOWS * cap, (uint64_t)NARROW_EVEN_WINDOWS * std::min<uint64_t>(cap, SMALL_SORT_MAX));
  dalloc((void**)&ctx->d_digits, wcap * 2);
  dalloc((void**)&ctx->d_range_counts, (size_t)NRANGE * MAX_SORT_BLOCKS * 4);  // chunks * wc <= MAX_SORT_BLOCKS
  dalloc((void**)&ctx->d_region_base, (size_t)MSM377_NUM_WINDOWS * (NRANGE + 1) * 4);
  dalloc((void**)&ctx->d_sort_temp, cap * MSM377_NUM_WINDOWS * sizeof(SortElem));
  dalloc((void**)&ctx->d_row_ptr, (size_t)MSM377_NUM_WINDOWS * RP * 4);
  dalloc((void**)&ctx->d_val_idx, wcap * 4);
  dalloc((void**)&ctx->d_buckets, (size_t)MSM377_NUM_WINDOWS * BKT_WORDS * NB * 4);
  dalloc((void**)&ctx->d_partials, (size_t)2 * SLOT_WORDS * 4);
  // extra work items / overflow slots beyond one per row: entries / SEG_MIN on the main path, entries / NARROW_SEG on the narrow one
  const uint64_t extra_items = std::max<uint64_t>((uint64_t)MSM377_NUM_WINDOWS * cap / SEG_MIN, (uint64_t)NARROW_EVEN_WINDOWS * std::min<uint64_t>(cap, SMALL_SORT_MAX) / NARROW_SEG) + 2;
  dalloc((void**)&ctx->d_work, ((size_t)MSM377_NUM_WINDOWS * NB + extra_items) * sizeof(WorkItem));
  dalloc((void**)&ctx->d_work_meta, (size_t)META_BLOCK_WORDS * 4);
  dalloc((void**)&ctx->d_row_ovf_base, (size_t)MSM377_NUM_WINDOWS * NB * 4);
  dalloc((void**)&ctx->d_split_rows, (size_t)MSM377_NUM_WINDOWS * NB * 4);
  dalloc((void**)&ctx->d_ovf, (size_t)extra_items * BKT_WORDS * 4);
  AffineConvert& aff = ctx->aff;
  ZeroCopyOut& zc = ctx->zc;
  const size_t aff_blocks = (size_t)affine_blocks(cap) + 1;
  dalloc((void**)&aff.d_count, 64);
  ok = ok && hipMemset(aff.d_count, 0, 64) == hipSuccess;
  dalloc((void**)&aff.d_stash, (size_t)affine_blocks(cap) * AFF_BLOCK_POINTS * AFF_STASH_WORDS * 4);  // whole workgroups: the stash is piece-major per workgroup
  dalloc((void**)&aff.d_trees, aff_blocks * 2 * AFF_THREADS * 13 * 4);
  const unsigned host_flags = hipHostMallocMapped | hipHostMallocCoherent;
  ok = ok && own.alloc_pinned((void**)&aff.h_prod, aff_blocks * 48, host_flags) == hipSuccess &&
       own.alloc_pinned((void**)&aff.h_inv, aff_blocks * 48, host_flags) == hipSuccess &&
       own.alloc_pinned((void**)&aff.h_flag, 64, host_flags) == hipSuccess &&
       hipHostGetDevicePointer((void**)&aff.dm_prod, aff.h_prod, 0) == hipSuccess &&
       hipHostGetDevicePointer((void**)&aff.dm_inv, aff.h_inv, 0) == hipSuccess &&
       hipHostGetDevicePointer((void**)&aff.dm_flag, aff.h_flag, 0) == hipSuccess &&
       own.event(&aff.up_done, hipEventDisableTiming) == hipSuccess;
  if (ok) aff.scratch.resize(aff_blocks);
  dalloc((void**)&ctx->d_err, 4 * sizeof(int));  // [0], [1]: the two double-buffer slots; [2]: base conversion (lives with the table)
  ok = ok && own.alloc_pinned((void**)&ctx->h_partials, (size_t)2 * SLOT_WORDS * 4, host_flags) == hipSuccess &&
       hipHostGetDevicePointer((void**)&zc.dm_partials, ctx->h_partials, 0) == hipSuccess &&
       own.alloc_pinned((void**)&zc.h_flag, 64, host_flags) == hipSuccess &&
       hipHostGetDevicePointer((void**)&zc.dm_flag, zc.h_flag, 0) == hipSuccess;
  if (ok) memset(zc.h_flag, 0, 64);
  dalloc((void**)&zc.d_count, 64);
  ok = ok && hipMemset(zc.d_count, 0, 64) == hipSuccess;
  ok = ok && own.alloc_pinned((void**)&ctx->h_err, 2 * sizeof(int)) == hipSuccess;
  for (int k = 0; ok && k < 2; k++) ok = ok && own.event(&ctx->done_ev[k], hipEventDisableTiming) == hipSuccess;
  for (int s = 0; ok && s < MSM377_NUM_STAGES; s++)
    for (int k = 0; k < 2; k++) ok = ok && own.event(&ctx->ev[s][k]) == hipSuccess;
  if (!ok) {
    ctx_destroy(ctx);
    return MSM377_ENOMEM;
  }
  *out = ctx;
  return MSM377_OK;
}

void ctx_destroy(msm377_ctx* ctx) {
  if (!ctx) return;
  ctx->tail_pool.shutdown();  // first: a share left running by a timed-out tail wait may still use the buffers below
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  if (ctx->twin) {  // it owns everything but the resident bases it borrows during a batch call
    twin_return(ctx);
    ctx_destroy(ctx->twin);
    ctx->twin = nullptr;
  }
  ctx->own.release_all();
  delete ctx;
}

int set_stage_capture(msm377_ctx* ctx, int enabled) {
  if (!ctx || enabled < 0 || enabled > 2) return MSM377_EINVAL;
  if (enabled && !ctx->d_buckets_snap) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->own.alloc((void**)&ctx->d_buckets_snap, (size_t)MSM377_NUM_WINDOWS * BKT_WORDS * NB * 4) != hipSuccess) return MSM377_ENOMEM;
  }
  ctx->capture = enabled;
  ctx->last.stage.valid = false;  // what an earlier call left was captured (or not) under another mode
  return MSM377_OK;
}

// The pinned staging buffer (128 bytes per point of capacity) and the copy streams of the host-buffer entry points.
// h2d_staged allocates them on first use -- which made the FIRST host-buffer call of a context ~35 ms; a caller that
// cares calls this right after msm377_ctx_create.
int reserve_host_staging(msm377_ctx* ctx) {
  if (!ctx) return MSM377_EINVAL;
  HostStaging& st = ctx->staging;
  if (st.h_stage) return MSM377_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->own.alloc_pinned((void**)&st.h_stage, (size_t)ctx->cap * 128) != hipSuccess) {
    ctx->err = "host staging buffer: out of pinned memory";
    return MSM377_ENOMEM;
  }
  for (int t = 0; t < 8; t++)
    if (!st.copy_stream[t]) HIP_TRY(ctx, ctx->own.stream(&st.copy_stream[t]));
  return MSM377_OK;
}

int ensure_import_buffers(msm377_ctx* ctx, bool host_staging) {
  NativeImport& nat = ctx->native;
  if (!nat.import_done) HIP_TRY(ctx, ctx->own.event(&nat.import_done, hipEventDisableTiming));
  if (!nat.d_inf_mask && ctx->own.alloc((void**)&nat.d_inf_mask, (2 * nat.mask_words() + 4) * 4) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "native input forms: out of device memory";
    return MSM377_ENOMEM;
  }
  if (host_staging && !nat.d_native && ctx->own.alloc((void**)&nat.d_native, nat.points_bytes() + (size_t)ctx->cap * 32) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "native input forms: out of device memory for the host-buffer staging";
    return MSM377_ENOMEM;
  }
  return MSM377_OK;
}

int bm_alloc(msm377_ctx* ctx, uint32_t** p, size_t bytes) {
  if (*p) return MSM377_OK;
  if (ctx->own.alloc((void**)p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "out of device memory for the batch multiplication scratch";
    return MSM377_ENOMEM;
  }
  return MSM377_OK;
}

}  // namespace eng
}  // namespace msm377
