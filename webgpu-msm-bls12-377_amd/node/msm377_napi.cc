// N-API shim: the thin native layer between the reference's TypeScript host code and the
// C ABI (include/msm377.h).  It replaces the WebGPU dispatch path behind compute_msm
// (/root/reference/src/submission/submission.ts:113-288: get_device, the five stage drivers,
// read_from_gpu) with ONE native call; compute_msm.ts / compute_msm.js in this directory keep
// the entry point's name, arguments and result.
//
// Exports (CommonJS addon, N-API >= 6 for BigInt-free Buffers only -- BigInt conversion is done
// in JS):
//   computeMsm(points: Buffer, scalars: Buffer): Promise<Buffer>   96-byte x||y, runs off the JS thread
//   computeMsmSync(points: Buffer, scalars: Buffer): Buffer
//   computeMsmShortSync(points: Buffer 96n, scalars: Buffer scalarBytes x n, scalarBytes, scalarBits): Buffer
//                                                                      compact scalars below 2^scalarBits (msm377_g1_msm_short)
//   computeEdMsmSync(points: Buffer 64n, scalars: Buffer 32n): Buffer   the Edwards-BLS12 twin (msm377_ed_msm), 64-byte x||y
//   setBasesSync(points: Buffer 96n): void                             fixed-base batches: keep a converted base set in HBM ...
//   fixedBaseMsmSync(scalars: Buffer 32n): Buffer                      ... and run MSMs of n <= its size against it
//   checkPointsSync(points: Buffer 96n, flags: number): object         input validation (msm377_g1_check_points): the report's
//                                                                      64-bit fields as BigInt, firstBad null if none
//   batchMulSync(base: Buffer 96, scalars: Buffer 32n, outForm: number): {points: Buffer, infinity: Buffer}
//                                                                      out[i] = [s_i]B (msm377_g1_batch_mul): 96-byte wire or
//                                                                      104-byte mont_flag records, one identity byte per output
//   batchMulVarSync(points: Buffer 96n, scalars: Buffer 32n | 32, outForm: number): {points: Buffer, infinity: Buffer}
//                                                                      out[i] = [s_i]P_i (msm377_g1_batch_mul_var); 32 bytes of
//                                                                      scalars for n > 1 points: one scalar for all
//   batchLincomb2Sync(p: Buffer 96n, q: Buffer 96n, a: Buffer 32n | 32, b: Buffer 32n | 32, outForm: number): {points, infinity}
//                                                                      out[i] = [a_i]P_i + [b_i]Q_i (msm377_g1_batch_lincomb2)
//   batchMulMultiSync(bases: Buffer 96k, scalars: Buffer 32kn, outForm: number, columns: number): {points, infinity}
//                                                                      out[i] = sum_j [s_ij]B_j (msm377_g1_batch_mul_multi); the
//                                                                      k x n scalars row-major, or column-major if columns != 0
//   edBatchMulMultiSync(bases: Buffer 64k, scalars: Buffer 32kn, columns: number): Buffer 64n
//                                                                      out[i] = sum_j [s_ij]B_j on Edwards-BLS12
//                                                                      (msm377_ed_batch_mul_multi), 64-byte records x || y
//   edBatchMulVarSync(points: Buffer, scalars: Buffer) -> Buffer     out[i] = [s_i]P_i on Edwards-BLS12 (msm377_ed_batch_mul_var)
//   edBatchLincomb2Sync(p: Buffer 64n | 64, q: Buffer 64n | 64, a: Buffer 32n | 32, b: Buffer 32n | 32) -> Buffer 64n
//                                                                      out[i] = [a_i]P_i + [b_i]Q_i on Edwards-BLS12
//                                                                      (msm377_ed_batch_lincomb2)
//   edBatchLincombSync(points: Buffer[k], scalars: Buffer[k]) -> Buffer 64n
//                                                                      out[i] = sum_j [s_ij]P_ij on Edwards-BLS12, 1 <= k <= 8
//                                                                      (msm377_ed_batch_lincomb); each Buffer n elements or ONE
//   setGeneratorsSync(gens: Buffer 96k, windowBits: number): void       row commitments: build and keep the window tables of k
//                                                                      generators (msm377_g1_set_generators); an empty Buffer
//                                                                      drops the set
//   commitRowsSync(scalars: Buffer 32kn, k: number, outForm: number, columns: number): {points, infinity}
//                                                                      out[i] = sum_j [s_ij]G_j over the first k generators of
//                                                                      the set (msm377_g1_commit_rows); the k x n scalars
//                                                                      row-major, or column-major if columns != 0
//   edSetGeneratorsSync(gens: Buffer 64k, windowBits: number): void     Edwards-BLS12 row commitments: build and keep the
//                                                                      window tables of k generators (msm377_ed_set_generators);
//                                                                      an empty Buffer drops the set
//   edCommitRowsSync(scalars: Buffer 32kn, k: number, columns: number): Buffer 64n
//                                                                      out[i] = sum_j [s_ij]G_j over the first k generators of
//                                                                      that set (msm377_ed_commit_rows), 64-byte records x || y
//   version(): string
// Errors reject / throw a JS Error carrying msm377_strerror + msm377_last_error, matching the
// reference's behaviour of throwing Error (cuzk/gpu.ts:7-10).
#define NAPI_VERSION 6
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>

#include "../../include/msm377.h"

namespace {

std::mutex g_mu;  // one call in flight per context (msm377.h)
msm377_ctx* g_ctx = nullptr;
uint64_t g_cap = 0;

int ensure_ctx(uint64_t n, std::string* err) {
  if (g_ctx && g_cap >= n) return MSM377_OK;
  if (g_ctx) {
    msm377_ctx_destroy(g_ctx);
    g_ctx = nullptr;
    g_cap = 0;
  }
  uint64_t cap = 1ull << 16;  // the harness's smallest case (README.md:90)
  while (cap < n) cap <<= 1;
  int device = 0;
  if (const char* d = getenv("MSM377_DEVICE")) device = atoi(d);
  int rc = msm377_ctx_create(device, cap, &g_ctx);
  if (rc) {
    *err = std::string("msm377_ctx_create: ") + msm377_strerror(rc) + " (no usable HIP device? there is no CPU fallback)";
    return rc;
  }
  g_cap = cap;
  return MSM377_OK;
}

int run(const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out[96], std::string* err) {
  std::lock_guard<std::mutex> lock(g_mu);
  int rc = ensure_ctx(n ? n : 1, err);
  if (rc) return rc;
  rc = msm377_g1_msm(g_ctx, points, scalars, n, out);
  if (rc) *err = std::string("msm377_g1_msm: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
  return rc;
}

bool get_buffers(napi_env env, napi_callback_info info, uint8_t** p, size_t* pl, uint8_t** s, size_t* sl, size_t point_bytes = 96) {
  size_t argc = 2;
  napi_value argv[2];
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer, scalars: Buffer)");
    return false;
  }
  bool is_buf = false;
  for (int i = 0; i < 2; i++) {
    if (napi_is_buffer(env, argv[i], &is_buf) != napi_ok || !is_buf) {
      napi_throw_type_error(env, nullptr, "points and scalars must be Buffers");
      return false;
    }
  }
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(p), pl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(s), sl);
  if (*sl % 32 != 0 || *pl != (*sl / 32) * point_bytes) {
    napi_throw_range_error(env, nullptr, point_bytes == 96 ? "points must hold 96 bytes and scalars 32 bytes per input" : "points must hold 64 bytes and scalars 32 bytes per input");
    return false;
  }
  return true;
}

napi_value ComputeMsmSync(napi_env env, napi_callback_info info) {
  uint8_t *p, *s;
  size_t pl, sl;
  if (!get_buffers(env, info, &p, &pl, &s, &sl)) return nullptr;
  uint8_t out[96];
  std::string err;
  if (run(p, s, sl / 32, out, &err)) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_value buf;
  void* data;
  napi_create_buffer_copy(env, 96, out, &data, &buf);
  return buf;
}

// computeMsmShortSync(points, scalars, scalarBytes, scalarBits): compact scalars of a declared width (msm377_g1_msm_short)
napi_value ComputeMsmShortSync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  bool pb = false, sb = false;
  uint32_t sbytes = 0, sbits = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 4 || napi_is_buffer(env, argv[0], &pb) != napi_ok || !pb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb || napi_get_value_uint32(env, argv[2], &sbytes) != napi_ok ||
      napi_get_value_uint32(env, argv[3], &sbits) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer, scalars: Buffer, scalarBytes: number, scalarBits: number)");
    return nullptr;
  }
  uint8_t *p, *s;
  size_t pl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&p), &pl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  if ((sbytes != 4 && sbytes != 8 && sbytes != 16 && sbytes != 32) || sl % sbytes != 0 || pl != (sl / sbytes) * 96) {
    napi_throw_range_error(env, nullptr, "scalarBytes must be 4, 8, 16 or 32; points must hold 96 bytes and scalars scalarBytes bytes per input");
    return nullptr;
  }
  const uint64_t n = sl / sbytes;
  uint8_t out[96];
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(n ? n : 1, &err);
    if (!rc) {
      rc = msm377_g1_msm_short(g_ctx, p, s, n, sbytes, sbits, out);
      if (rc) err = std::string("msm377_g1_msm_short: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_value buf;
  void* data;
  napi_create_buffer_copy(env, 96, out, &data, &buf);
  return buf;
}

// computeMsmNativeSync(points, scalars, pointForm, scalarForm): the callers' native forms (msm377_ctx_set_input_format:
// MSM377_POINTS_* / MSM377_SCALARS_* values) for this one call; the shared context goes back to the wire format.
napi_value ComputeMsmNativeSync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  bool pb = false, sb = false;
  uint32_t pform = 0, sform = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 4 || napi_is_buffer(env, argv[0], &pb) != napi_ok || !pb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb || napi_get_value_uint32(env, argv[2], &pform) != napi_ok ||
      napi_get_value_uint32(env, argv[3], &sform) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer, scalars: Buffer, pointForm: number, scalarForm: number)");
    return nullptr;
  }
  uint8_t *p, *s;
  size_t pl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&p), &pl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  const size_t stride = pform == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  if (pform > MSM377_POINTS_MONT_FLAG || sform > MSM377_SCALARS_MONT || sl % 32 != 0 || pl != (sl / 32) * stride) {
    napi_throw_range_error(env, nullptr, "pointForm 0..2, scalarForm 0..1; points must hold 96 (104 with flags) bytes and scalars 32 bytes per input");
    return nullptr;
  }
  const uint64_t n = sl / 32;
  uint8_t out[96];
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(n ? n : 1, &err);
    if (!rc) {
      rc = msm377_ctx_set_input_format(g_ctx, pform, sform);
      if (!rc) rc = msm377_g1_msm(g_ctx, p, s, n, out);
      if (rc) err = std::string("msm377_g1_msm (native input forms): ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
      msm377_ctx_set_input_format(g_ctx, MSM377_POINTS_WIRE, MSM377_SCALARS_WIRE);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_value buf;
  void* data;
  napi_create_buffer_copy(env, 96, out, &data, &buf);
  return buf;
}

// ---- the other entry points of the C ABI a TypeScript host may want (synchronous forms) ----
napi_value ComputeEdMsmSync(napi_env env, napi_callback_info info) {
  uint8_t *p, *s;
  size_t pl, sl;
  if (!get_buffers(env, info, &p, &pl, &s, &sl, 64)) return nullptr;
  uint8_t out[64];
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(sl / 32 ? sl / 32 : 1, &err);
    if (!rc) {
      rc = msm377_ed_msm(g_ctx, p, s, sl / 32, out);
      if (rc) err = std::string("msm377_ed_msm: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_value buf;
  void* data;
  napi_create_buffer_copy(env, 64, out, &data, &buf);
  return buf;
}

bool one_buffer(napi_env env, napi_callback_info info, uint8_t** p, size_t* len, size_t unit, const char* what) {
  size_t argc = 1;
  napi_value argv[1];
  bool is_buf = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || napi_is_buffer(env, argv[0], &is_buf) != napi_ok || !is_buf) {
    napi_throw_type_error(env, nullptr, what);
    return false;
  }
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(p), len);
  if (*len % unit) {
    napi_throw_range_error(env, nullptr, what);
    return false;
  }
  return true;
}

napi_value SetBasesSync(napi_env env, napi_callback_info info) {
  uint8_t* p;
  size_t len;
  if (!one_buffer(env, info, &p, &len, 96, "expected (points: Buffer of 96 bytes per point)")) return nullptr;
  std::string err;
  std::lock_guard<std::mutex> lock(g_mu);
  int rc = ensure_ctx(len / 96 ? len / 96 : 1, &err);
  if (!rc) {
    rc = msm377_g1_set_bases(g_ctx, p, len / 96);
    if (rc) err = std::string("msm377_g1_set_bases: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
  }
  if (rc) napi_throw_error(env, nullptr, err.c_str());
  return nullptr;
}

napi_value FixedBaseMsmSync(napi_env env, napi_callback_info info) {
  uint8_t* s;
  size_t len;
  if (!one_buffer(env, info, &s, &len, 32, "expected (scalars: Buffer of 32 bytes per scalar)")) return nullptr;
  uint8_t out[96];
  std::string err;
  int rc = MSM377_ESTATE;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (!g_ctx || g_cap < len / 32) {
      err = "fixedBaseMsmSync: call setBasesSync with at least as many points first";
    } else {
      rc = msm377_g1_msm_fixed_base(g_ctx, s, len / 32, out);
      if (rc) err = std::string("msm377_g1_msm_fixed_base: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_value buf;
  void* data;
  napi_create_buffer_copy(env, 96, out, &data, &buf);
  return buf;
}

// checkPointsSync(points, flags) -> {checked, noncanonical, off_curve, outside_subgroup, first_bad, first_bad_reason}
napi_value CheckPointsSync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  bool is_buf = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 1 || napi_is_buffer(env, argv[0], &is_buf) != napi_ok || !is_buf) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer of 96 bytes per point, flags?: number)");
    return nullptr;
  }
  uint8_t* p;
  size_t len;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&p), &len);
  uint32_t flags = MSM377_CHECK_ALL;
  if (argc >= 2) {
    napi_valuetype t;
    if (napi_typeof(env, argv[1], &t) == napi_ok && t != napi_undefined && napi_get_value_uint32(env, argv[1], &flags) != napi_ok) {
      napi_throw_type_error(env, nullptr, "flags must be a number (MSM377_CHECK_* bits)");
      return nullptr;
    }
  }
  if (len % 96) {
    napi_throw_range_error(env, nullptr, "points must hold 96 bytes per point");
    return nullptr;
  }
  msm377_check_report rep;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(len / 96 ? len / 96 : 1, &err);
    if (!rc) {
      rc = msm377_g1_check_points(g_ctx, p, len / 96, flags, &rep);
      if (rc) err = std::string("msm377_g1_check_points: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_value obj, v;
  napi_create_object(env, &obj);
  const struct {
    const char* name;
    uint64_t value;
  } fields[] = {{"checked", rep.checked}, {"noncanonical", rep.noncanonical}, {"off_curve", rep.off_curve}, {"outside_subgroup", rep.outside_subgroup}};
  for (const auto& f : fields) {
    napi_create_bigint_uint64(env, f.value, &v);
    napi_set_named_property(env, obj, f.name, v);
  }
  if (rep.first_bad == UINT64_MAX) napi_get_null(env, &v);
  else napi_create_bigint_uint64(env, rep.first_bad, &v);
  napi_set_named_property(env, obj, "first_bad", v);
  napi_create_uint32(env, rep.first_bad_reason, &v);
  napi_set_named_property(env, obj, "first_bad_reason", v);
  return obj;
}

// batchMulSync(base, scalars, outForm) -> {points, infinity}: n multiples of one base, each its own point
napi_value BatchMulSync(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  bool bb = false, sb = false;
  uint32_t form = MSM377_POINTS_WIRE;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3 || napi_is_buffer(env, argv[0], &bb) != napi_ok || !bb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb || napi_get_value_uint32(env, argv[2], &form) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (base: Buffer of 96 bytes, scalars: Buffer of 32 bytes per scalar, outForm: number)");
    return nullptr;
  }
  uint8_t *b, *s;
  size_t bl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&b), &bl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  if (bl != 96 || sl % 32 != 0 || (form != MSM377_POINTS_WIRE && form != MSM377_POINTS_MONT_FLAG)) {
    napi_throw_range_error(env, nullptr, "base must hold 96 bytes, scalars 32 bytes each; outForm is 0 (wire) or 2 (mont_flag)");
    return nullptr;
  }
  const uint64_t n = sl / 32;
  const size_t stride = form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  napi_value points, infinity, obj;
  void *pd = nullptr, *id = nullptr;
  if (napi_create_buffer(env, n * stride, &pd, &points) != napi_ok || napi_create_buffer(env, n, &id, &infinity) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in chunks of its own
    if (!rc) {
      rc = msm377_g1_batch_mul(g_ctx, b, s, n, form, static_cast<uint8_t*>(pd), static_cast<uint8_t*>(id));
      if (rc) err = std::string("msm377_g1_batch_mul: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "points", points);
  napi_set_named_property(env, obj, "infinity", infinity);
  return obj;
}

// batchMulVarSync(points, scalars, outForm) -> {points, infinity}: out[i] = [s_i]P_i on wire points; 32 bytes of scalars
// for more than one point are the ONE scalar of all points (scalar_stride 0)
napi_value BatchMulVarSync(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  bool pb = false, sb = false;
  uint32_t form = MSM377_POINTS_WIRE;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3 || napi_is_buffer(env, argv[0], &pb) != napi_ok || !pb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb || napi_get_value_uint32(env, argv[2], &form) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer of 96 bytes per point, scalars: Buffer of 32 bytes per scalar, outForm: number)");
    return nullptr;
  }
  uint8_t *p, *s;
  size_t pl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&p), &pl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  const uint64_t n = pl / 96;
  const uint32_t scalar_stride = (sl == 32 && n > 1) ? 0 : 32;
  if (pl % 96 != 0 || (scalar_stride && sl != n * 32) || (form != MSM377_POINTS_WIRE && form != MSM377_POINTS_MONT_FLAG)) {
    napi_throw_range_error(env, nullptr, "points must hold 96 bytes each, scalars 32 bytes per point (or 32 bytes for all); outForm is 0 (wire) or 2 (mont_flag)");
    return nullptr;
  }
  const size_t stride = form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  napi_value points, infinity, obj;
  void *pd = nullptr, *id = nullptr;
  if (napi_create_buffer(env, n * stride, &pd, &points) != napi_ok || napi_create_buffer(env, n, &id, &infinity) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_g1_batch_mul_var(g_ctx, p, s, n, scalar_stride, form, static_cast<uint8_t*>(pd), static_cast<uint8_t*>(id));
      if (rc) err = std::string("msm377_g1_batch_mul_var: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "points", points);
  napi_set_named_property(env, obj, "infinity", infinity);
  return obj;
}

// batchLincomb2Sync(p, q, a, b, outForm) -> {points, infinity}: out[i] = [a_i]P_i + [b_i]Q_i on wire points; 32 bytes of a
// or of b for more than one pair are the ONE scalar of all pairs (stride 0)
napi_value BatchLincomb2Sync(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  uint32_t form = MSM377_POINTS_WIRE;
  bool ok = napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) == napi_ok && argc >= 5;
  for (int k = 0; ok && k < 4; k++) {
    bool is = false;
    ok = napi_is_buffer(env, argv[k], &is) == napi_ok && is;
  }
  if (!ok || napi_get_value_uint32(env, argv[4], &form) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (p, q: Buffers of 96 bytes per point, a, b: Buffers of 32 bytes per scalar, outForm: number)");
    return nullptr;
  }
  uint8_t* in[4];
  size_t len[4];
  for (int k = 0; k < 4; k++) napi_get_buffer_info(env, argv[k], reinterpret_cast<void**>(&in[k]), &len[k]);
  const uint64_t n = len[0] / 96;
  const uint32_t a_stride = (len[2] == 32 && n > 1) ? 0 : 32, b_stride = (len[3] == 32 && n > 1) ? 0 : 32;
  if (len[0] % 96 != 0 || len[1] != len[0] || (a_stride && len[2] != n * 32) || (b_stride && len[3] != n * 32) || (form != MSM377_POINTS_WIRE && form != MSM377_POINTS_MONT_FLAG)) {
    napi_throw_range_error(env, nullptr, "p and q must hold the same number of 96-byte points, a and b 32 bytes per pair (or 32 bytes for all); outForm is 0 (wire) or 2 (mont_flag)");
    return nullptr;
  }
  const size_t stride = form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  napi_value points, infinity, obj;
  void *pd = nullptr, *id = nullptr;
  if (napi_create_buffer(env, n * stride, &pd, &points) != napi_ok || napi_create_buffer(env, n, &id, &infinity) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_g1_batch_lincomb2(g_ctx, in[0], in[1], in[2], in[3], n, a_stride, b_stride, form, static_cast<uint8_t*>(pd), static_cast<uint8_t*>(id));
      if (rc) err = std::string("msm377_g1_batch_lincomb2: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "points", points);
  napi_set_named_property(env, obj, "infinity", infinity);
  return obj;
}

// batchMulMultiSync(bases, scalars, outForm, columns) -> {points, infinity}: out[i] = sum_j [s_ij]B_j over k = bases / 96 fixed
// bases; scalars: the dense k x n matrix, row-major (columns = 0) or column-major
napi_value BatchMulMultiSync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  bool bb = false, sb = false;
  uint32_t form = MSM377_POINTS_WIRE, columns = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 4 || napi_is_buffer(env, argv[0], &bb) != napi_ok || !bb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb || napi_get_value_uint32(env, argv[2], &form) != napi_ok || napi_get_value_uint32(env, argv[3], &columns) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (bases: Buffer of 96 bytes per base, scalars: Buffer of 32 bytes per scalar, outForm: number, columns: number)");
    return nullptr;
  }
  uint8_t *b, *s;
  size_t bl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&b), &bl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  const uint32_t k = static_cast<uint32_t>(bl / 96);
  if (bl % 96 != 0 || k < 1 || k > MSM377_MUL_MAX_BASES || sl % (32 * static_cast<size_t>(k)) != 0 || (form != MSM377_POINTS_WIRE && form != MSM377_POINTS_MONT_FLAG)) {
    napi_throw_range_error(env, nullptr, "bases must hold 1 to 16 points of 96 bytes, scalars 32 bytes per base and output; outForm is 0 (wire) or 2 (mont_flag)");
    return nullptr;
  }
  const uint64_t n = sl / (32 * static_cast<size_t>(k));
  const uint64_t out_stride = columns ? 32 : 32 * static_cast<uint64_t>(k), base_stride = columns ? 32 * (n ? n : 1) : 32;
  const size_t stride = form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  napi_value points, infinity, obj;
  void *pd = nullptr, *id = nullptr;
  if (napi_create_buffer(env, n * stride, &pd, &points) != napi_ok || napi_create_buffer(env, n, &id, &infinity) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_g1_batch_mul_multi(g_ctx, b, k, s, n, out_stride, base_stride, form, static_cast<uint8_t*>(pd), static_cast<uint8_t*>(id));
      if (rc) err = std::string("msm377_g1_batch_mul_multi: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "points", points);
  napi_set_named_property(env, obj, "infinity", infinity);
  return obj;
}

// edBatchMulMultiSync(bases, scalars, columns) -> Buffer: out[i] = sum_j [s_ij]B_j on Edwards-BLS12 over k = bases / 64 fixed
// bases (msm377_ed_batch_mul_multi); scalars: the dense k x n matrix, row-major (columns = 0) or column-major; n records of
// 64 bytes x || y, the identity as (0, 1)
napi_value EdBatchMulMultiSync(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  bool bb = false, sb = false;
  uint32_t columns = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3 || napi_is_buffer(env, argv[0], &bb) != napi_ok || !bb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb || napi_get_value_uint32(env, argv[2], &columns) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (bases: Buffer of 64 bytes per base, scalars: Buffer of 32 bytes per scalar, columns: number)");
    return nullptr;
  }
  uint8_t *b, *s;
  size_t bl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&b), &bl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  const uint32_t k = static_cast<uint32_t>(bl / 64);
  if (bl % 64 != 0 || k < 1 || k > MSM377_MUL_MAX_BASES || sl % (32 * static_cast<size_t>(k)) != 0) {
    napi_throw_range_error(env, nullptr, "bases must hold 1 to 16 points of 64 bytes, scalars 32 bytes per base and output");
    return nullptr;
  }
  const uint64_t n = sl / (32 * static_cast<size_t>(k));
  const uint64_t out_stride = columns ? 32 : 32 * static_cast<uint64_t>(k), base_stride = columns ? 32 * (n ? n : 1) : 32;
  napi_value points;
  void* pd = nullptr;
  if (napi_create_buffer(env, n * 64, &pd, &points) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_ed_batch_mul_multi(g_ctx, b, k, s, n, out_stride, base_stride, static_cast<uint8_t*>(pd));
      if (rc) err = std::string("msm377_ed_batch_mul_multi: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  return points;
}

// edBatchMulVarSync(points, scalars) -> Buffer: out[i] = [s_i]P_i on Edwards-BLS12 (msm377_ed_batch_mul_var); points: 64 bytes
// x || y each, scalars: 32 bytes per point, or 32 bytes of ONE scalar for all; n records of 64 bytes, the identity as (0, 1).
// A point that is not on the curve throws, with the index in the text
napi_value EdBatchMulVarSync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  bool pb = false, sb = false;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_is_buffer(env, argv[0], &pb) != napi_ok || !pb ||
      napi_is_buffer(env, argv[1], &sb) != napi_ok || !sb) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer of 64 bytes per point, scalars: Buffer of 32 bytes per point or 32 bytes)");
    return nullptr;
  }
  uint8_t *p, *s;
  size_t pl, sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&p), &pl);
  napi_get_buffer_info(env, argv[1], reinterpret_cast<void**>(&s), &sl);
  const uint64_t n = pl / 64;
  const uint32_t scalar_stride = (sl == 32 && n > 1) ? 0 : 32;
  if (pl % 64 != 0 || (scalar_stride && sl != n * 32)) {
    napi_throw_range_error(env, nullptr, "points must hold 64 bytes each, scalars 32 bytes per point or 32 bytes for all");
    return nullptr;
  }
  napi_value points;
  void* pd = nullptr;
  if (napi_create_buffer(env, n * 64, &pd, &points) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_ed_batch_mul_var(g_ctx, p, s, n, scalar_stride, static_cast<uint8_t*>(pd));
      if (rc) err = std::string("msm377_ed_batch_mul_var: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  return points;
}

// edBatchLincomb2Sync(p, q, a, b) -> Buffer: out[i] = [a_i]P_i + [b_i]Q_i on Edwards-BLS12 (msm377_ed_batch_lincomb2); p, q:
// 64 bytes x || y each, a, b: 32 bytes each; n is the largest element count, an argument of exactly ONE element with n > 1
// stands for all pairs (stride 0); n records of 64 bytes, the identity as (0, 1).  A point that is not on the curve throws,
// with the array and the index in the text
napi_value EdBatchLincomb2Sync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  bool ok = napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) == napi_ok && argc >= 4;
  for (int i = 0; ok && i < 4; i++) {
    bool is = false;
    ok = napi_is_buffer(env, argv[i], &is) == napi_ok && is;
  }
  if (!ok) {
    napi_throw_type_error(env, nullptr, "expected (p: Buffer, q: Buffer, a: Buffer, b: Buffer): 64 bytes per point, 32 per scalar");
    return nullptr;
  }
  uint8_t* in[4];
  size_t len[4];
  const size_t size[4] = {64, 64, 32, 32};
  uint64_t n = 0;
  for (int i = 0; i < 4; i++) {
    napi_get_buffer_info(env, argv[i], reinterpret_cast<void**>(&in[i]), &len[i]);
    ok = ok && len[i] % size[i] == 0;
    if (len[i] / size[i] > n) n = len[i] / size[i];
  }
  uint32_t stride[4];
  for (int i = 0; i < 4; i++) {
    const uint64_t count = len[i] / size[i];
    stride[i] = count == n ? (uint32_t)size[i] : 0;
    ok = ok && (count == n || (count == 1 && n > 1));
  }
  if (!ok) {
    napi_throw_range_error(env, nullptr, "p, q hold 64 bytes per point, a, b 32 per scalar: one element per pair, or exactly one element for all pairs");
    return nullptr;
  }
  napi_value points;
  void* pd = nullptr;
  if (napi_create_buffer(env, n * 64, &pd, &points) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_ed_batch_lincomb2(g_ctx, in[0], in[1], in[2], in[3], n, stride[0], stride[1], stride[2], stride[3], static_cast<uint8_t*>(pd));
      if (rc) err = std::string("msm377_ed_batch_lincomb2: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  return points;
}

// edBatchLincombSync(points, scalars) -> Buffer: out[i] = sum_j [s_ij]P_ij on Edwards-BLS12 (msm377_ed_batch_lincomb); points,
// scalars: arrays of k Buffers, 64 bytes per point and 32 per scalar; n is the largest element count, a Buffer of exactly ONE
// element with n > 1 stands for all outputs (stride 0); n records of 64 bytes, the identity as (0, 1).  A point that is not
// on the curve throws, with the index and the term in the text
napi_value EdBatchLincombSync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  uint32_t k = 0, ks = 0;
  bool ok = napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) == napi_ok && argc >= 2;
  for (int i = 0; ok && i < 2; i++) {
    bool is = false;
    ok = napi_is_array(env, argv[i], &is) == napi_ok && is;
  }
  ok = ok && napi_get_array_length(env, argv[0], &k) == napi_ok && napi_get_array_length(env, argv[1], &ks) == napi_ok && k == ks && k <= MSM377_LINCOMB_MAX_TERMS;
  uint8_t* in[2][MSM377_LINCOMB_MAX_TERMS];
  size_t len[2][MSM377_LINCOMB_MAX_TERMS];
  for (int i = 0; ok && i < 2; i++)
    for (uint32_t j = 0; ok && j < k; j++) {
      napi_value el;
      bool is = false;
      ok = napi_get_element(env, argv[i], j, &el) == napi_ok && napi_is_buffer(env, el, &is) == napi_ok && is &&
           napi_get_buffer_info(env, el, reinterpret_cast<void**>(&in[i][j]), &len[i][j]) == napi_ok;
    }
  if (!ok) {
    napi_throw_type_error(env, nullptr, "expected (points: Buffer[], scalars: Buffer[]): at most 8 terms, one Buffer of points and one of scalars each");
    return nullptr;
  }
  const size_t size[2] = {64, 32};
  uint64_t n = 0;
  for (int i = 0; i < 2; i++)
    for (uint32_t j = 0; j < k; j++) {
      ok = ok && len[i][j] % size[i] == 0;
      if (len[i][j] / size[i] > n) n = len[i][j] / size[i];
    }
  msm377_lincomb_term terms[MSM377_LINCOMB_MAX_TERMS];
  for (uint32_t j = 0; j < k; j++) {
    const uint64_t cp = len[0][j] / 64, cs = len[1][j] / 32;
    ok = ok && (cp == n || (cp == 1 && n > 1)) && (cs == n || (cs == 1 && n > 1));
    terms[j] = msm377_lincomb_term{in[0][j], in[1][j], cp == n ? 64u : 0u, cs == n ? 32u : 0u};
  }
  if (!ok) {
    napi_throw_range_error(env, nullptr, "64 bytes per point, 32 per scalar: in every term one element per output, or exactly one element for all outputs");
    return nullptr;
  }
  napi_value points;
  void* pd = nullptr;
  if (napi_create_buffer(env, n * 64, &pd, &points) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity: the call walks n in passes of its own
    if (!rc) {
      rc = msm377_ed_batch_lincomb(g_ctx, terms, k, n, static_cast<uint8_t*>(pd));
      if (rc) err = std::string("msm377_ed_batch_lincomb: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  return points;
}

// setGeneratorsSync(gens, windowBits): the resident generator set of commitRowsSync; an empty Buffer drops it
napi_value SetGeneratorsSync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  bool gb = false;
  int32_t bits = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_is_buffer(env, argv[0], &gb) != napi_ok || !gb ||
      napi_get_value_int32(env, argv[1], &bits) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (gens: Buffer of 96 bytes per generator, windowBits: number)");
    return nullptr;
  }
  uint8_t* g;
  size_t gl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&g), &gl);
  if (gl % 96 != 0 || gl / 96 > MSM377_GEN_MAX) {
    napi_throw_range_error(env, nullptr, "gens must hold 0 to 4096 points of 96 bytes");
    return nullptr;
  }
  std::string err;
  std::lock_guard<std::mutex> lock(g_mu);
  int rc = ensure_ctx(1, &err);  // any capacity: the set is an allocation of its own
  if (!rc) {
    rc = msm377_g1_set_generators(g_ctx, gl ? g : nullptr, static_cast<uint32_t>(gl / 96), bits);
    if (rc) err = std::string("msm377_g1_set_generators: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
  }
  if (rc) napi_throw_error(env, nullptr, err.c_str());
  return nullptr;
}

// commitRowsSync(scalars, k, outForm, columns) -> {points, infinity}: out[i] = sum_j [s_ij]G_j over the first k generators of
// the resident set; scalars: the dense k x n matrix, row-major (columns = 0) or column-major
napi_value CommitRowsSync(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  bool sb = false;
  uint32_t k = 0, form = MSM377_POINTS_WIRE, columns = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 4 || napi_is_buffer(env, argv[0], &sb) != napi_ok || !sb ||
      napi_get_value_uint32(env, argv[1], &k) != napi_ok || napi_get_value_uint32(env, argv[2], &form) != napi_ok || napi_get_value_uint32(env, argv[3], &columns) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (scalars: Buffer of 32 bytes per scalar, k: number, outForm: number, columns: number)");
    return nullptr;
  }
  uint8_t* s;
  size_t sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&s), &sl);
  if (k < 1 || k > MSM377_GEN_MAX || sl % (32 * static_cast<size_t>(k)) != 0 || (form != MSM377_POINTS_WIRE && form != MSM377_POINTS_MONT_FLAG)) {
    napi_throw_range_error(env, nullptr, "k is 1 to 4096, scalars 32 bytes per generator and output; outForm is 0 (wire) or 2 (mont_flag)");
    return nullptr;
  }
  const uint64_t n = sl / (32 * static_cast<size_t>(k));
  const uint64_t out_stride = columns ? 32 : 32 * static_cast<uint64_t>(k), base_stride = columns ? 32 * (n ? n : 1) : 32;
  const size_t stride = form == MSM377_POINTS_MONT_FLAG ? 104 : 96;
  napi_value points, infinity, obj;
  void *pd = nullptr, *id = nullptr;
  if (napi_create_buffer(env, n * stride, &pd, &points) != napi_ok || napi_create_buffer(env, n, &id, &infinity) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity; without a set the call itself answers MSM377_ESTATE
    if (!rc) {
      rc = msm377_g1_commit_rows(g_ctx, s, n, k, out_stride, base_stride, form, static_cast<uint8_t*>(pd), static_cast<uint8_t*>(id));
      if (rc) err = std::string("msm377_g1_commit_rows: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  napi_create_object(env, &obj);
  napi_set_named_property(env, obj, "points", points);
  napi_set_named_property(env, obj, "infinity", infinity);
  return obj;
}

// edSetGeneratorsSync(gens, windowBits): the resident Edwards-BLS12 generator set of edCommitRowsSync; an empty Buffer drops
// it.  A generator that is not on the curve throws, with the index in the text
napi_value EdSetGeneratorsSync(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  bool gb = false;
  int32_t bits = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 2 || napi_is_buffer(env, argv[0], &gb) != napi_ok || !gb ||
      napi_get_value_int32(env, argv[1], &bits) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (gens: Buffer of 64 bytes per generator, windowBits: number)");
    return nullptr;
  }
  uint8_t* g;
  size_t gl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&g), &gl);
  if (gl % 64 != 0 || gl / 64 > MSM377_GEN_MAX) {
    napi_throw_range_error(env, nullptr, "gens must hold 0 to 4096 points of 64 bytes");
    return nullptr;
  }
  std::string err;
  std::lock_guard<std::mutex> lock(g_mu);
  int rc = ensure_ctx(1, &err);  // any capacity: the set is an allocation of its own
  if (!rc) {
    rc = msm377_ed_set_generators(g_ctx, gl ? g : nullptr, static_cast<uint32_t>(gl / 64), bits);
    if (rc) err = std::string("msm377_ed_set_generators: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
  }
  if (rc) napi_throw_error(env, nullptr, err.c_str());
  return nullptr;
}

// edCommitRowsSync(scalars, k, columns) -> Buffer: out[i] = sum_j [s_ij]G_j over the first k generators of the resident
// Edwards-BLS12 set; scalars: the dense k x n matrix, row-major (columns = 0) or column-major; n records of 64 bytes, the
// identity as (0, 1)
napi_value EdCommitRowsSync(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  bool sb = false;
  uint32_t k = 0, columns = 0;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3 || napi_is_buffer(env, argv[0], &sb) != napi_ok || !sb ||
      napi_get_value_uint32(env, argv[1], &k) != napi_ok || napi_get_value_uint32(env, argv[2], &columns) != napi_ok) {
    napi_throw_type_error(env, nullptr, "expected (scalars: Buffer of 32 bytes per scalar, k: number, columns: number)");
    return nullptr;
  }
  uint8_t* s;
  size_t sl;
  napi_get_buffer_info(env, argv[0], reinterpret_cast<void**>(&s), &sl);
  if (k < 1 || k > MSM377_GEN_MAX || sl % (32 * static_cast<size_t>(k)) != 0) {
    napi_throw_range_error(env, nullptr, "k is 1 to 4096, scalars 32 bytes per generator and output");
    return nullptr;
  }
  const uint64_t n = sl / (32 * static_cast<size_t>(k));
  const uint64_t out_stride = columns ? 32 : 32 * static_cast<uint64_t>(k), base_stride = columns ? 32 * (n ? n : 1) : 32;
  napi_value points;
  void* pd = nullptr;
  if (napi_create_buffer(env, n * 64, &pd, &points) != napi_ok) return nullptr;
  std::string err;
  int rc;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    rc = ensure_ctx(1, &err);  // any capacity; without a set the call itself answers MSM377_ESTATE
    if (!rc) {
      rc = msm377_ed_commit_rows(g_ctx, s, n, k, out_stride, base_stride, static_cast<uint8_t*>(pd));
      if (rc) err = std::string("msm377_ed_commit_rows: ") + msm377_strerror(rc) + ": " + msm377_last_error(g_ctx);
    }
  }
  if (rc) {
    napi_throw_error(env, nullptr, err.c_str());
    return nullptr;
  }
  return points;
}

struct Job {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref points_ref = nullptr, scalars_ref = nullptr;  // keep the caller's Buffers alive
  uint8_t *points = nullptr, *scalars = nullptr;
  uint64_t n = 0;
  uint8_t out[96];
  int rc = 0;
  std::string err;
};

void Execute(napi_env, void* data) {
  Job* j = static_cast<Job*>(data);
  j->rc = run(j->points, j->scalars, j->n, j->out, &j->err);
}

void Complete(napi_env env, napi_status, void* data) {
  Job* j = static_cast<Job*>(data);
  if (j->rc == 0) {
    napi_value buf;
    void* p;
    napi_create_buffer_copy(env, 96, j->out, &p, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  } else {
    napi_value msg, e;
    napi_create_string_utf8(env, j->err.c_str(), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, nullptr, msg, &e);
    napi_reject_deferred(env, j->deferred, e);
  }
  napi_delete_reference(env, j->points_ref);
  napi_delete_reference(env, j->scalars_ref);
  napi_delete_async_work(env, j->work);
  delete j;
}

napi_value ComputeMsm(napi_env env, napi_callback_info info) {
  uint8_t *p, *s;
  size_t pl, sl;
  if (!get_buffers(env, info, &p, &pl, &s, &sl)) return nullptr;
  size_t argc = 2;
  napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  Job* j = new Job();
  j->points = p;
  j->scalars = s;
  j->n = sl / 32;
  napi_value promise, name;
  napi_create_promise(env, &j->deferred, &promise);
  napi_create_reference(env, argv[0], 1, &j->points_ref);
  napi_create_reference(env, argv[1], 1, &j->scalars_ref);
  napi_create_string_utf8(env, "msm377.computeMsm", NAPI_AUTO_LENGTH, &name);
  napi_create_async_work(env, nullptr, name, Execute, Complete, j, &j->work);
  napi_queue_async_work(env, j->work);
  return promise;
}

napi_value Version(napi_env env, napi_callback_info) {
  napi_value v;
  napi_create_string_utf8(env, msm377_version(), NAPI_AUTO_LENGTH, &v);
  return v;
}

napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"computeMsm", nullptr, ComputeMsm, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"computeMsmSync", nullptr, ComputeMsmSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"computeMsmShortSync", nullptr, ComputeMsmShortSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"computeMsmNativeSync", nullptr, ComputeMsmNativeSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"computeEdMsmSync", nullptr, ComputeEdMsmSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setBasesSync", nullptr, SetBasesSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"fixedBaseMsmSync", nullptr, FixedBaseMsmSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"checkPointsSync", nullptr, CheckPointsSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"batchMulSync", nullptr, BatchMulSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"batchMulVarSync", nullptr, BatchMulVarSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"batchLincomb2Sync", nullptr, BatchLincomb2Sync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"batchMulMultiSync", nullptr, BatchMulMultiSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"edBatchMulMultiSync", nullptr, EdBatchMulMultiSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"edBatchMulVarSync", nullptr, EdBatchMulVarSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"edBatchLincomb2Sync", nullptr, EdBatchLincomb2Sync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"edBatchLincombSync", nullptr, EdBatchLincombSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setGeneratorsSync", nullptr, SetGeneratorsSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"commitRowsSync", nullptr, CommitRowsSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"edSetGeneratorsSync", nullptr, EdSetGeneratorsSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"edCommitRowsSync", nullptr, EdCommitRowsSync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"version", nullptr, Version, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
