// TEST INFRASTRUCTURE: the product's field and curve primitives, and the arithmetic that exists only in its kernel
// headers (te_add_quad, g1_add_quad, te_madd_quad, AffWireSource::load, the bucket-record loads and stores), run one case
// per lane -- or per lane quad -- on gfx950.  Built as libmsm377_primtest.so by csrc/Makefile, loaded by
// tests/test_primitives_gpu.py; never linked into libmsm377.so.  Every launcher takes host arrays, copies them in,
// launches 256-thread blocks over n cases, copies the results out and returns the HIP status.  The two normalise
// launchers (tests/test_normalise_gpu.py) run the batch calls' own k_bm_* / k_edbm_* kernels on a stash the caller writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "curves.hpp"
#include "ed_ext.hpp"
#include "field29.hpp"
#include "g1_xyzz.hpp"
#include "kernels/accumulate.hpp"
#include "kernels/batch_mul.hpp"
#include "kernels/convert.hpp"
#include "kernels/ed_batch_mul.hpp"
#include "kernels/reduce.hpp"
#include "primitives_ops.hpp"
#include "te377.hpp"

using namespace msm377;

namespace {

#define PT_TRY(x)                  \
  do {                             \
    hipError_t e_ = (x);           \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// Device buffers of one launcher call; freed on every way out.
struct Bufs {
  std::vector<void*> all;
  ~Bufs() {
    for (void* p : all) (void)hipFree(p);
  }
  // words u32 of device memory, from src (or filled with `fill` bytes when src is null); at least one word
  hipError_t get(uint32_t** out, const uint32_t* src, size_t words, int fill = 0) {
    void* p = nullptr;
    const size_t bytes = (words ? words : 1) * sizeof(uint32_t);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    all.push_back(p);
    *out = static_cast<uint32_t*>(p);
    if (src && words) return hipMemcpy(p, src, words * sizeof(uint32_t), hipMemcpyHostToDevice);
    return hipMemset(p, fill, bytes);
  }
};
hipError_t fetch(uint32_t* dst, const uint32_t* dev, size_t words) {
  if (!words) return hipSuccess;
  return hipMemcpy(dst, dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost);
}
uint32_t blocks_for(uint64_t threads) { return (uint32_t)((threads + 255) / 256); }
hipError_t finish_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipDeviceSynchronize();
}

// ---- one case per lane ----
template <class F>
__global__ void __launch_bounds__(256) k_field(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr uint32_t N = F::N;
  primtest::field_op<F>(op, a + N * i, b + N * i, c + N * i, d + N * i, out + N * i);
}
template <class TE>
__global__ void __launch_bounds__(256) k_te(int op, const uint32_t* p, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t* flags, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr uint32_t W = 4 * TE::F::N;
  flags[i] = primtest::te_op<TE>(op, p + W * i, q + W * i, neg[i], out + W * i);
}
__global__ void __launch_bounds__(256) k_g1(int op, const uint32_t* a, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  primtest::g1_op(op, a + 52 * i, q + 52 * i, neg[i], out + 52 * i);
}
__global__ void __launch_bounds__(256) k_ed(int op, const uint32_t* p, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  primtest::ed_op(op, p + 36 * i, q + 36 * i, neg[i], out + 36 * i);
}
// AffWireSource::load: raw = n x 24 wire words; out = n x 39 limbs (n1, n2, z); flags = its return value
__global__ void __launch_bounds__(256) k_aff_wire(const uint32_t* raw, uint32_t* out, uint32_t* flags, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const AffWireSource src{raw};
  Fp::El n1, n2, z;
  flags[i] = src.load(i, n1, n2, z) ? 1u : 0u;
  primtest::st<Fp>(out + 39 * i, n1);
  primtest::st<Fp>(out + 39 * i + 13, n2);
  primtest::st<Fp>(out + 39 * i + 26, z);
}

// ---- one case per lane quad: every lane reads both operands and writes ITS copy of the sum (4 copies per case) ----
template <class CV>
__device__ __forceinline__ typename CV::Pt packed_point(const uint32_t* p) {
  uint32_t w[CV::PT_WORDS];
#pragma unroll
  for (uint32_t j = 0; j < CV::PT_WORDS; j++) w[j] = p[j];
  return CV::from_words(w);
}
template <class CV>
__device__ __forceinline__ void put_point(uint32_t* p, const typename CV::Pt& r) {
  uint32_t w[CV::PT_WORDS];
  CV::to_words(r, w);
#pragma unroll
  for (uint32_t j = 0; j < CV::PT_WORDS; j++) p[j] = w[j];
}
template <class CV>  // add_quad: te_add_quad<Fp> (TeDev), te_add_quad<Fq> (EdDev), g1_add_quad (G1Dev)
__global__ void __launch_bounds__(256) k_add_quad(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags, uint32_t n) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t i = gid >> 2, q = threadIdx.x & 3;
  if (i >= n) return;  // whole quads leave together
  constexpr uint32_t W = CV::PT_WORDS;
  const typename CV::Pt sum = add_quad(packed_point<CV>(a + W * i), packed_point<CV>(b + W * i), q);
  put_point<CV>(out + (size_t)W * gid, sum);
  flags[gid] = CV::is_bad(sum) ? 1u : 0u;
}
// te_madd_quad the way k_accumulate_quad feeds it: lane q multiplies by coordinate q of the record (0 and 1 swapped for a
// negated point, 2 negated limb-wise).  b = PBase records, 4 N limbs.
template <class TE>
__global__ void __launch_bounds__(256) k_madd_quad(const uint32_t* a, const uint32_t* b, const uint32_t* neg, uint32_t* out, uint32_t n) {
  using F = typename TE::F;
  using K = typename TE::K;
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t i = gid >> 2, q = threadIdx.x & 3;
  if (i >= n) return;
  constexpr uint32_t N = F::N, W = 4 * N;
  typename TE::Ext p;
  p.x = primtest::ld<F>(a + W * i), p.y = primtest::ld<F>(a + W * i + N), p.t = primtest::ld<F>(a + W * i + 2 * N), p.z = primtest::ld<F>(a + W * i + 3 * N);
  const bool ng = neg[i] != 0;
  const uint32_t comp = q < 2 ? (q ^ (ng ? 1u : 0u)) : q;
  const typename F::El cur = primtest::ld<F>(b + W * i + comp * N);
  const typename F::El mine = (q == 2 && ng) ? F::kp_sub(K::KP2, cur) : cur;
  const typename TE::Ext o = te_madd_quad<F, K>(p, mine, q);
  uint32_t* dst = out + (size_t)W * gid;
  primtest::st<F>(dst, o.x), primtest::st<F>(dst + N, o.y), primtest::st<F>(dst + 2 * N, o.t), primtest::st<F>(dst + 3 * N, o.z);
}

// ---- bucket records: store_record, then (a launch later) load_record, load_record_quad and store_coord ----
template <class CV>
__global__ void __launch_bounds__(256) k_record_store(const uint32_t* in, uint32_t* rec, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  store_record<CV>(rec + (size_t)CV::BKT_WORDS * i, packed_point<CV>(in + CV::PT_WORDS * i));
}
template <class CV>
__global__ void __launch_bounds__(256) k_record_load(const uint32_t* rec, uint32_t* out_thread, uint32_t* out_quad, uint32_t* rec2, uint32_t n) {
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  const uint32_t i = gid >> 2, q = threadIdx.x & 3;
  if (i >= n) return;
  const uint32_t* r = rec + (size_t)CV::BKT_WORDS * i;
  const typename CV::Pt mine = load_record_quad<CV>(r, q);
  put_point<CV>(out_quad + (size_t)CV::PT_WORDS * gid, mine);
  if (q == 0) put_point<CV>(out_thread + (size_t)CV::PT_WORDS * i, load_record<CV>(r));
  store_coord<CV>(rec2 + (size_t)CV::BKT_WORDS * i + q * CV::COORD_WORDS, coord4(q, mine).l);
}

template <class F>
int run_field(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, uint32_t n) {
  Bufs m;
  uint32_t *da, *db, *dc, *dd, *dout;
  const size_t w = (size_t)F::N * n;
  PT_TRY(m.get(&da, a, w));
  PT_TRY(m.get(&db, b, w));
  PT_TRY(m.get(&dc, c, w));
  PT_TRY(m.get(&dd, d, w));
  PT_TRY(m.get(&dout, nullptr, w));
  if (n) k_field<F><<<blocks_for(n), 256>>>(op, da, db, dc, dd, dout, n);
  PT_TRY(finish_launch());
  return (int)fetch(out, dout, w);
}
template <class TE>
int run_te(int op, const uint32_t* p, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t* flags, uint32_t n) {
  Bufs m;
  uint32_t *dp, *dq, *dn, *dout, *df;
  const size_t w = (size_t)4 * TE::F::N * n;
  PT_TRY(m.get(&dp, p, w));
  PT_TRY(m.get(&dq, q, w));
  PT_TRY(m.get(&dn, neg, n));
  PT_TRY(m.get(&dout, nullptr, w));
  PT_TRY(m.get(&df, nullptr, n));
  if (n) k_te<TE><<<blocks_for(n), 256>>>(op, dp, dq, dn, dout, df, n);
  PT_TRY(finish_launch());
  PT_TRY(fetch(out, dout, w));
  return (int)fetch(flags, df, n);
}
template <class CV>
int run_add_quad(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags, uint32_t n) {
  Bufs m;
  uint32_t *da, *db, *dout, *df;
  const size_t w = (size_t)CV::PT_WORDS * n;
  PT_TRY(m.get(&da, a, w));
  PT_TRY(m.get(&db, b, w));
  PT_TRY(m.get(&dout, nullptr, 4 * w));
  PT_TRY(m.get(&df, nullptr, (size_t)4 * n));
  if (n) k_add_quad<CV><<<blocks_for((uint64_t)4 * n), 256>>>(da, db, dout, df, n);
  PT_TRY(finish_launch());
  PT_TRY(fetch(out, dout, 4 * w));
  return (int)fetch(flags, df, (size_t)4 * n);
}
template <class TE>
int run_madd_quad(const uint32_t* a, const uint32_t* b, const uint32_t* neg, uint32_t* out, uint32_t n) {
  Bufs m;
  uint32_t *da, *db, *dn, *dout;
  const size_t w = (size_t)4 * TE::F::N * n;
  PT_TRY(m.get(&da, a, w));
  PT_TRY(m.get(&db, b, w));
  PT_TRY(m.get(&dn, neg, n));
  PT_TRY(m.get(&dout, nullptr, 4 * w));
  if (n) k_madd_quad<TE><<<blocks_for((uint64_t)4 * n), 256>>>(da, db, dn, dout, n);
  PT_TRY(finish_launch());
  return (int)fetch(out, dout, 4 * w);
}
template <class CV>
int run_records(const uint32_t* in, uint32_t* rec, uint32_t* out_thread, uint32_t* out_quad, uint32_t* rec2, uint32_t n) {
  Bufs m;
  uint32_t *din, *drec, *dt, *dq, *drec2;
  const size_t w = (size_t)CV::PT_WORDS * n, rw = (size_t)CV::BKT_WORDS * n;
  PT_TRY(m.get(&din, in, w));
  PT_TRY(m.get(&drec, nullptr, rw, 0xff));  // all-ones: a pad word that is not written shows
  PT_TRY(m.get(&drec2, nullptr, rw, 0xff));
  PT_TRY(m.get(&dt, nullptr, w));
  PT_TRY(m.get(&dq, nullptr, 4 * w));
  if (n) k_record_store<CV><<<blocks_for(n), 256>>>(din, drec, n);
  PT_TRY(finish_launch());
  if (n) k_record_load<CV><<<blocks_for((uint64_t)4 * n), 256>>>(drec, dt, dq, drec2, n);
  PT_TRY(finish_launch());
  PT_TRY(fetch(rec, drec, rw));
  PT_TRY(fetch(rec2, drec2, rw));
  PT_TRY(fetch(out_thread, dt, w));
  return (int)fetch(out_quad, dq, 4 * w);
}


// ---- the batch calls' normalisation (k_bm_up / k_bm_across / k_bm_down, k_edbm_*) on a stash the CALLER writes ----
// The product's own kernels at the product's own launch geometry (sequencer.hip normalise()); nothing is re-implemented.
// The stash has the size the kernels' indexing needs (piece stride BM_CHUNK: BM_PIECES x 16 MiB); only the n rows of the
// point pieces are written.  The output and flag buffers are filled with 0xEE and end in a guard band that comes back too.
constexpr size_t NORM_GUARD = 256;
constexpr uint32_t NORM_MAX_N = 1u << 16;
struct NormG1 {
  static constexpr uint32_t PT_WORDS = 52, PIECES = BM_POINT_PIECES;
  static constexpr auto up = k_bm_up;
  static constexpr auto across = k_bm_across;
  static size_t record(int form) { return form == 0 ? 96 : form == 1 ? 104 : form == 2 ? 128 : 0; }
  static void down(int form, uint32_t blocks, const uint4* stash, uint64_t n, const uint32_t* trees, const uint32_t* inv, uint8_t* out, uint8_t* inf) {
    const auto k = form == 0 ? k_bm_down<MSM377_POINTS_WIRE> : form == 1 ? k_bm_down<MSM377_POINTS_MONT_FLAG> : k_bm_down<BM_FORM_TABLE>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(BM_THREADS), 0, 0, stash, n, trees, inv, out, inf);
  }
};
struct NormEd {
  static constexpr uint32_t PT_WORDS = 36, PIECES = EDBM_POINT_PIECES;
  static constexpr auto up = k_edbm_up;
  static constexpr auto across = k_edbm_across;
  static size_t record(int form) { return form == 0 ? 64 : form == 1 ? 128 : 0; }
  static void down(int form, uint32_t blocks, const uint4* stash, uint64_t n, const uint32_t* trees, const uint32_t* inv, uint8_t* out, uint8_t*) {
    const auto k = form == 0 ? k_edbm_down<EDBM_FORM_WIRE> : k_edbm_down<EDBM_FORM_TABLE>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(BM_THREADS), 0, 0, stash, n, trees, inv, out);
  }
};
static_assert(4 * NormG1::PIECES == NormG1::PT_WORDS && 4 * NormEd::PIECES == NormEd::PT_WORDS, "a point is whole pieces");
// pts: n points of PT_WORDS raw words.  out: n records + NORM_GUARD bytes.  inf: n + NORM_GUARD bytes, or null (the kernel
// then gets a null out_inf).
template <class C>
int run_normalise(int form, const uint32_t* pts, uint32_t n, uint8_t* out, uint8_t* inf) {
  const size_t rec = C::record(form);
  if (!rec || n == 0 || n > NORM_MAX_N) return -1;
  const uint32_t blocks = (n + BM_BLOCK - 1) / BM_BLOCK;
  Bufs m;
  uint32_t *stash_w, *trees, *prod, *inv, *dout, *dinf = nullptr;
  void* raw = nullptr;
  PT_TRY(hipMalloc(&raw, (size_t)BM_PIECES * BM_CHUNK * sizeof(uint4)));
  m.all.push_back(raw);
  stash_w = static_cast<uint32_t*>(raw);
  uint4* stash = reinterpret_cast<uint4*>(stash_w);
  std::vector<uint32_t> piece((size_t)4 * n);
  for (uint32_t k = 0; k < C::PIECES; k++) {
    for (uint32_t i = 0; i < n; i++)
      for (uint32_t j = 0; j < 4; j++) piece[(size_t)4 * i + j] = pts[(size_t)C::PT_WORDS * i + 4 * k + j];
    PT_TRY(hipMemcpy(stash + (size_t)k * BM_CHUNK, piece.data(), (size_t)n * sizeof(uint4), hipMemcpyHostToDevice));
  }
  PT_TRY(m.get(&trees, nullptr, (size_t)blocks * BM_TREE_WORDS));
  PT_TRY(m.get(&prod, nullptr, (size_t)blocks * 13));
  PT_TRY(m.get(&inv, nullptr, (size_t)blocks * 13));
  const size_t out_bytes = (size_t)n * rec + NORM_GUARD, inf_bytes = (size_t)n + NORM_GUARD;
  PT_TRY(m.get(&dout, nullptr, (out_bytes + 3) / 4, 0xEE));
  if (inf) PT_TRY(m.get(&dinf, nullptr, (inf_bytes + 3) / 4, 0xEE));
  hipLaunchKernelGGL(C::up, dim3(blocks), dim3(BM_THREADS), 0, 0, stash, (uint64_t)n, trees, prod);
  hipLaunchKernelGGL(C::across, dim3(1), dim3(BM_THREADS), 0, 0, (const uint32_t*)prod, blocks, inv);
  C::down(form, blocks, stash, n, trees, inv, reinterpret_cast<uint8_t*>(dout), reinterpret_cast<uint8_t*>(dinf));
  PT_TRY(finish_launch());
  PT_TRY(hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost));
  if (inf) PT_TRY(hipMemcpy(inf, dinf, inf_bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

// field 0 = Fp (13 limbs), 1 = Fq (9 limbs); op = primtest::FieldOp.  Same arguments as the host shim's shim_raw_field.
int primtest_field(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, uint32_t n) {
  if (op < 0 || op >= primtest::F_NUM_OPS) return -1;
  return field == 0 ? run_field<Fp>(op, a, b, c, d, out, n) : run_field<Fq>(op, a, b, c, d, out, n);
}
// field 0 = Te377, 1 = EdLazy; op = primtest::TeOp.  Same arguments as shim_raw_te.
int primtest_te(int field, int op, const uint32_t* p, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t* flags, uint32_t n) {
  if (op < 0 || op >= primtest::T_NUM_OPS) return -1;
  return field == 0 ? run_te<Te377>(op, p, q, neg, out, flags, n) : run_te<EdLazy>(op, p, q, neg, out, flags, n);
}
// op = primtest::G1Op.  Same arguments as shim_raw_g1.
int primtest_g1(int op, const uint32_t* a, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t n) {
  if (op < 0 || op >= primtest::G_NUM_OPS) return -1;
  Bufs m;
  uint32_t *da, *dq, *dn, *dout;
  const size_t w = (size_t)52 * n;
  PT_TRY(m.get(&da, a, w));
  PT_TRY(m.get(&dq, q, w));
  PT_TRY(m.get(&dn, neg, n));
  PT_TRY(m.get(&dout, nullptr, w));
  if (n) k_g1<<<blocks_for(n), 256>>>(op, da, dq, dn, dout, n);
  PT_TRY(finish_launch());
  return (int)fetch(out, dout, w);
}
// op = primtest::EdOp, the strict Edwards-BLS12 formulas.  Same arguments as shim_raw_ed.
int primtest_ed(int op, const uint32_t* p, const uint32_t* q, const uint32_t* neg, uint32_t* out, uint32_t n) {
  if (op < 0 || op >= primtest::E_NUM_OPS) return -1;
  Bufs m;
  uint32_t *dp, *dq, *dn, *dout;
  const size_t w = (size_t)36 * n;
  PT_TRY(m.get(&dp, p, w));
  PT_TRY(m.get(&dq, q, w));
  PT_TRY(m.get(&dn, neg, n));
  PT_TRY(m.get(&dout, nullptr, w));
  if (n) k_ed<<<blocks_for(n), 256>>>(op, dp, dq, dn, dout, n);
  PT_TRY(finish_launch());
  return (int)fetch(out, dout, w);
}
// k_bm_up / k_bm_across / k_bm_down<form> over n XYZZ points (52 raw words each) placed at the kernels' own stash indices.
// form 0 = MSM377_POINTS_WIRE (96-byte records), 1 = MSM377_POINTS_MONT_FLAG (104), 2 = BM_FORM_TABLE (128).  out: n records
// and the 256-byte guard band behind them; inf: n flag bytes and their guard band, or null for a null out_inf.
int primtest_normalise_g1(int form, const uint32_t* pts, uint32_t n, uint8_t* out, uint8_t* inf) { return run_normalise<NormG1>(form, pts, n, out, inf); }
// k_edbm_up / k_edbm_across / k_edbm_down<form> over n extended points (36 raw words).  form 0 = EDBM_FORM_WIRE (64-byte
// records), 1 = EDBM_FORM_TABLE (128).
int primtest_normalise_ed(int form, const uint32_t* pts, uint32_t n, uint8_t* out) { return run_normalise<NormEd>(form, pts, n, out, nullptr); }
int primtest_normalise_guard() { return (int)NORM_GUARD; }
// kind 0 = te_add_quad<Fp>, 1 = te_add_quad<Fq>, 2 = g1_add_quad.  a, b: n packed points (4 N limbs); out: 4 n points (one per
// lane of every quad); flags: 4 n words, is_bad of each lane's sum.
int primtest_add_quad(int kind, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flags, uint32_t n) {
  if (kind == 0) return run_add_quad<TeDev>(a, b, out, flags, n);
  if (kind == 1) return run_add_quad<EdDev>(a, b, out, flags, n);
  if (kind == 2) return run_add_quad<G1Dev>(a, b, out, flags, n);
  return -1;
}
// te_madd_quad, field 0 = Fp / G1Consts, 1 = Fq / EdConsts.  a: n Ext; b: n PBase records; out: 4 n Ext.
int primtest_madd_quad(int field, const uint32_t* a, const uint32_t* b, const uint32_t* neg, uint32_t* out, uint32_t n) {
  return field == 0 ? run_madd_quad<Te377>(a, b, neg, out, n) : run_madd_quad<EdLazy>(a, b, neg, out, n);
}
// AffWireSource::load.  raw: n x 24 wire words; out: n x 39 limbs (n1, n2, z); flags: n words.
int primtest_aff_wire(const uint32_t* raw, uint32_t* out, uint32_t* flags, uint32_t n) {
  Bufs m;
  uint32_t *draw, *dout, *df;
  PT_TRY(m.get(&draw, raw, (size_t)24 * n));
  PT_TRY(m.get(&dout, nullptr, (size_t)39 * n));
  PT_TRY(m.get(&df, nullptr, n));
  if (n) k_aff_wire<<<blocks_for(n), 256>>>(draw, dout, df, n);
  PT_TRY(finish_launch());
  PT_TRY(fetch(out, dout, (size_t)39 * n));
  return (int)fetch(flags, df, n);
}
// Bucket records of kind 0 = TeDev, 1 = EdDev, 2 = G1Dev.  in: n packed points.  rec: the n records store_record wrote into
// all-ones memory (BKT_WORDS each, pads included); out_thread: load_record of them; out_quad: load_record_quad, 4 n points;
// rec2: the records rebuilt coordinate by coordinate with store_coord, again into all-ones memory.
int primtest_records(int kind, const uint32_t* in, uint32_t* rec, uint32_t* out_thread, uint32_t* out_quad, uint32_t* rec2, uint32_t n) {
  if (kind == 0) return run_records<TeDev>(in, rec, out_thread, out_quad, rec2, n);
  if (kind == 1) return run_records<EdDev>(in, rec, out_thread, out_quad, rec2, n);
  if (kind == 2) return run_records<G1Dev>(in, rec, out_thread, out_quad, rec2, n);
  return -1;
}

}  // extern "C"
