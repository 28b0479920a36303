// Fixed-base batch multiplication on Edwards-BLS12 (msm377_ed_batch_mul_multi*): out[i] = sum_{j<k} [s_ij]B_j for k <= 16
// fixed bases and n rows of scalars, every output its own 64-byte wire point (account addresses [sk_i]G, Pedersen-style
// commitments [m_i]G + [r_i]H, Schnorr nonces, ElGamal halves).  The structure is that of kernels/batch_mul_multi.hpp --
// window tables, the signed recode of batch_mul_recode.hpp, a thread per output, Montgomery's trick over a pass -- on the
// complete addition law of ed_ext.hpp: no identity / equal / opposite cases, no infinity flags, the identity an ordinary
// record (y - x, y + x, 2dxy) = (1, 1, 0).
//
//   k_edbm_row_bases   workgroup b, thread w: [2^(c w)]B_b by c w doublings, for every base a build is missing
//   k_edbm_entries     thread (b, w, d) over the concatenated records of the missing tables: [d] of row base w by
//                      double-and-add
//   k_edbm_accumulate  THE HOT KERNEL: a thread per output walks table 0 with s_i0, table 1 with s_i1, .. into ONE lazy
//                      accumulator (EdLazy::madd_affine on signed operands: the operand pattern of the bucket accumulation,
//                      which tools/check_lazy_bounds.py replays)
//   k_edbm_up / k_edbm_across / k_edbm_down   Montgomery's trick across the Z's of a pass: running products per thread and a
//                      product tree per workgroup, ONE inversion per pass on one lane (fq_inverse.hpp), the trees walked
//                      down, x = X / Z and y = Y / Z written as wire records or as table records
// The two table kernels use the canonical Ed:: formulas (they run once per build) and leave extended points in the stash
// the hot kernel writes; the same three launches normalise them into table records.  The build itself is the one table
// builder of the batch calls (sequencer.hip build_mul_tables) under this curve's policy, the slots the one slot type.  The completeness of the law on the
// curve is what keeps every Z non-zero: the host verifies the bases (EdHostCheck) before anything is launched.
// Stash, trees and block products are the G1 batch calls' (ctx->bm): 9 point pieces and 3 running-product pieces of their
// 17, 9-limb nodes in their 13-limb trees.  Device code; included by sequencer.hip only, after kernels/batch_mul_multi.hpp.
#pragma once
#include "../fq_inverse.hpp"
#include "batch_mul_multi.hpp"

namespace msm377 {
namespace {

// Stash: pieces 0..8: X, Y, T, Z (36 words, canonical, written by the hot kernel and the table kernels); pieces 9..11:
// the exclusive running product of the thread's Z's (9 words + 3 pad, k_edbm_up).
constexpr uint32_t EDBM_POINT_PIECES = 9, EDBM_PIECES = 12;
static_assert(EDBM_PIECES <= BM_PIECES, "the stash is the G1 calls'");
constexpr uint32_t EDBM_TREE_WORDS = 2 * BM_THREADS * 9;  // one workgroup's product tree in HBM
static_assert(EDBM_TREE_WORDS <= BM_TREE_WORDS, "the trees are the G1 calls'");
// Table record: (y - x)[9] (y + x)[9] (2dxy)[9] pad[5] = 128 bytes, canonical device Montgomery limbs: EdDev's base record
// (MSM377_BASES_ED), one cache line per gather.
constexpr uint32_t EDBM_FORM_WIRE = 0, EDBM_FORM_TABLE = 1;

struct EdbmTables {  // as BmmTables: a scalar load at a run-time offset of the argument segment
  const uint32_t* t[MSM377_MUL_MAX_BASES];
};

__device__ __forceinline__ void put9(uint32_t* w, const Fq::El& e) {
#pragma unroll
  for (int j = 0; j < 9; j++) w[j] = e.l[j];
}
__device__ __forceinline__ Fq::El get9(const uint32_t* w) {
  Fq::El e;
#pragma unroll
  for (int j = 0; j < 9; j++) e.l[j] = w[j];
  return e;
}
// Canonical coordinates in: the normalisation runs the canonical products on them.
__device__ __forceinline__ void edbm_store_point(uint4* __restrict__ stash, uint64_t i, const Fq::El& x, const Fq::El& y, const Fq::El& t, const Fq::El& z) {
  uint32_t w[36];
  put9(w, x);
  put9(w + 9, y);
  put9(w + 18, t);
  put9(w + 27, z);
#pragma unroll
  for (uint32_t k = 0; k < EDBM_POINT_PIECES; k++) stash[(size_t)k * BM_CHUNK + i] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
__device__ __forceinline__ Ed::Base edbm_load_record(const uint32_t* __restrict__ table, uint64_t idx) {
  uint32_t w[28];
  load_words16(table + idx * BM_REC_WORDS, w, 7);
  Ed::Base q;
  q.ymx = get9(w);
  q.ypx = get9(w + 9);
  q.kt = get9(w + 18);
  return q;
}

// ---- table build, every missing slot at once ----
// bases_wire: 64 bytes per missing base; row base w of base b goes to stash index b (W + 1) + w.
__global__ void __launch_bounds__(64) k_edbm_row_bases(const uint32_t* __restrict__ bases_wire, uint32_t c, uint4* __restrict__ stash) {
  const uint32_t w = threadIdx.x, W = (uint32_t)bm_windows((int)c), b = blockIdx.x;
  if (w > W) return;
  uint32_t raw[16];
  load_words16(bases_wire + (size_t)b * 16, raw, 4);
  Ed::Ext acc;
  acc.x = Fq::to_mont(Fq::from_words<8>(raw));
  acc.y = Fq::to_mont(Fq::from_words<8>(raw + 8));
  acc.t = Fq::mul(acc.x, acc.y);
  acc.z = Fq::one();
#pragma unroll 1
  for (uint32_t k = 0; k < c * w; k++) acc = Ed::dbl(acc);
  edbm_store_point(stash, (uint64_t)b * (W + 1) + w, acc.x, acc.y, acc.t, acc.z);
}

// Record g = first + u of the concatenation, u < count <= BM_CHUNK: table b = g / records, entry t = g mod records of it,
// from the row bases of base b; the point goes to stash index u.
__global__ void __launch_bounds__(BM_THREADS) k_edbm_entries(const uint32_t* __restrict__ row_bases, uint32_t c, uint64_t first, uint64_t count, uint4* __restrict__ stash) {
  const uint64_t u = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  if (u >= count) return;
  const uint64_t records = bm_table_records(c), g = first + u;
  const uint32_t b = (uint32_t)(g / records), W = (uint32_t)bm_windows((int)c);
  const uint64_t t = g - (uint64_t)b * records;
  const uint32_t w = (uint32_t)(t >> (c - 1)), d = ((uint32_t)t & ((1u << (c - 1)) - 1u)) + 1u;
  const Ed::Base q = edbm_load_record(row_bases, (uint64_t)b * (W + 1) + w);
  Ed::Ext acc = Ed::identity();
#pragma unroll 1
  for (int bit = 31 - __clz((int)d); bit >= 0; bit--) {
    acc = Ed::dbl(acc);
    if ((d >> bit) & 1u) acc = Ed::madd(acc, q);
  }
  edbm_store_point(stash, u, acc.x, acc.y, acc.t, acc.z);
}

// ---- the hot kernel ----
// k_bmm_accumulate's walk on the lazy Edwards law: a 4 x 9-limb accumulator and the 3 x 9 limbs of a record, seven
// products per addition.  s_ij is the 32 bytes at scalars + i out_stride + j base_stride, read as an integer and not
// reduced; a zero digit sits out, a window in which the whole wave holds zero digits is skipped.  The accumulator starts as
// the identity and takes EdLazy::madd_affine(acc, record, sign) only: EdDev::first / EdDev::madd of k_accumulate.  The
// coordinates leave the kernel canonical (Fq::canon: any N-form value below 8 q).
// Code object (profiles/ed_batch_mul/device_code.txt): no scratch, no spill.
__global__ void __launch_bounds__(BM_THREADS, 4) k_edbm_accumulate(const EdbmTables tables, const uint8_t* __restrict__ scalars, uint64_t n, uint32_t k, uint64_t out_stride,
                                                                   uint64_t base_stride, uint32_t c, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < n;
  const uint32_t W = (uint32_t)bm_windows((int)c), half = 1u << (c - 1);
  EdLazy::Ext acc = EdLazy::identity();
#pragma unroll 1
  for (uint32_t j = 0; j < k; j++) {
    uint32_t s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = 0;  // an idle lane walks the zero scalar: no digit, no load
    if (live) load_words16(reinterpret_cast<const uint32_t*>(scalars + i * out_stride + (uint64_t)j * base_stride), s, 2);
    const uint32_t* __restrict__ table = tables.t[j];
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t w = 0; w <= W; w++) {
      // As in k_bmm_accumulate: the scalar moves down by c bits per step, bm_digit always reads window 0.  Row W: the carry.
      const int32_t d = w < W ? bm_digit(s, (int)c, 0, carry) : (int32_t)carry;
#pragma unroll
      for (int q = 0; q < 7; q++) s[q] = (s[q] >> c) | (s[q + 1] << (32 - c));  // c <= 16
      s[7] >>= c;
      const bool act = d != 0;
      if (__ballot(act) == 0) continue;  // wave-uniform
      const uint32_t mag = act ? (uint32_t)(d < 0 ? -d : d) : 1u;
      const EdLazy::ABase q = EdDev::load_base(table, (uint32_t)((uint64_t)w * half + (mag - 1u)));
      if (act) acc = EdLazy::madd_affine(acc, q, d < 0);
    }
  }
  if (live) edbm_store_point(stash, i, Fq::canon(acc.x), Fq::canon(acc.y), Fq::canon(acc.t), Fq::canon(acc.z));
}

// ---- normalisation ----
// Up-sweep: thread tid of workgroup blk owns outputs blk * BM_BLOCK + j * BM_THREADS + tid, j < BM_K.  Every Z is non-zero.
__global__ void __launch_bounds__(BM_THREADS, 2) k_edbm_up(uint4* __restrict__ stash, uint64_t n, uint32_t* __restrict__ trees, uint32_t* __restrict__ block_prod) {
  __shared__ uint32_t tree[2 * BM_THREADS][9];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x;
  const uint64_t base = (uint64_t)blk * BM_BLOCK + tid;
  Fq::El c = Fq::one();
#pragma unroll 1
  for (uint32_t j = 0; j < BM_K; j++) {
    const uint64_t i = base + (uint64_t)j * BM_THREADS;
    if (i >= n) break;
    uint32_t w[12];
    bm_load_pieces<6, 3>(stash, i, w);  // words 24..35 of the point: Z is words 27..35
    const Fq::El z = get9(w + 3);
    stash[(size_t)9 * BM_CHUNK + i] = make_uint4(c.l[0], c.l[1], c.l[2], c.l[3]);
    stash[(size_t)10 * BM_CHUNK + i] = make_uint4(c.l[4], c.l[5], c.l[6], c.l[7]);
    stash[(size_t)11 * BM_CHUNK + i] = make_uint4(c.l[8], 0u, 0u, 0u);
    c = Fq::mul(c, z);
  }
  put9(tree[BM_THREADS + tid], c);
  for (uint32_t size = BM_THREADS / 2; size >= 1; size >>= 1) {
    __syncthreads();
    if (tid < size) put9(tree[size + tid], Fq::mul(get9(tree[2 * (size + tid)]), get9(tree[2 * (size + tid) + 1])));
  }
  __syncthreads();
  uint32_t* out = trees + (size_t)blk * EDBM_TREE_WORDS;
  const uint32_t* flat = &tree[0][0];
  for (uint32_t k = tid; k < EDBM_TREE_WORDS; k += BM_THREADS) out[k] = flat[k];
  if (tid < 9) block_prod[(size_t)blk * 9 + tid] = tree[1][tid];
}

// One workgroup: the pass's workgroup products (at most BM_BLOCK of them) -> their inverses, by the same trick one level
// up; ONE inversion on one lane.  MSM377_EDBM_FERMAT (a build switch of the measurement in profiles/ed_batch_mul only)
// runs the 253-squaring chain in its place.
__global__ void __launch_bounds__(BM_THREADS) k_edbm_across(const uint32_t* __restrict__ block_prod, uint32_t blocks, uint32_t* __restrict__ block_inv) {
  __shared__ uint32_t tree[2 * BM_THREADS][9];
  const uint32_t tid = threadIdx.x;
  Fq::El c = Fq::one();
#pragma unroll 1
  for (uint32_t j = 0; j < BM_K; j++) {
    const uint32_t b = tid * BM_K + j;
    if (b >= blocks) break;
    put9(block_inv + (size_t)b * 9, c);
    c = Fq::mul(c, get9(block_prod + (size_t)b * 9));
  }
  put9(tree[BM_THREADS + tid], c);
  for (uint32_t size = BM_THREADS / 2; size >= 1; size >>= 1) {
    __syncthreads();
    if (tid < size) put9(tree[size + tid], Fq::mul(get9(tree[2 * (size + tid)]), get9(tree[2 * (size + tid) + 1])));
  }
  __syncthreads();
  if (tid == 0) {  // every factor is non-zero mod q: the root has an inverse
#if defined(MSM377_EDBM_FERMAT)
    put9(tree[1], fe_pow<Fq, EdConsts::PM2_NW>(get9(tree[1]), EdConsts::PM2_W));
#else
    put9(tree[1], FqInverse::inverse_mont(get9(tree[1])));
#endif
  }
  for (uint32_t size = 1; size < BM_THREADS; size <<= 1) {
    __syncthreads();
    if (tid < size) {
      const uint32_t k = size + tid;
      const Fq::El inv_k = get9(tree[k]), a = get9(tree[2 * k]), b = get9(tree[2 * k + 1]);
      put9(tree[2 * k], Fq::mul(inv_k, b));
      put9(tree[2 * k + 1], Fq::mul(inv_k, a));
    }
  }
  __syncthreads();
  Fq::El inv = get9(tree[BM_THREADS + tid]);
#pragma unroll 1
  for (int j = (int)BM_K - 1; j >= 0; j--) {
    const uint32_t b = tid * BM_K + (uint32_t)j;
    if (b >= blocks) continue;
    const Fq::El cj = get9(block_inv + (size_t)b * 9);
    put9(block_inv + (size_t)b * 9, Fq::mul(inv, cj));  // 1 / product_b = (1 / C_(b+1)) C_b
    inv = Fq::mul(inv, get9(block_prod + (size_t)b * 9));
  }
}

// Down-sweep: x = X / Z, y = Y / Z, then
//   EDBM_FORM_WIRE    canonical residues, 64-byte records x || y; the identity comes out as (0, 1) by itself
//   EDBM_FORM_TABLE   (y - x, y + x, 2dxy) in canonical Montgomery limbs and 5 zero words: 128-byte table records
template <uint32_t FORM>
__global__ void __launch_bounds__(BM_THREADS, 2) k_edbm_down(const uint4* __restrict__ stash, uint64_t n, const uint32_t* __restrict__ trees, const uint32_t* __restrict__ block_inv,
                                                             uint8_t* __restrict__ out) {
  __shared__ uint32_t tree[2 * BM_THREADS][9];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x;
  const uint32_t* in = trees + (size_t)blk * EDBM_TREE_WORDS;
  uint32_t* flat = &tree[0][0];
  for (uint32_t k = tid; k < EDBM_TREE_WORDS; k += BM_THREADS) flat[k] = in[k];
  __syncthreads();
  if (tid < 9) tree[1][tid] = block_inv[(size_t)blk * 9 + tid];
  for (uint32_t size = 1; size < BM_THREADS; size <<= 1) {
    __syncthreads();
    if (tid < size) {
      const uint32_t k = size + tid;
      const Fq::El inv_k = get9(tree[k]), a = get9(tree[2 * k]), b = get9(tree[2 * k + 1]);
      put9(tree[2 * k], Fq::mul(inv_k, b));
      put9(tree[2 * k + 1], Fq::mul(inv_k, a));
    }
  }
  __syncthreads();
  Fq::El inv = get9(tree[BM_THREADS + tid]);  // 1 / (the product of this thread's Z's)
  const uint64_t base = (uint64_t)blk * BM_BLOCK + tid;
#pragma unroll 1
  for (int j = (int)BM_K - 1; j >= 0; j--) {
    const uint64_t i = base + (uint64_t)j * BM_THREADS;
    if (i >= n) continue;
    uint32_t w[4 * EDBM_PIECES];
    bm_load_pieces<0, EDBM_PIECES>(stash, i, w);
    const Fq::El zi = Fq::mul(inv, get9(w + 36));  // 1 / Z_j = (1 / C_(j+1)) C_j
    inv = Fq::mul(inv, get9(w + 27));              // 1 / C_j
    const Fq::El x = Fq::mul(get9(w), zi), y = Fq::mul(get9(w + 9), zi);
    if constexpr (FORM == EDBM_FORM_TABLE) {
      const Ed::Base b = Ed::make_base(x, y);
      uint32_t o[BM_REC_WORDS];
#pragma unroll
      for (uint32_t k = 27; k < BM_REC_WORDS; k++) o[k] = 0;
      put9(o, b.ymx);
      put9(o + 9, b.ypx);
      put9(o + 18, b.kt);
      uint4* dst = reinterpret_cast<uint4*>(out + i * (BM_REC_WORDS * 4));
#pragma unroll
      for (uint32_t k = 0; k < BM_REC_WORDS / 4; k++) dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
      uint32_t o[16];
      Fq::to_words<8>(Fq::from_mont(x), o);
      Fq::to_words<8>(Fq::from_mont(y), o + 8);
      uint4* dst = reinterpret_cast<uint4*>(out + i * 64);
#pragma unroll
      for (int k = 0; k < 4; k++) dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    }
  }
}

}  // namespace
}  // namespace msm377
