// Fixed-base batch multiplication (msm377_g1_batch_mul*): out[i] = [s_i]B for ONE base B and n scalars, every output
// its own affine point.  Nothing in the reference corresponds to this (it computes sums only); the counterpart in the
// prover stacks is arkworks' FixedBase::msm / batch_mul.
//
//   (the table)      row w, w = 0 .. W (W = ceil(256 / c); row W is the carry's entry), holds [d 2^(c w)]B, d = 1 .. 2^(c-1);
//                    built by the one table builder of the batch calls (sequencer.hip build_mul_tables) with the build
//                    kernels of kernels/batch_mul_multi.hpp, for one base
//   k_bm_accumulate  THE HOT KERNEL: a thread per output walks the signed digits of its scalar (batch_mul_recode.hpp) from
//                    the low end and adds one table record per non-zero digit
//   k_bm_up / k_bm_across / k_bm_down   Montgomery's trick across the outputs of a chunk, entirely on the device: running
//                    products per thread and a product tree per workgroup on the way up, ONE inversion per chunk in a
//                    single-workgroup launch (a binary Euclid walk on one lane, fp_inverse.hpp), the trees walked down
//                    and the affine records written on the way down
// The build kernels leave XYZZ points in the same stash the hot kernel writes, and the same three launches normalise
// them into table records: the table is built with the machinery it serves.  Grid-wide dependencies are launch
// boundaries on one stream; no kernel waits for another workgroup.
//
// Every curve point is a legal base (orders 2, 3, 4, 6, points outside the prime-order subgroup), so the additions keep
// the identity / equal / opposite cases of g1_xyzz.hpp and follow them through -- k_check_subgroup's shortcut of
// recording such events and discarding the result does not apply where every output is wanted:
//   * acc = O before the first non-zero digit, and again whenever the partial sum is a multiple of the base's order;
//   * acc = +-entry: [m]B = [d 2^(c w)]B with m != d 2^(c w) happens for a base of small order and is then common
//     (order 3: every third step);
//   * a table entry may itself be O ([4]B for a base of order 4: whole rows).  Its record carries a flag word and the
//     addition is skipped like a zero digit.
// Device code; included by sequencer.hip only.
#pragma once
#include "../batch_mul_recode.hpp"
#include "../curves.hpp"
#include "../fp_inverse.hpp"
#include "convert.hpp"

namespace msm377 {
namespace {

constexpr uint32_t BM_THREADS = 256;
constexpr uint32_t BM_K = 4;                               // outputs per thread of the normalisation
constexpr uint32_t BM_BLOCK = BM_THREADS * BM_K;           // outputs per workgroup product tree
constexpr uint64_t BM_CHUNK = 1ull << 20;                  // outputs per pass: the stash, the trees and ONE inversion
constexpr uint32_t BM_CHUNK_BLOCKS = (uint32_t)(BM_CHUNK / BM_BLOCK);
static_assert(BM_CHUNK_BLOCKS <= BM_BLOCK, "k_bm_across folds a chunk's workgroup products in one workgroup");
// Stash: 16-byte piece k of chunk-local output i at piece index k * BM_CHUNK + i, so that every load and store of a wave
// is 1 KB of contiguous memory (the lesson of k_affine_up's stash).  Pieces 0..12: X, Y, ZZ, ZZZ (52 words, written by
// the hot kernel); pieces 13..16: the exclusive running product C of the thread's ZZZ's (13 words + 3 pad, k_bm_up).
constexpr uint32_t BM_POINT_PIECES = 13, BM_PIECES = 17;
constexpr uint32_t BM_TREE_WORDS = 2 * BM_THREADS * 13;    // one workgroup's product tree in HBM
// Table record: x[13] y[13] flag[1] pad[5] = 128 bytes, one cache line per gather; canonical device Montgomery limbs.
// flag != 0: the entry is the identity (x = y = 0, which is not on y^2 = x^3 + 1 either).
constexpr uint32_t BM_REC_WORDS = 32, BM_REC_FLAG = 26;
constexpr uint32_t BM_FORM_TABLE = 0x100;                  // k_bm_down's third output form, beside MSM377_POINTS_WIRE / _MONT_FLAG
constexpr uint64_t bm_table_records(uint32_t c) { return (uint64_t)bm_windows((int)c) * (1ull << (c - 1)) + 1; }
static_assert(bm_table_records(16) <= BM_CHUNK && bm_table_records(8) <= BM_CHUNK, "a table is normalised in one chunk");

__device__ __forceinline__ void bm_store_point(uint4* __restrict__ stash, uint64_t i, const G1XYZZ& p) {
  uint32_t w[52];
  G1Dev::to_words(p, w);
#pragma unroll
  for (uint32_t k = 0; k < BM_POINT_PIECES; k++) stash[(size_t)k * BM_CHUNK + i] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
template <uint32_t FIRST, uint32_t COUNT>
__device__ __forceinline__ void bm_load_pieces(const uint4* __restrict__ stash, uint64_t i, uint32_t* w) {
#pragma unroll
  for (uint32_t k = 0; k < COUNT; k++) {
    const uint4 v = stash[(size_t)(FIRST + k) * BM_CHUNK + i];
    w[4 * k + 0] = v.x;
    w[4 * k + 1] = v.y;
    w[4 * k + 2] = v.z;
    w[4 * k + 3] = v.w;
  }
}
// A table record; false: the entry is the identity.
__device__ __forceinline__ bool bm_load_record(const uint32_t* __restrict__ table, uint64_t idx, G1Affine& q) {
  uint32_t w[28];
  load_words16(table + idx * BM_REC_WORDS, w, 7);
#pragma unroll
  for (int j = 0; j < 13; j++) {
    q.x.l[j] = w[j];
    q.y.l[j] = w[13 + j];
  }
  return w[BM_REC_FLAG] == 0;
}
// The identity of the stash: ZZ = ZZZ = 0 limb by limb, whatever the formulas left in X and Y (a doubled 2-torsion point
// has ZZ = 0 beside arbitrary X, Y).  The normalisation tests ZZZ alone.
__device__ __forceinline__ G1XYZZ bm_tidy(const G1XYZZ& p) {
  G1XYZZ r = p;
  if (G1::is_identity(p)) r = G1::identity();
  return r;
}

// ---- table build ----
// k_bmm_row_bases and k_bmm_entries (kernels/batch_mul_multi.hpp): the one table of this call is a build of one base.

// ---- the hot kernel ----
// 4 x 13 accumulator limbs, the 2 x 13 of a record and madd's temporaries in registers, two workgroups per CU: the
// budget of k_check_subgroup.  A window in which every lane of the wave holds a zero digit is skipped (short scalars:
// most of them); inside a window the lanes with a zero digit or an identity entry sit the addition out.  Code object:
// 205 VGPRs, no register spill; 100 bytes of scratch per lane hold 25 accumulator limbs across madd's four exits (a dozen
// 4-byte stores per step beside ~4 400 instructions) -- the scalar is not in it.
__global__ void __launch_bounds__(BM_THREADS, 2) k_bm_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint64_t n, uint32_t c,
                                                                 uint32_t scalars_mont, uint4* __restrict__ stash) {
  const uint64_t i = (uint64_t)blockIdx.x * BM_THREADS + threadIdx.x;
  const bool live = i < n;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = 0;  // an idle lane walks the zero scalar: no digit, no load
  if (live) {
    load_words16(scalars + i * 8, s, 2);
    if (scalars_mont) {  // v -> v 2^-256 mod r, fully reduced: the product of kernels/import.hpp
      const Fq::El v = Fq::mul(Fq::from_words<8>(s), Fq::from_const(EdConsts::IMPORT_MONT256));
      Fq::to_words<8>(v, s);
    }
  }
  const uint32_t W = (uint32_t)bm_windows((int)c), half = 1u << (c - 1);
  G1XYZZ acc = G1::identity();
  uint32_t carry = 0;
#pragma unroll 1
  for (uint32_t w = 0; w <= W; w++) {
    // Window w sits in the low bits: the scalar moves down by c bits per step, so bm_digit always reads window 0 and no
    // register array is indexed by a run-time value.  Row W: the final carry.
    const int32_t d = w < W ? bm_digit(s, (int)c, 0, carry) : (int32_t)carry;
#pragma unroll
    for (int k = 0; k < 7; k++) s[k] = (s[k] >> c) | (s[k + 1] << (32 - c));  // c <= 16
    s[7] >>= c;
    bool act = d != 0;
    if (__ballot(act) == 0) continue;  // wave-uniform
    const uint32_t mag = act ? (uint32_t)(d < 0 ? -d : d) : 1u;
    G1Affine q;
    act = bm_load_record(table, (uint64_t)w * half + (mag - 1u), q) && act;
    if (act) acc = G1::madd(acc, q, d < 0);
  }
  if (live) bm_store_point(stash, i, bm_tidy(acc));
}

// ---- normalisation ----
// Up-sweep: thread tid of workgroup blk owns outputs blk * BM_BLOCK + j * BM_THREADS + tid, j < BM_K.  An identity
// output contributes 1 to every product (never 0: it would wipe the block) and is recognised again on the way down.
__global__ void __launch_bounds__(BM_THREADS, 2) k_bm_up(uint4* __restrict__ stash, uint64_t n, uint32_t* __restrict__ trees, uint32_t* __restrict__ block_prod) {
  __shared__ uint32_t tree[2 * BM_THREADS][13];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x;
  const uint64_t base = (uint64_t)blk * BM_BLOCK + tid;
  Fp::El c = Fp::one();
#pragma unroll 1
  for (uint32_t j = 0; j < BM_K; j++) {
    const uint64_t i = base + (uint64_t)j * BM_THREADS;
    if (i >= n) break;
    uint32_t w[16];
    bm_load_pieces<9, 4>(stash, i, w);  // words 36..51 of the point: ZZZ is words 39..51
    Fp::El z = get13(w + 3);
    if (Fp::is_zero(z)) z = Fp::one();
    stash[(size_t)13 * BM_CHUNK + i] = make_uint4(c.l[0], c.l[1], c.l[2], c.l[3]);
    stash[(size_t)14 * BM_CHUNK + i] = make_uint4(c.l[4], c.l[5], c.l[6], c.l[7]);
    stash[(size_t)15 * BM_CHUNK + i] = make_uint4(c.l[8], c.l[9], c.l[10], c.l[11]);
    stash[(size_t)16 * BM_CHUNK + i] = make_uint4(c.l[12], 0u, 0u, 0u);
    c = Fp::mul_lz(c, z);  // both below p + 2^354
  }
  put13(tree[BM_THREADS + tid], c);
  for (uint32_t size = BM_THREADS / 2; size >= 1; size >>= 1) {
    __syncthreads();
    if (tid < size) put13(tree[size + tid], Fp::mul_lz(get13(tree[2 * (size + tid)]), get13(tree[2 * (size + tid) + 1])));
  }
  __syncthreads();
  uint32_t* out = trees + (size_t)blk * BM_TREE_WORDS;
  const uint32_t* flat = &tree[0][0];
  for (uint32_t k = tid; k < BM_TREE_WORDS; k += BM_THREADS) out[k] = flat[k];
  if (tid < 13) block_prod[(size_t)blk * 13 + tid] = tree[1][tid];
}

// One workgroup: the chunk's workgroup products (at most BM_BLOCK of them) -> their inverses, by the same trick one
// level up -- running products per thread, a tree, ONE inversion on one lane (fp_inverse.hpp: per chunk, not per
// workgroup), the tree down, the products unfolded.  block_inv holds the running products on the way up.
__global__ void __launch_bounds__(BM_THREADS) k_bm_across(const uint32_t* __restrict__ block_prod, uint32_t blocks, uint32_t* __restrict__ block_inv) {
  __shared__ uint32_t tree[2 * BM_THREADS][13];
  const uint32_t tid = threadIdx.x;
  Fp::El c = Fp::one();
#pragma unroll 1
  for (uint32_t j = 0; j < BM_K; j++) {
    const uint32_t b = tid * BM_K + j;
    if (b >= blocks) break;
    put13(block_inv + (size_t)b * 13, c);
    c = Fp::mul_lz(c, get13(block_prod + (size_t)b * 13));
  }
  put13(tree[BM_THREADS + tid], c);
  for (uint32_t size = BM_THREADS / 2; size >= 1; size >>= 1) {
    __syncthreads();
    if (tid < size) put13(tree[size + tid], Fp::mul_lz(get13(tree[2 * (size + tid)]), get13(tree[2 * (size + tid) + 1])));
  }
  __syncthreads();
  if (tid == 0) put13(tree[1], FpInverse::inverse_mont(get13(tree[1])));  // every factor is non-zero mod p: the root has an inverse
  for (uint32_t size = 1; size < BM_THREADS; size <<= 1) {
    __syncthreads();
    if (tid < size) {
      const uint32_t k = size + tid;
      const Fp::El inv_k = get13(tree[k]), a = get13(tree[2 * k]), b = get13(tree[2 * k + 1]);
      put13(tree[2 * k], Fp::mul_lz(inv_k, b));
      put13(tree[2 * k + 1], Fp::mul_lz(inv_k, a));
    }
  }
  __syncthreads();
  Fp::El inv = get13(tree[BM_THREADS + tid]);
#pragma unroll 1
  for (int j = (int)BM_K - 1; j >= 0; j--) {
    const uint32_t b = tid * BM_K + (uint32_t)j;
    if (b >= blocks) continue;
    const Fp::El cj = get13(block_inv + (size_t)b * 13);
    put13(block_inv + (size_t)b * 13, Fp::mul_lz(inv, cj));  // 1 / product_b = (1 / C_(b+1)) C_b
    inv = Fp::mul_lz(inv, get13(block_prod + (size_t)b * 13));
  }
}

// Down-sweep: x = X (ZZ / ZZZ)^2, y = Y / ZZZ, then ONE more product per coordinate into the requested form:
//   MSM377_POINTS_WIRE       canonical residues (a product with the raw 1), 96-byte records, the identity as x = 0, y = 1
//   MSM377_POINTS_MONT_FLAG  2^384-Montgomery residues (a product with TO64), 104-byte records, flag byte 1 for the identity
//                            beside the coordinates msm377_g1_result_to_native gives the wire identity
//   BM_FORM_TABLE            the 2^406-Montgomery limbs themselves, reduced once: 128-byte table records
// out_inf (may be null): one byte per output, 1 for the identity.
template <uint32_t FORM>
__global__ void __launch_bounds__(BM_THREADS, 2) k_bm_down(const uint4* __restrict__ stash, uint64_t n, const uint32_t* __restrict__ trees, const uint32_t* __restrict__ block_inv,
                                                           uint8_t* __restrict__ out, uint8_t* __restrict__ out_inf) {
  __shared__ uint32_t tree[2 * BM_THREADS][13];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x;
  const uint32_t* in = trees + (size_t)blk * BM_TREE_WORDS;
  uint32_t* flat = &tree[0][0];
  for (uint32_t k = tid; k < BM_TREE_WORDS; k += BM_THREADS) flat[k] = in[k];
  __syncthreads();
  if (tid < 13) tree[1][tid] = block_inv[(size_t)blk * 13 + tid];
  for (uint32_t size = 1; size < BM_THREADS; size <<= 1) {
    __syncthreads();
    if (tid < size) {
      const uint32_t k = size + tid;
      const Fp::El inv_k = get13(tree[k]), a = get13(tree[2 * k]), b = get13(tree[2 * k + 1]);
      put13(tree[2 * k], Fp::mul_lz(inv_k, b));
      put13(tree[2 * k + 1], Fp::mul_lz(inv_k, a));
    }
  }
  __syncthreads();
  Fp::El inv = get13(tree[BM_THREADS + tid]);  // 1 / (the product of this thread's ZZZ's)
  const uint64_t base = (uint64_t)blk * BM_BLOCK + tid;
#pragma unroll 1
  for (int j = (int)BM_K - 1; j >= 0; j--) {
    const uint64_t i = base + (uint64_t)j * BM_THREADS;
    if (i >= n) continue;
    uint32_t w[4 * BM_PIECES];
    bm_load_pieces<0, BM_PIECES>(stash, i, w);
    const G1XYZZ p = G1Dev::from_words(w);
    const bool ident = Fp::is_zero(p.zzz);
    Fp::El x = Fp::zero(), y = Fp::one();
    if (!ident) {  // (an identity took no part in the products: inv stays)
      const Fp::El zi = Fp::mul_lz(inv, get13(w + 52));  // 1 / ZZZ_j = (1 / C_(j+1)) C_j
      inv = Fp::mul_lz(inv, p.zzz);                       // 1 / C_j
      const Fp::El tt = Fp::mul_lz(zi, p.zz);             // ZZ / ZZZ = 1 / sqrt(ZZ)
      x = Fp::mul_lz(p.x, Fp::sqr_lz(tt));                // X: N-form below 5p + 2^354, the square below p + 2^354
      y = Fp::mul_lz(p.y, zi);
    }
    if constexpr (FORM == BM_FORM_TABLE) {
      uint32_t o[BM_REC_WORDS];
#pragma unroll
      for (uint32_t k = 0; k < BM_REC_WORDS; k++) o[k] = 0;
      if (ident) {
        o[BM_REC_FLAG] = 1;
      } else {
        put13(o, Fp::reduce_once(x));
        put13(o + 13, Fp::reduce_once(y));
      }
      uint4* dst = reinterpret_cast<uint4*>(out + i * (BM_REC_WORDS * 4));
#pragma unroll
      for (uint32_t k = 0; k < BM_REC_WORDS / 4; k++) dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
      Fp::El f = Fp::zero();
      if constexpr (FORM == MSM377_POINTS_WIRE) f.l[0] = 1;
      else f = Fp::from_const(G1Consts::TO64);
      uint32_t o[26];
      Fp::to_words<12>(Fp::mul(x, f), o);
      Fp::to_words<12>(Fp::mul(y, f), o + 12);
      if constexpr (FORM == MSM377_POINTS_WIRE) {
        uint4* dst = reinterpret_cast<uint4*>(out + i * 96);
#pragma unroll
        for (int k = 0; k < 6; k++) dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
      } else {
        o[24] = ident ? 1u : 0u;  // flag byte, then seven zero bytes
        o[25] = 0;
        uint2* dst = reinterpret_cast<uint2*>(out + i * 104);  // a record is 8-byte aligned only
#pragma unroll
        for (int k = 0; k < 13; k++) dst[k] = make_uint2(o[2 * k], o[2 * k + 1]);
      }
    }
    if (out_inf) out_inf[i] = ident ? 1 : 0;
  }
}

}  // namespace
}  // namespace msm377
