// Input validation (msm377_*_check_points*): is every wire point canonical, on its curve, in the prime-order subgroup?
// Nothing in the reference corresponds to this: its shaders assume valid input.
//   k_check_curve     a thread per point: coordinates below the modulus, then the curve equation; counts the two classes
//                     and appends the points that passed to a compact index list for the subgroup pass
//   k_check_subgroup  a thread per listed point: acc = [order]P along ONE fixed signed-digit chain (consts_gen.hpp
//                     CheckConsts, written by tools/gen_consts.py) that every lane walks in step; P is in the subgroup
//                     iff the chain ends in the identity
// G1 runs in Weierstrass XYZZ form (g1_xyzz.hpp): the chain of a point of order 2, 3, 4 or 6 passes through the identity,
// through P = -acc and through doublings of 2-torsion points (Y = 0), where those formulas leave their general case in a
// way that one compare detects (G1Check); the twisted Edwards form of G1 (te377.hpp) has exceptional pairs exactly there.  Edwards-BLS12's law is complete on the curve
// (ed_ext.hpp), and the cascade guarantees that the subgroup kernel only sees curve points.
// The report is deterministic: counters are sums, and the first failing point is the minimum of (index << 2 | class)
// under a 64-bit atomicMin, not the lane that got there first.
// Device code; included by sequencer.hip only.
#pragma once
#include "../curves.hpp"

namespace msm377 {
namespace {

// Scratch words of one check call (the front of ctx->d_work_meta, which every MSM clears for itself).
constexpr uint32_t CHK_NONCANON = 0, CHK_OFFCURVE = 1, CHK_OUTSIDE = 2, CHK_LIST_COUNT = 3, CHK_FIRST = 4;  // CHK_FIRST: a u64, words 4-5
constexpr uint32_t CHK_WORDS = 8;
constexpr uint32_t CHK_CLASS_NONCANON = 1, CHK_CLASS_OFFCURVE = 2, CHK_CLASS_OUTSIDE = 3;  // low bits of the first-bad key
constexpr uint32_t CHK_THREADS = 256;

__global__ void __launch_bounds__(64) k_check_clear(uint32_t* __restrict__ scratch) {
  if (threadIdx.x < CHK_WORDS) scratch[threadIdx.x] = (threadIdx.x == CHK_FIRST || threadIdx.x == CHK_FIRST + 1) ? 0xffffffffu : 0u;
}

// x (limbs of a wire coordinate, each below 2^29) >= the modulus?
template <class F>
__device__ __forceinline__ bool limbs_geq_mod(const typename F::El& x) {
  int32_t bw = 0;
#pragma unroll
  for (int j = 0; j < F::N; j++) bw = ((int32_t)x.l[j] - (int32_t)F::Consts::MOD[j] + bw) >> 31;
  return bw == 0;  // no borrow out of x - modulus
}

// What the two kernels need from a curve beyond the pipeline's policy (curves.hpp): the wire checks and the chain.
struct G1Check {
  using CV = G1Dev;
  static constexpr int NAF_LEN = CheckConsts::G1_NAF_LEN;
  static __device__ __forceinline__ uint32_t naf_pos(int w) { return CheckConsts::G1_NAF_POS[w]; }
  static __device__ __forceinline__ uint32_t naf_neg(int w) { return CheckConsts::G1_NAF_NEG[w]; }
  // A 48-byte coordinate holds 384 bits, the 13 limbs 377: the seven bits above them are part of the comparison.
  static __device__ __forceinline__ bool canonical(const uint32_t* w) {
    const bool high = ((w[11] | w[23]) >> 25) != 0;
    return !high && !limbs_geq_mod<Fp>(Fp::from_words<12>(w)) && !limbs_geq_mod<Fp>(Fp::from_words<12>(w + 12));
  }
  // y^2 = x^3 + 1 on the RAW coordinates (a raw value v is the Montgomery form of v / R): x^2 / R, y^2 / R, then
  // (x^2 / R) x + (y^2 / R) (p - 1) in one reduction = (x^3 - y^2) / R^2, which is -1 / R^2 on the curve.  Two squarings
  // and one double product, no conversion.  Bounds (field29.hpp): canonical inputs; the squares are lazy products below
  // p + 2^354 in N-form; the double product takes N-form x canonical twice, 26 a b terms and 12 q p terms of < 2^58 in a
  // column; its value is below p + 2^354, which canon() takes to [0, p).
  static __device__ __forceinline__ bool on_curve(const uint32_t* w) {
    const Fp::El x = Fp::from_words<12>(w), y = Fp::from_words<12>(w + 12);
    Fp::El m1 = Fp::from_const(G1Consts::MOD);
    m1.l[0] -= 1u;  // p - 1 (p = 1 mod 2^29)
    const Fp::El d = Fp::mul_add_mul_lz(Fp::sqr_lz(x), x, Fp::sqr_lz(y), m1);
    return Fp::eq(Fp::canon(d), Fp::from_const(G1Consts::CHK_RHS_RAW));
  }
  using Base = G1Affine;
  using Acc = G1XYZZ;
  static __device__ __forceinline__ Base load(const uint32_t* w) {
    Base p;
    p.x = Fp::to_mont(Fp::from_words<12>(w));
    p.y = Fp::to_mont(Fp::from_words<12>(w + 12));
    return p;
  }
  // The chain in Weierstrass XYZZ form, WITHOUT case distinctions -- by this argument.  Walking the digits of r from the
  // top, the accumulator before a step is [m]P with 0 < m < r, and so is every value m +- 1 an addition compares against.
  // The formulas of g1_xyzz.hpp leave their general case exactly when the group does something special:
  //   dbl   ZZ3 = 0          <=>  [2m]P = O (the input was O already, or a 2-torsion point, Y = 0)
  //   madd  P = 0 (mod p)    <=>  [m]P = +-P, i.e. [m -+ 1]P = O
  // Before the LAST addition each of these says [j]P = O for some 0 < j < r.  r is prime and P is not O (the wire format
  // cannot encode it), so P then has an order that is not r: the point is outside the subgroup, whatever the rest of the
  // chain would compute.  The events are therefore recorded in a sticky flag (`small`) instead of being followed through;
  // what the formulas compute afterwards is discarded (their bounds are bounds on magnitudes and hold for any residues,
  // so nothing overflows on the way).  The last addition is [r -+ 1]P +- P: the point is in the subgroup iff that
  // addition is the "opposite points" case (P = 0 and R != 0 mod p) and nothing was recorded before.  Points of order
  // 2, 3, 4, 6 set the flag in the first steps; P + T (P in the subgroup, T of small order) walks the general case to the
  // end and arrives at [r]T != O.  The host implementation (validate_host.hpp) follows every case through instead; the
  // tests compare the two.
  struct Walk {
    bool small = false;   // [j]P = O met for some 0 < j < r
    bool closed = false;  // the last addition produced O
  };
  static __device__ __forceinline__ Acc start(const Base& q) { return G1::from_affine(q); }
  // G1::dbl (dbl-2008-s-1, canonical forms, canon_pt on entry) without its early return
  static __device__ __forceinline__ Acc dbl(const Acc& a, Walk& wk) {
    const Acc p = G1::canon_pt(a);
    const Fp::El u = Fp::dbl(p.y), v = Fp::sqr(u), w = Fp::mul(u, v), s = Fp::mul(p.x, v), xx = Fp::sqr(p.x);
    const Fp::El m = Fp::add(Fp::dbl(xx), xx);
    Acc r;
    r.x = Fp::sub(Fp::sqr(m), Fp::dbl(s));
    r.y = Fp::mul_sub_mul(m, Fp::sub(s, r.x), w, p.y);
    r.zz = Fp::mul(v, p.zz);
    r.zzz = Fp::mul(w, p.zzz);
    wk.small |= Fp::is_zero(r.zz);  // canonical: an exact test
    return r;
  }
  // G1::madd_lz (madd-2008-s in the lazy forms; same lines, same bounds) with its cases recorded, not followed.
  static __device__ __forceinline__ Acc madd(const Acc& a, const Base& q, bool negq, bool last, Walk& wk) {
    using K = G1Consts;
    const Fp::El u2 = Fp::mul_lz(q.x, a.zz);
    const Fp::El s2 = Fp::mul_lz(Fp::select(negq, Fp::kp_sub(K::KP2, q.y), q.y), a.zzz);
    const Fp::El p = Fp::norm(Fp::add_kp_sub(u2, K::KP6, a.x));
    const Fp::El r = Fp::norm(Fp::add_kp_sub(s2, K::KP2, a.y));
    if ((p.l[0] - 1u) < 7u) {  // P = 0 mod p means P in {p, .., 7p}, low limb 1..7: one compare guards the exact test
      if (Fp::is_zero(Fp::canon(p))) {
        if (last) wk.closed = !Fp::is_zero(Fp::canon(r));
        else wk.small = true;
      }
    }
    const Fp::El pp = Fp::sqr_lz(p);
    const Fp::El ppp = Fp::mul_lz(p, pp);
    const Fp::El qq = Fp::mul_lz(a.x, pp);
    Acc o;
    o.x = Fp::norm(Fp::add_kp_sub_sub2(Fp::sqr_lz(r), K::KP4W3, ppp, qq));
    const Fp::El d = Fp::norm(Fp::add_kp_sub(qq, K::KP6, o.x));
    o.y = Fp::mul_add_mul_lz(r, d, Fp::kp_sub(K::KP2, a.y), ppp);
    o.zz = Fp::mul_lz(a.zz, pp);
    o.zzz = Fp::mul_lz(a.zzz, ppp);
    return o;
  }
  static __device__ __forceinline__ bool in_subgroup(const Acc&, const Walk& wk) { return wk.closed && !wk.small; }
};

struct EdCheck {
  using CV = EdDev;
  static constexpr int NAF_LEN = CheckConsts::ED_NAF_LEN;
  static __device__ __forceinline__ uint32_t naf_pos(int w) { return CheckConsts::ED_NAF_POS[w]; }
  static __device__ __forceinline__ uint32_t naf_neg(int w) { return CheckConsts::ED_NAF_NEG[w]; }
  static __device__ __forceinline__ bool canonical(const uint32_t* w) {  // 9 limbs hold all 256 bits
    return !limbs_geq_mod<Fq>(Fq::from_words<8>(w)) && !limbs_geq_mod<Fq>(Fq::from_words<8>(w + 8));
  }
  // -x^2 + y^2 = 1 + d x^2 y^2 in the canonical forms of the 9-limb field
  static __device__ __forceinline__ bool on_curve(const uint32_t* w) {
    const Fq::El x = Fq::to_mont(Fq::from_words<8>(w)), y = Fq::to_mont(Fq::from_words<8>(w + 8));
    const Fq::El xx = Fq::sqr(x), yy = Fq::sqr(y);
    const Fq::El rhs = Fq::add(Fq::one(), Fq::mul(Fq::mul(xx, yy), Fq::from_const(EdConsts::ED_D)));
    return Fq::eq(Fq::sub(yy, xx), rhs);
  }
  using Base = Ed::Base;
  using Acc = Ed::Ext;
  static __device__ __forceinline__ Base load(const uint32_t* w) {
    return Ed::make_base(Fq::to_mont(Fq::from_words<8>(w)), Fq::to_mont(Fq::from_words<8>(w + 8)));
  }
  // The law is complete on the curve (a = -1 a square, d a non-square): no events to record, the chain is followed to
  // its end and the result compared with the identity (0 : c : 0 : c).
  struct Walk {};
  static __device__ __forceinline__ Acc start(const Base& q) { return Ed::madd(Ed::identity(), q); }
  static __device__ __forceinline__ Acc dbl(const Acc& a, Walk&) { return Ed::dbl(a); }
  static __device__ __forceinline__ Acc madd(const Acc& a, const Base& q, bool negq, bool, Walk&) { return Ed::madd(a, Ed::cneg(q, negq)); }
  static __device__ __forceinline__ bool in_subgroup(const Acc& a, const Walk&) { return Fq::is_zero(a.x) && Fq::eq(a.y, a.z); }
};

static_assert((CheckConsts::G1_NAF_POS[0] | CheckConsts::G1_NAF_NEG[0]) & 1u, "the chain ends with an addition (odd order)");
static_assert((CheckConsts::ED_NAF_POS[0] | CheckConsts::ED_NAF_NEG[0]) & 1u, "the chain ends with an addition (odd order)");
static_assert((CheckConsts::G1_NAF_POS[(CheckConsts::G1_NAF_LEN - 1) >> 5] >> ((CheckConsts::G1_NAF_LEN - 1) & 31)) & 1u, "top digit +1");
static_assert((CheckConsts::ED_NAF_POS[(CheckConsts::ED_NAF_LEN - 1) >> 5] >> ((CheckConsts::ED_NAF_LEN - 1) & 31)) & 1u, "top digit +1");

// Adds a wave's findings to the workgroup's LDS counters: ONE global atomic per class and workgroup afterwards (the
// hot-counter lesson of k_work_hist), and one 64-bit atomicMin for the lowest failing index.  Lanes of a wave hold
// consecutive (k_check_curve) or arbitrary (k_check_subgroup) indices, so the minimum is taken over keys, not lanes.
struct CheckTally {
  uint32_t count[3];
  unsigned long long first;
};
__device__ __forceinline__ void tally_init(CheckTally& t) {
  if (threadIdx.x < 3) t.count[threadIdx.x] = 0;
  if (threadIdx.x == 3) t.first = ~0ull;
  __syncthreads();
}
__device__ __forceinline__ void tally_wave(CheckTally& t, bool bad, uint32_t cls, uint64_t index) {
  const unsigned long long m = __ballot(bad);
  if (m == 0) return;  // wave-uniform
  if (bad && (m & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0) atomicAdd(&t.count[cls - 1], (uint32_t)__popcll(m));  // its first lane
  if (bad) atomicMin(&t.first, (unsigned long long)((index << 2) | cls));  // LDS; only waves that hold a bad point get here
}
__device__ __forceinline__ void tally_flush(CheckTally& t, uint32_t* __restrict__ scratch) {
  __syncthreads();
  if (threadIdx.x < 3 && t.count[threadIdx.x]) atomicAdd(&scratch[CHK_NONCANON + threadIdx.x], t.count[threadIdx.x]);
  if (threadIdx.x == 3 && t.first != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(scratch + CHK_FIRST), t.first);
}

// want_curve = 0: the canonical test alone.  list != nullptr: the subgroup pass follows.
template <class CK>
__global__ void __launch_bounds__(CHK_THREADS) k_check_curve(const uint32_t* __restrict__ raw, uint64_t n, uint32_t want_curve, uint32_t* __restrict__ scratch,
                                                             uint32_t* __restrict__ list) {
  using CV = typename CK::CV;
  __shared__ CheckTally tally;
  tally_init(tally);
  const uint64_t i = (uint64_t)blockIdx.x * CHK_THREADS + threadIdx.x;
  const bool live = i < n;
  bool noncanon = false, offcurve = false;
  if (live) {
    uint32_t w[CV::RAW_WORDS];
    load_words16(raw + i * CV::RAW_WORDS, w, CV::RAW_WORDS / 4);
    noncanon = !CK::canonical(w);
    if (!noncanon && want_curve) offcurve = !CK::on_curve(w);
  }
  tally_wave(tally, noncanon, CHK_CLASS_NONCANON, i);
  tally_wave(tally, offcurve, CHK_CLASS_OFFCURVE, i);
  if (list) {  // kernel-uniform
    const bool pass = live && !noncanon && !offcurve;
    const unsigned long long m = __ballot(pass);
    if (m) {
      const uint32_t lane = threadIdx.x & 63;
      const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&scratch[CHK_LIST_COUNT], (uint32_t)__popcll(m));  // one atomic per wave
      base = __shfl(base, (int)leader);
      if (pass) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
  }
  tally_flush(tally, scratch);
}

// 4 x 13 accumulator limbs, 2 x 13 of the point and the temporaries of dbl / madd_lz live in registers: two workgroups
// per CU like k_accumulate.  The digit of a step is a kernel-uniform scalar and the steps have no per-lane control flow
// beyond the rare exact test behind madd's one-compare guard (G1Check).
template <class CK>
__global__ void __launch_bounds__(CHK_THREADS, 2) k_check_subgroup(const uint32_t* __restrict__ raw, uint32_t* __restrict__ scratch, const uint32_t* __restrict__ list) {
  using CV = typename CK::CV;
  __shared__ CheckTally tally;
  const uint32_t count = scratch[CHK_LIST_COUNT];  // complete: k_check_curve is the previous launch on this stream
  const uint32_t t = blockIdx.x * CHK_THREADS + threadIdx.x;
  if ((uint32_t)(blockIdx.x * CHK_THREADS) >= count) return;  // workgroup-uniform: a wave is never held by points that failed
  tally_init(tally);
  const bool live = t < count;
  const uint32_t idx = live ? list[t] : list[0];  // idle lanes of the last workgroup walk the chain of a listed point
  uint32_t w[CV::RAW_WORDS];
  load_words16(raw + (size_t)idx * CV::RAW_WORDS, w, CV::RAW_WORDS / 4);
  const typename CK::Base p = CK::load(w);
  typename CK::Acc acc = CK::start(p);  // the top digit is +1
  typename CK::Walk wk;
#pragma unroll 1
  for (int k = CK::NAF_LEN - 2; k >= 0; k--) {
    acc = CK::dbl(acc, wk);
    const uint32_t bit = 1u << (k & 31);
    const bool pos = (CK::naf_pos(k >> 5) & bit) != 0, neg = (CK::naf_neg(k >> 5) & bit) != 0;
    if (pos || neg) acc = CK::madd(acc, p, neg, k == 0, wk);  // kernel-uniform; digit 0 is not zero (the orders are odd)
  }
  tally_wave(tally, live && !CK::in_subgroup(acc, wk), CHK_CLASS_OUTSIDE, idx);
  tally_flush(tally, scratch);
}

}  // namespace
}  // namespace msm377
