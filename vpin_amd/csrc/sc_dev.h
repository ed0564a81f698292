// sc_dev.h -- device pieces shared by the sum-check kernels (sumcheck.hip) and the SPARK kernels
// (spark.hip): per-pair evaluation stages, the table fold, the pair bodies, block/grid reductions.
// A round kernel is: set-up, a loop over its pairs calling ONE pair body, block_sum, store or publish.
#pragma once
#include <cstring>
#include <type_traits>

#include "ctx.h"

namespace vpin {

#ifndef VPIN_SC_MIN_WAVES
#define VPIN_SC_MIN_WAVES 3  // 164 VGPRs, no scratch (4 would need 128 VGPRs and spill ~150 B)
#endif
constexpr int kBlock = 256;
constexpr int kMinWaves = VPIN_SC_MIN_WAVES;  // waves per SIMD asked of the register allocator
constexpr int kMaxBlocksCap = 16384;
inline int max_blocks() {
  static const int n = [] { const char* e = getenv("VPIN_SC_BLOCKS"); int v = e ? atoi(e) : 1024; return v < 1 ? 1 : v > kMaxBlocksCap ? kMaxBlocksCap : v; }();
  return n;
}

// Kernels written for one large workgroup (512 or 1024 threads) take their block size as a template parameter TB: the full
// size, or kSlotBlock on a context whose CUs other contexts fill with row-commitment workgroups (vpin_ctx::slot_blocks).
// Such a workgroup is placed as soon as ONE row workgroup retires: at most 256 threads, 176 VGPRs, 60 KB of LDS (DESIGN.md
// section 4).  kMinWaves caps the registers of the 256-thread forms at 168; the full forms keep the allocator's own bound.
constexpr int kSlotBlock = 256;
constexpr int tb_min_waves(int tb) { return tb <= kSlotBlock ? kMinWaves : 1; }
// f(std::integral_constant<int, TB>) with the context's TB for a kernel whose full size is FULL
template <int FULL, class F>
inline void dispatch_block(const vpin_ctx* c, F&& f) {
  if (c->slot_blocks) f(std::integral_constant<int, kSlotBlock>{});
  else f(std::integral_constant<int, FULL>{});
}

// level k (k = 1..ell) of the suffix pyramid inside one table of 2^ell elements
__host__ __device__ inline size_t pyramid_offset(int ell, int k) { return ((size_t)1 << ell) - ((size_t)2 << (ell - k)); }

// ---- per-pair evaluation -------------------------------------------------------------

template <int K>
struct Acc;

template <>
struct Acc<4> {
  static constexpr int NE = 3;
  fq e[3];
  __device__ __forceinline__ void init() { e[0] = e[1] = e[2] = fq_zero(); }
  // Phase-1 combiner (r1csproof.rs:104-108, sumcheck.rs:631-650): A * (B*C - D) at x = 0, 2, 3.  With p = the low element
  // and d = high - low of a table, the evaluation points are p (x=0), 2*high-low = p+2d (x=2), p+3d (x=3).
  // Staged form with a small live set: u[x] = B_x*C_x - D_x is built table by table, A is
  // loaded last.  Each stage takes (p,d) of ONE table; the caller loads/folds that table just
  // before the call, so at most two tables' values are live next to u[3] and e[3].
  __device__ __forceinline__ void stage_bc(fq* u, fq pb, const fq& db, fq pc, const fq& dc) {
    u[0] = fq_mul(pb, pc);
    pb = fq_add(fq_add(pb, db), db); pc = fq_add(fq_add(pc, dc), dc);
    u[1] = fq_mul(pb, pc);
    pb = fq_add(pb, db); pc = fq_add(pc, dc);
    u[2] = fq_mul(pb, pc);
  }
  __device__ __forceinline__ void stage_d(fq* u, fq pd, const fq& dd) {
    u[0] = fq_sub(u[0], pd);
    pd = fq_add(fq_add(pd, dd), dd);
    u[1] = fq_sub(u[1], pd);
    pd = fq_add(pd, dd);
    u[2] = fq_sub(u[2], pd);
  }
  // eq-factored form: the folded eq(tau,.) table is a per-round scalar times the suffix table E, so
  // A_x = c_x * E[i]; the kernel accumulates sum_i E[i]*u_x[i] and the host applies c_x
  __device__ __forceinline__ void stage_e(const fq* u, const fq& E) {
    e[0] = fq_add(e[0], fq_mul(E, u[0]));
    e[1] = fq_add(e[1], fq_mul(E, u[1]));
    e[2] = fq_add(e[2], fq_mul(E, u[2]));
  }
  // Leading-coefficient form.  With the eq factor split off, the round polynomial is l(x) * t(x) with l linear and
  // t(x) = sum_i E[i] u_x[i] quadratic, so t(0), the x^2 coefficient of t and the round's claim (which fixes t(1))
  // determine it: e[0] += E * u(0), e[1] += E * dB*dC -- two products and no p+2d / p+3d chains per pair instead
  // of three.  `first` rounds (claim not yet known to be consistent) also return e[2] += E * u(1).
  // (Without a D table the same two sums go through LeadNow or LeadAcc below.)
  __device__ __forceinline__ void lead_bcd(const fq& pb, const fq& db, const fq& pc, const fq& dc, const fq& pd, const fq& E) {
    e[0] = fq_add(e[0], fq_mul(E, fq_sub(fq_mul(pb, pc), pd)));
    e[1] = fq_add(e[1], fq_mul(E, fq_mul(db, dc)));
  }
  __device__ __forceinline__ void lead_one(const fq& pb, const fq& db, const fq& pc, const fq& dc, const fq& pd, const fq& dd,
                                           const fq& E) {
    e[2] = fq_add(e[2], fq_mul(E, fq_sub(fq_mul(fq_add(pb, db), fq_add(pc, dc)), fq_add(pd, dd))));
  }
  __device__ __forceinline__ void stage_a(const fq* u, fq pa, const fq& da) {
    e[0] = fq_add(e[0], fq_mul(pa, u[0]));
    pa = fq_add(fq_add(pa, da), da);
    e[1] = fq_add(e[1], fq_mul(pa, u[1]));
    pa = fq_add(pa, da);
    e[2] = fq_add(e[2], fq_mul(pa, u[2]));
  }
};

// The two sums of the product circuits' leading-coefficient rounds, e[0] += E * X, e[1] += E * Y with X = A_0*B_0 and
// Y = dA*dB, behind two accumulator policies with one interface (init / add / flush).  Same field values, different
// instruction mixes for different regimes:
// LeadNow: every product reduced at once (the resident tail: a pair or two per lane, latency bound).
struct LeadNow {
  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ void add(fq* e, const fq& E, const fq& X, const fq& Y) {
    e[0] = fq_add(e[0], fq_mul(E, X));
    e[1] = fq_add(e[1], fq_mul(E, Y));
  }
  __device__ __forceinline__ void flush(fq*) {}
};
// LeadAcc: the products accumulated unreduced (fq_dev.h fqw_mac), reduced every seven pairs and once at the end
// (the streaming rounds: VALU bound).
struct LeadAcc {
  fq_wide w[2];
  int n;
  __device__ __forceinline__ void init() { fqw_zero(w[0]); fqw_zero(w[1]); n = 0; }
  __device__ __forceinline__ void add(fq* e, const fq& E, const fq& X, const fq& Y) {
#ifdef VPIN_NO_LAZY_ACC  // A/B builds: every product reduced at once, as before round 4
    e[0] = fq_add(e[0], fq_mul(E, X));
    e[1] = fq_add(e[1], fq_mul(E, Y));
#else
    fqw_mac(w[0], E, X);
    fqw_mac(w[1], E, Y);
#ifndef VPIN_LAZY_NO_FLUSH  // (tools/isa_counts.py compiles the loop once without the flush to price the two apart)
    if (++n == 7) flush(e);
#endif
#endif
  }
  __device__ __forceinline__ void flush(fq* e) {
    if (n == 0) return;
    e[0] = fq_add(e[0], fqw_reduce(w[0]));
    e[1] = fq_add(e[1], fqw_reduce(w[1]));
    fqw_zero(w[0]); fqw_zero(w[1]);
    n = 0;
  }
};

template <>
struct Acc<2> {
  static constexpr int NE = 2;
  fq e[2];
  __device__ __forceinline__ void init() { e[0] = e[1] = fq_zero(); }
  // sumcheck.rs:460-469, comb A*B (r1csproof.rs:139-140) at x = 0, 2
  __device__ __forceinline__ void add_pair(fq* p, const fq* d) {
    e[0] = fq_add(e[0], fq_mul(p[0], p[1]));
#pragma unroll
    for (int k = 0; k < 2; k++) p[k] = fq_add(fq_add(p[k], d[k]), d[k]);
    e[1] = fq_add(e[1], fq_mul(p[0], p[1]));
  }
};

template <int K>
struct Tabs {
  fq* t[K];
};

// ---- (p, d) of one table's pair ----------------------------------------------------------------

// r as a fold multiplies by it: the element, or its launch-wide constant form staged in LDS (fq_dev.h fq_mul_const)
using fq_const_lds = const uint32_t (*)[8];
struct FoldR {
  fq r;
  fq_const_lds tt;
};

// Every thread of the block calls it: the first wave copies the constants of r to LDS.
__device__ __forceinline__ fq_const_lds stage_fq_const(const fq_const& rc) {
  __shared__ __attribute__((aligned(16))) uint32_t tt[8][8];
  if (threadIdx.x < 64) tt[threadIdx.x >> 3][threadIdx.x & 7] = rc.tt[threadIdx.x >> 3][threadIdx.x & 7];
  __syncthreads();
  return tt;
}

enum PdMode {
  PD_LOAD,     // the pair (i, i+n) as it is
  PD_FOLD,     // fold the table's 4n live entries with r in place, take the folded pair (i, i+n)
  PD_FOLD_C,   // the same with r in its constant form
  PD_FOLD_TO,  // fold src's entries with r into dst (dst == src: in place)
};

// fold one table's two pairs with r (dense_mlpoly.rs:232), store the folded values, return (p, d)
template <bool CONST>
__device__ __forceinline__ void fold_pair(const fq* src, fq* dst, size_t i, size_t n, const FoldR& r, fq& p, fq& d) {
  fq a0 = fq_load(src + i), a1 = fq_load(src + 2 * n + i);
  fq b0 = fq_load(src + n + i), b1 = fq_load(src + 3 * n + i);
  fq hi;
  if constexpr (CONST) {
    p = fq_add(a0, fq_mul_const(fq_sub(a1, a0), r.tt));
    hi = fq_add(b0, fq_mul_const(fq_sub(b1, b0), r.tt));
  } else {
    p = fq_add(a0, fq_mul(r.r, fq_sub(a1, a0)));
    hi = fq_add(b0, fq_mul(r.r, fq_sub(b1, b0)));
  }
  fq_store(dst + i, p);
  fq_store(dst + n + i, hi);
  d = fq_sub(hi, p);
}
// the in-place forms promise the compiler that nothing else aliases the table
template <bool CONST>
__device__ __forceinline__ void fold_pair_in_place(fq* __restrict__ t, size_t i, size_t n, const FoldR& r, fq& p, fq& d) {
  fold_pair<CONST>(t, t, i, n, r, p, d);
}
__device__ __forceinline__ void load_pair(const fq* __restrict__ t, size_t i, size_t n, fq& p, fq& d) {
  p = fq_load(t + i);
  d = fq_sub(fq_load(t + n + i), p);
}

// p = the low element and d = high - low of pair i of n, taken from the table the way m says.  PD_FOLD_TO reads src and
// writes dst, and the in-place rounds of the dot-product tables call it with dst == src: no __restrict__ on that path.
// PD_LOAD uses src alone, the in-place folds dst alone.  (The mode is a template parameter on purpose: as a function argument,
// even a constant one, it cost sc_bind_eval_kernel<4> 30 VGPRs and four spills.)
template <PdMode M>
__device__ __forceinline__ void take_pd(const fq* src, fq* dst, size_t i, size_t n, const FoldR& r, fq& p, fq& d) {
  if constexpr (M == PD_LOAD) load_pair(src, i, n, p, d);
  else if constexpr (M == PD_FOLD_TO) fold_pair<false>(src, dst, i, n, r, p, d);
  else fold_pair_in_place<M == PD_FOLD_C>(dst, i, n, r, p, d);
}
template <PdMode M>
__device__ __forceinline__ void take_pd(fq* t, size_t i, size_t n, const FoldR& r, fq& p, fq& d) {
  take_pd<M>(t, t, i, n, r, p, d);
}

// ---- pair bodies: one per combiner ---------------------------------------------------------------------------

// K tables (sumcheck.rs:624-652, 460-469): K = 4 adds A*(B*C - D), K = 2 adds A*B, at x = 0, 2(, 3)
template <int K, PdMode M>
__device__ __forceinline__ void pair_ktab(Acc<K>& acc, const Tabs<K>& tabs, size_t i, size_t n, const FoldR& r) {
  if constexpr (K == 4) {
    fq u[3], p1, d1, p2, d2;
    take_pd<M>(tabs.t[1], i, n, r, p1, d1);
    take_pd<M>(tabs.t[2], i, n, r, p2, d2);
    acc.stage_bc(u, p1, d1, p2, d2);
    take_pd<M>(tabs.t[3], i, n, r, p1, d1);
    acc.stage_d(u, p1, d1);
    take_pd<M>(tabs.t[0], i, n, r, p1, d1);
    acc.stage_a(u, p1, d1);
  } else {
    fq p[K], d[K];
#pragma unroll
    for (int k = 0; k < K; k++) take_pd<M>(tabs.t[k], i, n, r, p[k], d[k]);
    acc.add_pair(p, d);
  }
}

// Phase 1 without the eq(tau,.) table: tables (B, C, D) = (Az, Bz, Cz) and the suffix table E.  Adds E*(B_x C_x - D_x) at
// x = 0, 2, 3, or with LEAD t(0) = E*(B_0 C_0 - D_0) and the x^2 coefficient E*dB*dC, and t(1) too when nothing is
// folded (the first round).
template <PdMode M, bool LEAD>
__device__ __forceinline__ void pair_phase1(Acc<4>& acc, const Tabs<3>& tabs, const fq* __restrict__ E, size_t i, size_t n,
                                            const FoldR& r) {
  fq p1, d1, p2, d2;
  take_pd<M>(tabs.t[0], i, n, r, p1, d1);
  take_pd<M>(tabs.t[1], i, n, r, p2, d2);
  if constexpr (LEAD) {
    fq p3, d3;
    take_pd<M>(tabs.t[2], i, n, r, p3, d3);
    const fq e = fq_load(E + i);
    acc.lead_bcd(p1, d1, p2, d2, p3, e);
    if constexpr (M == PD_LOAD) acc.lead_one(p1, d1, p2, d2, p3, d3, e);
  } else {
    fq u[3];
    acc.stage_bc(u, p1, d1, p2, d2);
    take_pd<M>(tabs.t[2], i, n, r, p1, d1);
    acc.stage_d(u, p1, d1);
    acc.stage_e(u, fq_load(E + i));
  }
}

// Product circuit (tables A, B and the suffix table E): adds E*A_x*B_x at x = 0, 2, 3, or with LEAD t(0) = E*A_0*B_0 and
// the x^2 coefficient E*dA*dB through the accumulator policy `lead` (LeadNow or LeadAcc; the caller flushes it).
template <PdMode M, bool LEAD, class Lead>
__device__ __forceinline__ void pair_prod(Acc<4>& acc, Lead& lead, fq* A, fq* B, const fq* __restrict__ E, size_t i, size_t n,
                                          const FoldR& r) {
  fq p1, d1, p2, d2;
  take_pd<M>(A, i, n, r, p1, d1);
  take_pd<M>(B, i, n, r, p2, d2);
  if constexpr (LEAD) {
    lead.add(acc.e, fq_load(E + i), fq_mul(p1, p2), fq_mul(d1, d2));
  } else {
    fq u[3];
    acc.stage_bc(u, p1, d1, p2, d2);
    acc.stage_e(u, fq_load(E + i));
  }
}

// Dot-product circuit (three tables): adds L_x*R_x*W_x at x = 0, 2, 3; BIND folds src[t] into dst[t] first
template <bool BIND>
__device__ __forceinline__ void pair_dotp(Acc<4>& acc, const fq* const* src, fq* const* dst, size_t i, size_t n, const FoldR& r) {
  constexpr PdMode M = BIND ? PD_FOLD_TO : PD_LOAD;
  fq u[3], p1, d1, p2, d2;
  take_pd<M>(src[0], dst[0], i, n, r, p1, d1);
  take_pd<M>(src[1], dst[1], i, n, r, p2, d2);
  acc.stage_bc(u, p1, d1, p2, d2);
  take_pd<M>(src[2], dst[2], i, n, r, p1, d1);
  acc.stage_a(u, p1, d1);
}

// ---- reductions ----------------------------------------------------------------------------------------------

// Sum of e[k] over the first nw waves of a block of THREADS threads, returned in thread k < NE (zero elsewhere).
// Every thread of the block calls it, whatever nw is: both barriers are outside the conditions.  The trailing barrier
// frees the LDS rows for a second call in the same kernel.
template <int NE, int THREADS>
__device__ __forceinline__ fq block_sum(const fq* e, int nw = THREADS / 64) {
  __shared__ fq sh[THREADS / 64][NE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < nw) {
#pragma unroll
    for (int k = 0; k < NE; k++) {
      fq s = fq_wave_sum(e[k]);
      if (lane == 0) sh[wave][k] = s;
    }
  }
  __syncthreads();
  fq s = fq_zero();
  if (threadIdx.x < NE) {
    s = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < nw; w++) s = fq_add(s, sh[w][threadIdx.x]);
  }
  __syncthreads();
  return s;
}

// e[k] = sum of partial k over rows first, first + step, .. below nblocks of rows[nblocks][NE]
template <int NE>
__device__ __forceinline__ void sum_partial_rows(const fq* rows,int nblocks, int first, int step, fq* e) {
#pragma unroll
  for (int k = 0; k < NE; k++) e[k] = fq_zero();
  for (int b = first; b < nblocks; b += step)
#pragma unroll
    for (int k = 0; k < NE; k++) e[k] = fq_add(e[k], fq_load(&rows[(size_t)b * NE + k]));
}

// block-level reduction of NE accumulators; thread k < NE of the block writes partial k of row blockIdx.x
template <int NE>
__device__ __forceinline__ void block_reduce_store(const fq* e, fq* __restrict__ partials) {
  const fq s = block_sum<NE, kBlock>(e);
  if (threadIdx.x < NE) fq_store(&partials[(size_t)blockIdx.x * NE + threadIdx.x], s);
}

// Workgroup y sums instance y's nblocks x NE block partials into out[NE * y ..].
template <int NE>
__global__ __launch_bounds__(kBlock) void sc_finish_kernel(const fq* __restrict__ partials, int nblocks,
                                                           fq* __restrict__ out) {
  fq e[NE];
  sum_partial_rows<NE>(partials + (size_t)blockIdx.x * nblocks * NE, nblocks, threadIdx.x, kBlock, e);
  const fq s = block_sum<NE, kBlock>(e);
  if (threadIdx.x < NE) fq_store(&out[NE * (size_t)blockIdx.x + threadIdx.x], s);
}

// f(std::bool_constant...) with the run-time bools as template arguments: dispatch_bools([&](auto B, auto L) {
// launch kernel<decltype(B)::value, decltype(L)::value> }, bind, lead)
template <class F>
inline void dispatch_bools(F&& f) { f(); }
template <class F, class... Bools>
inline void dispatch_bools(F&& f, bool b, Bools... rest) {
  if (b) dispatch_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else dispatch_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

static inline int grid_for(size_t work) {
  size_t b = (work + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > (size_t)max_blocks()) b = max_blocks();
  return (int)b;
}

// T_i = r~ * 2^(32 i) * 2^-256 mod q for the Montgomery image r~ in `p` (host arithmetic, once per launch), transposed
fq_const make_fq_const(const uint8_t* p);

static inline fq load_host_fq(const uint8_t* p) {
  fq r;
  memcpy(r.v, p, 32);
  return r;
}

}  // namespace vpin
