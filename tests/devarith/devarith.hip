// devarith.hip -- test-only harness: every device function of fq_dev.h, fp_dev.h, fp10_dev.h, e2_dev.h, the helpers of
// ge_tree_dev.h and the shared sum-check pieces of sc_dev.h (block_sum, take_pd, the pair bodies) behind one __global__
// kernel and one extern "C" launcher each, so that tests/test_gpu_dev_*.py can hand them
// chosen LIMB PATTERNS (not only chosen values) and compare with plain integer arithmetic (tests/limb_vectors.py).
//
// Conventions: inputs and outputs are flat arrays of raw 32-bit words, IW words in and OW words out per case; one case per
// lane (one per workgroup for the wave and block functions); the tail of the last workgroup is masked.  A launcher allocates,
// copies, launches, synchronises and returns HIP's error code (0 = hipSuccess); it never aborts.
//
// KNOWN LIMIT.  The harness checks the arithmetic as written in the headers and compiled at -O3 into THIS library.  It does
// not check the copy that the compiler inlined into each product kernel.
//
// Built by vpin_amd.build.build_devtest() into vpin_amd/lib/libvpin_devtest.so: a library of its own, no part of
// libvpin_hip.so and of include/vpin_hip.h.  Its one reference to the product is the host function make_fq_const
// (sumcheck.hip), which dv_fq_mul_const_host checks against fq_mul.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "e2_dev.h"
#include "fp10_dev.h"
#include "fp_dev.h"
#include "fq_dev.h"
#include "ge_tree_dev.h"
#include "sc_dev.h"

using namespace vpin;

namespace {

struct DvBuf {
  void* p = nullptr;
  ~DvBuf() {
    if (p) (void)hipFree(p);
  }
};

template <class Kernel>
int dv_run(Kernel kernel, const uint32_t* in, size_t iw, uint32_t* out, size_t ow, int n, int block, int grid) {
  if (n <= 0) return 0;
  DvBuf din, dout;
  hipError_t e;
  if ((e = hipMalloc(&din.p, iw * n * 4)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&dout.p, ow * n * 4)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(din.p, in, iw * n * 4, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemset(dout.p, 0xa5, ow * n * 4)) != hipSuccess) return (int)e;
  kernel<<<dim3((unsigned)grid), dim3(block), 0, 0>>>((const uint32_t*)din.p, (uint32_t*)dout.p, n);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(out, dout.p, ow * n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  return 0;
}

template <class T>
__device__ __forceinline__ T ld8(const uint32_t* p) {
  T r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = p[i];
  return r;
}
template <class T>
__device__ __forceinline__ void st8(uint32_t* p, const T& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
__device__ __forceinline__ fe10 ld10(const uint32_t* p) {
  fe10 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void st10(uint32_t* p, const fe10& a) {
#pragma unroll
  for (int i = 0; i < 10; i++) p[i] = a.v[i];
}
__device__ __forceinline__ ge_ext ld_ext(const uint32_t* p) {
  ge_ext r;
  r.X = ld8<fp>(p); r.Y = ld8<fp>(p + 8); r.Z = ld8<fp>(p + 16); r.T = ld8<fp>(p + 24);
  return r;
}
__device__ __forceinline__ void st_ext(uint32_t* p, const ge_ext& a) {
  st8(p, a.X); st8(p + 8, a.Y); st8(p + 16, a.Z); st8(p + 24, a.T);
}
__device__ __forceinline__ ge_niels ld_niels(const uint32_t* p) {
  ge_niels r;
  r.ypx = ld8<fp>(p); r.ymx = ld8<fp>(p + 8); r.xy2d = ld8<fp>(p + 16);
  return r;
}
__device__ __forceinline__ ge_cached ld_cached(const uint32_t* p) {
  ge_cached r;
  r.YpX = ld8<fp>(p); r.YmX = ld8<fp>(p + 8); r.Z = ld8<fp>(p + 16); r.T2d = ld8<fp>(p + 24);
  return r;
}
__device__ __forceinline__ e2_jac ld_jac(const uint32_t* p) {
  e2_jac r;
  r.X = ld8<fq>(p); r.Y = ld8<fq>(p + 8); r.Z = ld8<fq>(p + 16);
  return r;
}
__device__ __forceinline__ void st_jac(uint32_t* p, const e2_jac& a) {
  st8(p, a.X); st8(p + 8, a.Y); st8(p + 16, a.Z);
}

}  // namespace

// one case per lane: ci / co are the case's IW input and OW output words
#define DV_LANE(name, IW, OW, BLOCK, ...)                                                                             \
  __global__ __launch_bounds__(BLOCK) void k_##name(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) { \
    const int i = blockIdx.x * (BLOCK) + threadIdx.x;                                                                 \
    if (i >= n) return;                                                                                               \
    const uint32_t* ci = in + (size_t)i * (IW);                                                                       \
    uint32_t* co = out + (size_t)i * (OW);                                                                            \
    __VA_ARGS__                                                                                                       \
  }                                                                                                                   \
  extern "C" int dv_##name(const uint32_t* in, uint32_t* out, int n) {                                                \
    return dv_run(k_##name, in, IW, out, OW, n, BLOCK, (n + (BLOCK)-1) / (BLOCK));                                    \
  }

// one case per workgroup of BLOCK lanes: ci / co are the case's IW input and OW output words, every lane runs the body
#define DV_BLOCK(name, IW, OW, BLOCK, ...)                                                                            \
  __global__ __launch_bounds__(BLOCK) void k_##name(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) { \
    const uint32_t* ci = in + (size_t)blockIdx.x * (IW);                                                              \
    uint32_t* co = out + (size_t)blockIdx.x * (OW);                                                                   \
    const int tid = threadIdx.x;                                                                                      \
    (void)tid;                                                                                                        \
    __VA_ARGS__                                                                                                       \
  }                                                                                                                   \
  extern "C" int dv_##name(const uint32_t* in, uint32_t* out, int n) { return dv_run(k_##name, in, IW, out, OW, n, BLOCK, n); }

// ---- fq_dev.h -----------------------------------------------------------------------------------------------------------
DV_LANE(fq_add, 16, 8, 256, st8(co, fq_add(ld8<fq>(ci), ld8<fq>(ci + 8)));)
DV_LANE(fq_sub, 16, 8, 256, st8(co, fq_sub(ld8<fq>(ci), ld8<fq>(ci + 8)));)
DV_LANE(fq_neg, 8, 8, 256, st8(co, fq_neg(ld8<fq>(ci)));)
DV_LANE(fq_dbl, 8, 8, 256, st8(co, fq_dbl(ld8<fq>(ci)));)
DV_LANE(fq_mul, 16, 8, 256, st8(co, fq_mul(ld8<fq>(ci), ld8<fq>(ci + 8)));)
DV_LANE(fq_sqr, 8, 8, 256, st8(co, fq_sqr(ld8<fq>(ci)));)
DV_LANE(fq_from_mont, 8, 8, 256, st8(co, fq_from_mont(ld8<fq>(ci)));)
DV_LANE(fq_cond_sub_q, 8, 8, 256, st8(co, fq_cond_sub_q(ld8<fq>(ci)));)

// in: count (1..7), then seven (a, b) pairs; out: fqw_reduce of the sum, then the sixteen words of the sum itself
DV_LANE(fqw_mac_reduce, 113, 24, 64,
        fq_wide w; fqw_zero(w);
        const int cnt = (int)ci[0];
        for (int k = 0; k < cnt && k < 7; k++) fqw_mac(w, ld8<fq>(ci + 1 + 16 * k), ld8<fq>(ci + 9 + 16 * k));
        st8(co, fqw_reduce(w));
        for (int k = 0; k < 16; k++) co[8 + k] = w.v[k];)

// in: d, then the eight constants T_0..T_7 as they are (arbitrary canonical values); the kernel transposes them
DV_LANE(fq_mul_const, 72, 8, 64,
        alignas(16) uint32_t tt[8][8];
        for (int t = 0; t < 8; t++)
          for (int k = 0; k < 8; k++) tt[k][t] = ci[8 + 8 * t + k];
        st8(co, fq_mul_const(ld8<fq>(ci), tt));)

// in: n values d, then, in the same buffer, the 64 words of the host's make_fq_const(r); one workgroup of 64 lanes stages them
__global__ __launch_bounds__(64) void k_fq_mul_const_host(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
  __shared__ alignas(16) uint32_t tt[8][8];
  tt[threadIdx.x >> 3][threadIdx.x & 7] = in[(size_t)8 * n + threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  st8(out + (size_t)8 * i, fq_mul_const(ld8<fq>(in + (size_t)8 * i), tt));
}
// r32: the challenge in Montgomery form, 32 bytes; in: n values d of eight words; out: n products
extern "C" int dv_fq_mul_const_host(const uint8_t* r32, const uint32_t* in, uint32_t* out, int n) {
  if (n <= 0) return 0;
  const fq_const c = make_fq_const(r32);
  DvBuf din, dout;
  hipError_t e;
  const size_t bytes = (size_t)n * 32;
  if ((e = hipMalloc(&din.p, bytes + sizeof(c))) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&dout.p, bytes)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy((uint8_t*)din.p + bytes, &c, sizeof(c), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemset(dout.p, 0xa5, bytes)) != hipSuccess) return (int)e;
  k_fq_mul_const_host<<<dim3((n + 63) / 64), dim3(64), 0, 0>>>((const uint32_t*)din.p, (uint32_t*)dout.p, n);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  return 0;
}

// one wave per case: in 64 elements, out the 64 lanes' totals
DV_BLOCK(fq_wave_sum, 512, 512, 64, st8(co + 8 * tid, fq_wave_sum(ld8<fq>(ci + 8 * tid)));)

// ---- sc_dev.h: block_sum, take_pd, the pair bodies ------------------------------------------------------------------------
// in: nw, then two sets of THREADS x NE elements (set, thread, k); out: the NE sums of the first set, then of the second.
// Two calls in a row, as finish_block makes them; nw = THREADS / 64 goes through the default argument.
template <int NE, int THREADS>
__device__ __forceinline__ void block_sum_case(const uint32_t* ci, uint32_t* co, int tid) {
  const int nw = (int)ci[0];
  fq e[NE], f[NE];
  for (int k = 0; k < NE; k++) {
    e[k] = ld8<fq>(ci + 1 + 8 * (NE * tid + k));
    f[k] = ld8<fq>(ci + 1 + 8 * NE * THREADS + 8 * (NE * tid + k));
  }
  const bool all = nw == THREADS / 64;  // uniform over the workgroup
  const fq s = all ? block_sum<NE, THREADS>(e) : block_sum<NE, THREADS>(e, nw);
  const fq t = all ? block_sum<NE, THREADS>(f) : block_sum<NE, THREADS>(f, nw);
  if (tid < NE) { st8(co + 8 * tid, s); st8(co + 8 * (NE + tid), t); }
}
DV_BLOCK(block_sum_2_256, 1 + 16 * 2 * 256, 32, 256, block_sum_case<2, 256>(ci, co, tid);)
DV_BLOCK(block_sum_3_256, 1 + 16 * 3 * 256, 48, 256, block_sum_case<3, 256>(ci, co, tid);)
DV_BLOCK(block_sum_2_512, 1 + 16 * 2 * 512, 32, 512, block_sum_case<2, 512>(ci, co, tid);)
DV_BLOCK(block_sum_3_512, 1 + 16 * 3 * 512, 48, 512, block_sum_case<3, 512>(ci, co, tid);)

// One table of 4 q entries (q <= 64), lane i < q takes pair i.  in: mode (PdMode; 4 = PD_FOLD_TO with dst == src), q, 2 unused
// words, r, the 64 words of r's constant form (tt[k][i], staged through stage_fq_const), 256 entries.  out: the table
// afterwards (256 entries), the destination of mode 3 (128 entries), then (p, d) of the 64 lanes.
DV_BLOCK(take_pd, 4 + 8 + 64 + 2048, 2048 + 1024 + 1024, 64,
         const int mode = (int)ci[0];
         const size_t q = ci[1];
         fq_const rc;
         for (int k = 0; k < 64; k++) rc.tt[k >> 3][k & 7] = ci[12 + k];
         const FoldR fr{ld8<fq>(ci + 4), stage_fq_const(rc)};
         fq* tab = reinterpret_cast<fq*>(co);
         fq* dst = tab + 256;
         for (size_t e = tid; e < 4 * q; e += 64) fq_store(tab + e, ld8<fq>(ci + 76 + 8 * e));
         __syncthreads();
         fq p = fq_zero(); fq d = fq_zero();
         if ((size_t)tid < q) {
           if (mode == 0) take_pd<PD_LOAD>(tab, tid, q, fr, p, d);
           else if (mode == 1) take_pd<PD_FOLD>(tab, tid, q, fr, p, d);
           else if (mode == 2) take_pd<PD_FOLD_C>(tab, tid, q, fr, p, d);
           else take_pd<PD_FOLD_TO>(tab, mode == 3 ? dst : tab, tid, q, fr, p, d);
         }
         st8(co + 3072 + 16 * tid, p); st8(co + 3072 + 16 * tid + 8, d);)

// np <= 15 pairs through one pair body on one lane, one lane kernel per fold mode M.  in: body, 1 unused word, np, 1 unused
// word, r, r's constant form (tt[k][i]), E[15], four tables of 60 entries (4 np used, pair i of np).  out: e[0..2] (e[2] unused
// by the K = 2 body), one unused row, the four tables afterwards, the dot-product body's three destination tables of 30 entries.
// body: 0 / 1 pair_ktab with K = 2 / 4; 2 / 3 pair_phase1 without / with LEAD; 4 pair_prod without LEAD; 5 / 6 pair_prod
// with LEAD through LeadNow / LeadAcc; 7 pair_dotp (BIND when the mode is not PD_LOAD).
// Everything is inlined into the kernel on purpose.  A body of this size left as a function of its own (a lambda called per
// mode) needs long branches, and the compiler builds those in s[30:31], the function's return address: it never returns.
template <PdMode M>
__device__ __forceinline__ void sc_body_case(const uint32_t* ci, uint32_t* co) {
  const int body = (int)ci[0];
  const size_t np = ci[2];
  alignas(16) uint32_t tt[8][8];
  for (int k = 0; k < 64; k++) tt[k >> 3][k & 7] = ci[12 + k];
  const FoldR fr{ld8<fq>(ci + 4), tt};
  const fq* E = reinterpret_cast<const fq*>(ci + 76);
  fq* tab = reinterpret_cast<fq*>(co + 32);
  for (int e = 0; e < 240; e++) fq_store(tab + e, ld8<fq>(ci + 196 + 8 * e));
  const Tabs<2> t2{{tab, tab + 60}};
  const Tabs<3> t3{{tab, tab + 60, tab + 120}};
  const Tabs<4> t4{{tab, tab + 60, tab + 120, tab + 180}};
  const fq* src[3] = {tab, tab + 60, tab + 120};
  fq* dst[3] = {tab + 240, tab + 270, tab + 300};
  Acc<2> a2; a2.init();
  Acc<4> a4; a4.init();
  LeadNow now; now.init();
  LeadAcc lazy; lazy.init();
  for (size_t p = 0; p < np && p < 15; p++) {
    if (body == 0) pair_ktab<2, M>(a2, t2, p, np, fr);
    else if (body == 1) pair_ktab<4, M>(a4, t4, p, np, fr);
    else if (body == 2) pair_phase1<M, false>(a4, t3, E, p, np, fr);
    else if (body == 3) pair_phase1<M, true>(a4, t3, E, p, np, fr);
    else if (body == 4) pair_prod<M, false>(a4, now, tab, tab + 60, E, p, np, fr);
    else if (body == 5) pair_prod<M, true>(a4, now, tab, tab + 60, E, p, np, fr);
    else if (body == 6) pair_prod<M, true>(a4, lazy, tab, tab + 60, E, p, np, fr);
    else pair_dotp<M != PD_LOAD>(a4, src, dst, p, np, fr);
  }
  lazy.flush(a4.e);
  if (body == 0) { st8(co, a2.e[0]); st8(co + 8, a2.e[1]); }
  else { st8(co, a4.e[0]); st8(co + 8, a4.e[1]); st8(co + 16, a4.e[2]); }
}
DV_LANE(sc_body_load, 4 + 8 + 64 + 120 + 1920, 32 + 1920 + 720, 64, sc_body_case<PD_LOAD>(ci, co);)
DV_LANE(sc_body_fold, 4 + 8 + 64 + 120 + 1920, 32 + 1920 + 720, 64, sc_body_case<PD_FOLD>(ci, co);)
DV_LANE(sc_body_fold_c, 4 + 8 + 64 + 120 + 1920, 32 + 1920 + 720, 64, sc_body_case<PD_FOLD_C>(ci, co);)
DV_LANE(sc_body_fold_to, 4 + 8 + 64 + 120 + 1920, 32 + 1920 + 720, 64, sc_body_case<PD_FOLD_TO>(ci, co);)

// ---- ge_tree_dev.h: fq_signed_window ------------------------------------------------------------------------------------
// in: the canonical scalar, c, W, wide (window w is c bits wide for w < wide and c - 1 above: msm_var.hip; wide = W is
// msm_pip.hip's equal windows); out: W digits (of at most 88), then the last carry, then 1 if scalar bits are left over
DV_LANE(fq_signed_window, 11, 90, 64,
        fq s = ld8<fq>(ci);
        const int c = (int)ci[8]; const int W = (int)ci[9]; const int wide = (int)ci[10];
        uint32_t carry = 0;
        for (int w = 0; w < 88; w++) co[w] = 0;
        for (int w = 0; w < W && w < 88; w++) co[w] = fq_signed_window(s, carry, (uint32_t)(w < wide ? c : c - 1), w + 1 == W);
        co[88] = carry;
        co[89] = fq_is_zero(s) ? 0u : 1u;)

// ---- ge_tree_dev.h: the table walks' digits and the row table's ----------------------------------------------------------
// in: the canonical scalar, c, W; out: W digits (of at most 44) as sign (bit 15) and magnitude, then the carry the top window
// leaves.  The sequential walk of table_mul_acc: fq_fold_sign, then fq_take_window and walk_digit per window.
DV_LANE(walk_digits, 10, 45, 256,
        fq s = ld8<fq>(ci);
        const uint32_t c = ci[8]; const int W = (int)ci[9];
        const bool flip = fq_fold_sign(s);
        uint32_t carry = 0;
        for (int w = 0; w < 44; w++) co[w] = 0;
        for (int w = 0; w < W && w < 44; w++) {
          bool neg;
          const uint32_t mag = walk_digit(fq_take_window(s, carry, c), c, flip, carry, neg);
          co[w] = mag | (neg && mag ? 0x8000u : 0u);
        }
        co[44] = carry;)
// The lane-split walk of table_mul_acc_range, eight lanes of ceil(W / 8) windows: scalar_digit and walk_digit per window, the
// carry into a lane's first window from carry_into.  out: the W digits and the last carry as above, then carry_into at the
// first window of each of the eight lanes (0 for a lane without windows).
DV_LANE(walk_lane_digits, 10, 53, 256,
        fq s = ld8<fq>(ci);
        const int c = (int)ci[8]; const int W = (int)ci[9];
        const bool flip = fq_fold_sign(s);
        const int wpg = (W + 7) / 8;
        uint32_t carry = 0;
        for (int w = 0; w < 53; w++) co[w] = 0;
        for (int lane = 0; lane < 8; lane++) {
          const int w0 = lane * wpg; const int w1 = w0 + wpg < W ? w0 + wpg : W;
          if (w0 >= w1 || w1 > 44) continue;
          carry = carry_into(s, w0, c);
          co[45 + lane] = carry;
          for (int w = w0; w < w1; w++) {
            bool neg;
            const uint32_t mag = walk_digit(scalar_digit(s, w, c) + carry, (uint32_t)c, flip, carry, neg);
            co[w] = mag | (neg && mag ? 0x8000u : 0u);
          }
        }
        co[44] = carry;)
// in: the canonical scalar, c, W; out: the W digit words of row_digit as they go to LDS (of at most 64; magnitude - 1 and the
// sign in bit 15, kNoDigit for a zero digit), then the last carry, then 1 if scalar bits are left over
DV_LANE(row_digits, 10, 66, 256,
        fq s = ld8<fq>(ci);
        const int c = (int)ci[8]; const int W = (int)ci[9];
        const bool flip = fq_fold_sign(s);
        uint32_t carry = 0;
        for (int w = 0; w < 64; w++) co[w] = 0;
        for (int w = 0; w < W && w < 64; w++) co[w] = row_digit(s, carry, c, flip, w == W - 1);
        co[64] = carry;
        co[65] = fq_is_zero(s) ? 0u : 1u;)

// ---- fp_dev.h -----------------------------------------------------------------------------------------------------------
DV_LANE(fp_add, 16, 8, 256, st8(co, fp_add(ld8<fp>(ci), ld8<fp>(ci + 8)));)
DV_LANE(fp_sub, 16, 8, 256, st8(co, fp_sub(ld8<fp>(ci), ld8<fp>(ci + 8)));)
DV_LANE(fp_neg, 8, 8, 256, st8(co, fp_neg(ld8<fp>(ci)));)
DV_LANE(fp_mul, 16, 8, 256, st8(co, fp_mul(ld8<fp>(ci), ld8<fp>(ci + 8)));)
DV_LANE(fp_sqr, 8, 8, 256, st8(co, fp_sqr(ld8<fp>(ci)));)
DV_LANE(fp_mul_small, 9, 8, 256, st8(co, fp_mul_small(ld8<fp>(ci), ci[8]));)
DV_LANE(fp_freeze, 8, 8, 256, st8(co, fp_freeze(ld8<fp>(ci)));)
// in: a, b; out: fp_is_negative(a), fp_eq(a, b), fp_is_zero(a)
DV_LANE(fp_pred, 16, 3, 256,
        const fp a = ld8<fp>(ci); const fp b = ld8<fp>(ci + 8);
        co[0] = fp_is_negative(a) ? 1u : 0u; co[1] = fp_eq(a, b) ? 1u : 0u; co[2] = fp_is_zero(a) ? 1u : 0u;)
DV_LANE(fp_invert, 8, 8, 64, st8(co, fp_invert(ld8<fp>(ci)));)
DV_LANE(fp_pow_p58, 8, 8, 64, st8(co, fp_pow_p58(ld8<fp>(ci)));)
DV_LANE(fp_invsqrt, 8, 9, 64, bool sq; st8(co, fp_invsqrt(ld8<fp>(ci), &sq)); co[8] = sq ? 1u : 0u;)
DV_LANE(ge_add, 64, 32, 64, st_ext(co, ge_add(ld_ext(ci), ld_ext(ci + 32)));)
DV_LANE(ge_double, 32, 32, 64, st_ext(co, ge_double(ld_ext(ci)));)
DV_LANE(ge_add_niels, 57, 32, 64, st_ext(co, ge_add_niels(ld_ext(ci), ld_niels(ci + 32), ci[56] != 0));)
DV_LANE(ge_add_cached, 65, 32, 64, st_ext(co, ge_add_cached(ld_ext(ci), ld_cached(ci + 32), ci[64] != 0));)
DV_LANE(ge_compress, 32, 8, 64, st8(co, ge_compress(ld_ext(ci)));)
// out: the point, then 1 if the encoding decodes (the point is written only then)
DV_LANE(ge_decompress, 8, 33, 64,
        ge_ext r = ge_identity();
        const bool ok = ge_decompress(ld8<fp>(ci), r);
        st_ext(co, r); co[32] = ok ? 1u : 0u;)

// ---- ge_tree_dev.h: ge_tree_quad ----------------------------------------------------------------------------------------
// one workgroup of N lanes per case: in N points, then split; out sh[0] and sh[split]
template <int N>
__device__ __forceinline__ void tree_quad_case(const uint32_t* ci, uint32_t* co, int tid) {
  __shared__ ge_ext sh[N];
  sh[tid] = ld_ext(ci + 32 * tid);
  __syncthreads();
  const int split = (int)ci[32 * N];
  ge_tree_quad(sh, N, split);
  __syncthreads();
  if (tid == 0) {
    st_ext(co, sh[0]);
    st_ext(co + 32, sh[split]);
  }
}
DV_BLOCK(ge_tree_quad64, 32 * 64 + 1, 64, 64, tree_quad_case<64>(ci, co, tid);)
DV_BLOCK(ge_tree_quad256, 32 * 256 + 1, 64, 256, tree_quad_case<256>(ci, co, tid);)

// ---- fp10_dev.h ---------------------------------------------------------------------------------------------------------
DV_LANE(fe10_mul, 20, 10, 256, st10(co, fe10_mul(ld10(ci), ld10(ci + 10)));)
DV_LANE(fe10_sub, 20, 10, 256, st10(co, fe10_sub(ld10(ci), ld10(ci + 10)));)
DV_LANE(fe10_add, 20, 10, 256, st10(co, fe10_add(ld10(ci), ld10(ci + 10)));)
DV_LANE(fe10_from_fp, 8, 10, 256, st10(co, fe10_from_fp(ld8<fp>(ci)));)
DV_LANE(fe10_to_fp, 10, 8, 256, st8(co, fe10_to_fp(ld10(ci)));)
// the points go in as eight-limb extended coordinates through ge10_from_ext and come back through ge10_to_ext
DV_LANE(ge10_roundtrip, 32, 72, 64,
        const ge10 g = ge10_from_ext(ld_ext(ci));
        st10(co, g.X); st10(co + 10, g.Y); st10(co + 20, g.Z); st10(co + 30, g.T);
        st_ext(co + 40, ge10_to_ext(g));)
DV_LANE(ge10_add_ge10, 64, 32, 64, st_ext(co, ge10_to_ext(ge10_add_ge10(ge10_from_ext(ld_ext(ci)), ge10_from_ext(ld_ext(ci + 32)))));)
DV_LANE(ge10_add_niels, 57, 32, 64, st_ext(co, ge10_to_ext(ge10_add_niels(ge10_from_ext(ld_ext(ci)), ld_niels(ci + 32), ci[56] != 0)));)
DV_LANE(ge10_add_cached, 64, 32, 64, st_ext(co, ge10_to_ext(ge10_add_cached(ge10_from_ext(ld_ext(ci)), ld_cached(ci + 32))));)
DV_LANE(ge10_double, 32, 32, 64, st_ext(co, ge10_to_ext(ge10_double(ge10_from_ext(ld_ext(ci)))));)

// in: W = 3 window sums (low window first), then the window width; the sums are read from global memory as the callers do
__global__ __launch_bounds__(64) void k_ge10_horner3(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* ci = in + (size_t)i * 128;  // 96 words of points, the width, padding to keep the points 16-byte aligned
  const int cw = (int)ci[96];
  const ge10 r = ge10_horner_windows(reinterpret_cast<const ge_ext*>(ci), 3, [=](int) { return cw; });
  st_ext(out + (size_t)i * 32, ge10_to_ext(r));
}
extern "C" int dv_ge10_horner3(const uint32_t* in, uint32_t* out, int n) {
  return dv_run(k_ge10_horner3, in, 128, out, 32, n, 64, (n + 63) / 64);
}

// ---- e2_dev.h -----------------------------------------------------------------------------------------------------------
// the curve's a (Montgomery form) is the last operand of every case
DV_LANE(e2_dbl, 32, 24, 64, st_jac(co, e2_dbl(ld_jac(ci), ld8<fq>(ci + 24)));)
DV_LANE(e2_add_mixed, 48, 24, 64, st_jac(co, e2_add_mixed(ld_jac(ci), ld8<fq>(ci + 24), ld8<fq>(ci + 32), ld8<fq>(ci + 40)));)
DV_LANE(e2_add, 56, 24, 64, st_jac(co, e2_add(ld_jac(ci), ld_jac(ci + 24), ld8<fq>(ci + 48)));)
DV_LANE(e2_fq_inv, 8, 8, 64, st8(co, e2_fq_inv(ld8<fq>(ci)));)
// in: x, y, r0..r3, nb, a
DV_LANE(e2_mul_affine, 29, 24, 64,
        st_jac(co, e2_mul_affine(ld8<fq>(ci), ld8<fq>(ci + 8), ci[16], ci[17], ci[18], ci[19], (int)ci[20], ld8<fq>(ci + 21)));)
// in: x, y, eight scalar words, a
DV_LANE(e2_mul_affine256, 32, 24, 64,
        const e2_scalar256 s{ci[16], ci[17], ci[18], ci[19], ci[20], ci[21], ci[22], ci[23]};
        st_jac(co, e2_mul_affine256(ld8<fq>(ci), ld8<fq>(ci + 8), s, ld8<fq>(ci + 24)));)
// one workgroup of kE2Block lanes per case
__global__ __launch_bounds__(kE2Block) void k_e2_block_inverse(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
  __shared__ fq tree[2 * kE2Block];
  const size_t at = ((size_t)blockIdx.x * kE2Block + threadIdx.x) * 8;
  st8(out + at, e2_block_inverse(tree, ld8<fq>(in + at)));
}
extern "C" int dv_e2_block_inverse(const uint32_t* in, uint32_t* out, int n) {
  return dv_run(k_e2_block_inverse, in, 8 * kE2Block, out, 8 * kE2Block, n, kE2Block, n);
}
// in: kE2Block Jacobian points, then a; out: their sum
__global__ __launch_bounds__(kE2Block) void k_e2_block_tree(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
  __shared__ e2_jac sh[kE2Block];
  const uint32_t* ci = in + (size_t)blockIdx.x * (24 * kE2Block + 8);
  e2_block_tree(sh, ld_jac(ci + 24 * threadIdx.x), ld8<fq>(ci + 24 * kE2Block));
  if (threadIdx.x == 0) st_jac(out + (size_t)blockIdx.x * 24, e2_load(&sh[0]));
}
extern "C" int dv_e2_block_tree(const uint32_t* in, uint32_t* out, int n) {
  return dv_run(k_e2_block_tree, in, 24 * kE2Block + 8, out, 24, n, kE2Block, n);
}
