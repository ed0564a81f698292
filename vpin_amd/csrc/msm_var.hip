// msm_var.hip -- variable-base multiscalar multiplication over ristretto255 on gfx950.
//
// Replaces GroupElement::vartime_multiscalar_mul (Spartan/src/group.rs:103-122) where the bases are NOT a generator
// stream with a window table: the verifier's C_LZ = <L, C> over the L decompressed row commitments
// (Spartan/src/dense_mlpoly.rs:381-404), and the row-wise sum of two commitment vectors
// (vPIN_proof_generation/src/commit_test.rs:340-361: comm_para[i] + comm_input[i]).
//
// The sizes are the row counts of Hyrax commitments (2^4 .. 2^14 points), not millions: a bucket method would spend its
// time in the bucket reduction (the second half of this file has one, vpin_msm_bucket: a measured alternative that is on no
// default path below 2^17 terms, profiles/r07_ab_msm_var_bucket.txt).
// One lane per (scalar, point): decompress (RFC 9496 4.3.1: one exponentiation), then a
// left-to-right double-and-add over the scalar's bits in the ten-limb field form (fp10_dev.h), then the block's points are
// summed by the four-lanes-per-addition tree of msm.hip and one partial point per workgroup goes back.  16384 points are
// 256 one-wave workgroups: the whole chip, ~3300 dependent products deep.
#include <cstring>
#include <vector>

#include "ctx.h"
#include "fp10_dev.h"
#include "ge_tree_dev.h"

namespace vpin {

constexpr int kVarBlock = 64;  // one wave per workgroup: 16384 points fill the chip

// partial[b] = sum over the block's lanes of s_i * P_i; bad[0] != 0 when a point does not decode.
// scalars: Montgomery form (mont != 0) or canonical integers.
__global__ __launch_bounds__(kVarBlock) void msm_var_kernel(const fq* __restrict__ scalars, const fp* __restrict__ points, size_t n, int mont,
                                                            ge_ext* __restrict__ partial, uint32_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kVarBlock + threadIdx.x;
  ge10 acc = ge10_identity();
  if (i < n) {
    ge_ext P;
    fq s = fq_load(scalars + i);
    if (mont) s = fq_from_mont(s);
    const bool ok = ge_decompress(fp_load(points + i), P);
    if (!ok) atomicOr(bad, 1u);
    if (ok && !fq_is_zero(s)) {
      // the point as an affine table entry (Z = 1 after decompression): (y + x, y - x, 2 d x y)
      ge_niels q;
      q.ypx = fp_add(P.Y, P.X); q.ymx = fp_sub(P.Y, P.X); q.xy2d = fp_mul(P.T, FP_D2());
      int top = 255;
      while (top > 0 && !((s.v[top >> 5] >> (top & 31)) & 1u)) top--;
      acc = ge10_from_ext(P);
      for (int b = top - 1; b >= 0; b--) {
        acc = ge10_double(acc);
        if ((s.v[b >> 5] >> (b & 31)) & 1u) acc = ge10_add_niels(acc, q, false);
      }
    }
  }
  __shared__ ge_ext sh[kVarBlock];
  sh[threadIdx.x] = ge10_to_ext(acc);
  __syncthreads();
  ge_tree_quad(sh, kVarBlock);
  if (threadIdx.x == 0) ge_store(partial + blockIdx.x, sh[0]);
}

// out[i] = compress(decompress(a[i]) + decompress(b[i]))
__global__ __launch_bounds__(kVarBlock) void points_add_kernel(const fp* __restrict__ a, const fp* __restrict__ b, size_t n,
                                                               fp* __restrict__ out, uint32_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kVarBlock + threadIdx.x;
  if (i >= n) return;
  ge_ext P, Q;
  const bool ok = ge_decompress(fp_load(a + i), P) && ge_decompress(fp_load(b + i), Q);
  if (!ok) { atomicOr(bad, 1u); return; }
  fp_store(out + i, ge_compress(ge_add(P, Q)));
}

// one block: sum of m partial points -> compressed and canonical X|Y|Z|T
__global__ __launch_bounds__(kVarBlock) void msm_var_finish_kernel(const ge_ext* __restrict__ partial, size_t m, fp* __restrict__ out32,
                                                                   fp* __restrict__ out_xyzt) {
  __shared__ ge_ext sh[kVarBlock];
  ge_ext acc = ge_identity();
  for (size_t k = threadIdx.x; k < m; k += kVarBlock) acc = ge_add(acc, ge_load(partial + k));
  sh[threadIdx.x] = acc;
  __syncthreads();
  ge_tree_quad(sh, kVarBlock);
  if (threadIdx.x == 0) {
    const ge_ext r = sh[0];
    ge_store_result(out32, out_xyzt, r);
  }
}

// ---- bucket method (vpin_msm_bucket) -------------------------------------------------------------------------------------
// The variable-base side of a batch verification (verify.cpp) from 2^17 terms on; below that msm_var_kernel is faster
// (profiles/r07_ab_msm_var_bucket.txt: 2.0 .. 2.3 ms flat against 1.5 .. 1.7 ms up to 2^16 terms, 2.7 against 3.0 ms at 2^17; 1.5 ms of
// every call is the single-lane Horner of bkt_finish_kernel).  Signed windows, 2^(c-1) buckets per window:
//   bkt_prep_kernel     one lane per point: decompress once (RFC 9496 4.3.1) into the 96-byte affine form (y + x, y - x, 2 d x y),
//                       recode the canonical scalar into W signed digits (|d| in bits 0..14, sign in bit 15), dig[w n + i]
//   bkt_sort_kernel     one workgroup per window: counting sort of the non-zero digits by bucket (histogram and scan in LDS,
//                       the ordered list of (point index | sign << 31) and the bucket offsets in global memory)
//   bkt_accum_kernel    one lane per (window, bucket): the bucket's points into one ten-limb accumulator with the complete
//                       unified addition (a point may meet itself or its negative); ~n / 2^(c-1) additions per lane
//   bkt_reduce_kernel   one workgroup per window: lane t owns K consecutive buckets, S_t = sum B_i and the running-sum
//                       W_t = sum (i + 1) B_i, adds (t K) S_t by double-and-add (t K < 2^12), block tree
//   bkt_finish_kernel   sum_w 2^(offset of window w) (window w): Horner on one lane (253 dependent doublings: the floor of a
//                       call); compressed + X|Y|Z|T
// WINDOW WIDTHS.  The 253 bits of a canonical scalar are cut into W = floor(253 / c) + 1 windows of c or c - 1 bits: the first
// `wide` windows take c bits, the others and the top window c - 1 (wide = 254 - c - (W - 1)(c - 1), so the widths add up to
// 253).  Equal windows of c bits leave the top window 253 mod c bits -- ONE bit at c = 9 or 12 -- and then every point of the
// list lands in two buckets of that window and one lane adds n / 2 points in a row (40 ms at 2^15 terms: the first version of
// this kernel did that).  With widths that differ by at most one bit no window has fewer than 2^(c-2) buckets in use.  The top
// window is c - 1 bits and a carry: at most 2^(c-1), never negated.
// Everything between the kernels lives in global memory (the sorted lists are n W u32: 10 MB at 2^17), so n is bounded by the
// 31-bit list entry only.  Worst case: n equal scalars put every point of a window into one bucket and one lane adds them all
// (~0.3 s at 2^17); a batch's scalars carry a random 128-bit weight each, so the verifier never meets it.
constexpr int kBktBlock = 256;       // reduce
constexpr int kBktSortBlock = 1024;  // sort: one workgroup per window
constexpr int kBktMaxC = 13;         // 4096 buckets: the LDS histogram of bkt_sort_kernel
constexpr int kBktLimbs = 40;

struct BktShape { int c, W, wide; uint32_t B; };
static BktShape bkt_shape(size_t n) {
  int lg = 0;
  while (((size_t)2 << lg) <= n) lg++;
  int c = lg - 3;
  c = c < 4 ? 4 : c > kBktMaxC ? kBktMaxC : c;
  const int W = 253 / c + 1;
  return BktShape{c, W, 254 - c - (W - 1) * (c - 1), 1u << (c - 1)};
}

__global__ __launch_bounds__(kVarBlock) void bkt_prep_kernel(const fq* __restrict__ scalars, const fp* __restrict__ points, size_t n, int c,
                                                             int W, int wide, ge_niels* __restrict__ gn, uint16_t* __restrict__ dig,
                                                             uint32_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kVarBlock + threadIdx.x;
  if (i >= n) return;
  ge_ext P;
  const bool ok = ge_decompress(fp_load(points + i), P);
  if (!ok) {
    atomicOr(bad, 1u);
    P = ge_identity();
  }
  ge_store(gn + i, ge_niels{fp_add(P.Y, P.X), fp_sub(P.Y, P.X), fp_mul(P.T, FP_D2())});
  fq s = fq_from_mont(fq_load(scalars + i));  // canonical: below 2^253
  uint32_t carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; w++) {
    // the top window holds c - 1 bits and a carry: at most 2^(c-1) = the number of buckets, never negated
    const uint16_t d = fq_signed_window(s, carry, (uint32_t)(w < wide ? c : c - 1), w + 1 == W);
    dig[(size_t)w * n + i] = ok ? d : (uint16_t)0;
  }
}

// sorted[w n + start[w (B + 1) + b] ..) = the points of bucket b of window w; start[w (B + 1) + B] = the window's non-zero digits
__global__ __launch_bounds__(kBktSortBlock) void bkt_sort_kernel(const uint16_t* __restrict__ dig, size_t n, uint32_t B,
                                                                 uint32_t* __restrict__ start, uint32_t* __restrict__ sorted) {
  __shared__ uint32_t cnt[1u << (kBktMaxC - 1)];
  __shared__ uint32_t sc[kBktSortBlock];
  const uint32_t t = threadIdx.x, w = blockIdx.x;
  const uint16_t* d = dig + (size_t)w * n;
  uint32_t* st = start + (size_t)w * (B + 1);
  uint32_t* out = sorted + (size_t)w * n;
  for (uint32_t i = t; i < B; i += kBktSortBlock) cnt[i] = 0;
  __syncthreads();
  for (size_t j = t; j < n; j += kBktSortBlock) {
    const uint32_t m = d[j] & 0x7fffu;
    if (m) atomicAdd(&cnt[m - 1], 1u);
  }
  __syncthreads();
  const uint32_t per = B >= kBktSortBlock ? B / kBktSortBlock : 1u;
  const bool mine = t * per < B;
  uint32_t loc = 0;
  if (mine)
    for (uint32_t i = 0; i < per; i++) loc += cnt[t * per + i];
  sc[t] = loc;
  __syncthreads();
  for (uint32_t off = 1; off < kBktSortBlock; off <<= 1) {
    const uint32_t v = t >= off ? sc[t - off] : 0u;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  if (mine) {
    uint32_t pos = sc[t] - loc;
    for (uint32_t i = 0; i < per; i++) {
      const uint32_t k = cnt[t * per + i];
      st[t * per + i] = pos;
      cnt[t * per + i] = pos;  // the scatter's cursor
      pos += k;
    }
  }
  if (t == kBktSortBlock - 1) st[B] = sc[t];
  __syncthreads();
  for (size_t j = t; j < n; j += kBktSortBlock) {
    const uint32_t v = d[j], m = v & 0x7fffu;
    if (m) out[atomicAdd(&cnt[m - 1], 1u)] = (uint32_t)j | ((v & 0x8000u) << 16);
  }
}

// limb l of bucket (w, b) at bkt[(w 40 + l) B + b]: limb-strided with stride B
__global__ __launch_bounds__(kVarBlock) void bkt_accum_kernel(const ge_niels* __restrict__ gn, const uint32_t* __restrict__ start,
                                                              const uint32_t* __restrict__ sorted, size_t n, uint32_t B, int W,
                                                              uint32_t* __restrict__ bkt) {
  const size_t idx = (size_t)blockIdx.x * kVarBlock + threadIdx.x;
  if (idx >= (size_t)W * B) return;
  const size_t w = idx / B, b = idx - w * B;
  const uint32_t lo = start[w * (B + 1) + b], hi = start[w * (B + 1) + b + 1];
  const uint32_t* list = sorted + w * n;
  ge10 acc = ge10_identity();
#pragma unroll 1
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t v = list[e];
    acc = ge10_add_niels(acc, ge_load(gn + (v & 0x7fffffffu)), (v >> 31) != 0);
  }
  ge10_store_strided(bkt + (w * kBktLimbs) * B + b, B, acc);
}

// wsum[w] = sum_b (b + 1) bucket(w, b)
__global__ __launch_bounds__(kBktBlock) void bkt_reduce_kernel(const uint32_t* __restrict__ bkt, uint32_t B, ge_ext* __restrict__ wsum) {
  __shared__ ge_ext sh[kBktBlock];
  const uint32_t t = threadIdx.x, w = blockIdx.x;
  const uint32_t K = B >= kBktBlock ? B / kBktBlock : 1u, T = B / K;
  const uint32_t* base = bkt + ((size_t)w * kBktLimbs) * B;
  ge10 wt = ge10_identity();
  if (t < T) {
    ge10 acc = ge10_identity();
#pragma unroll 1
    for (int i = (int)K - 1; i >= 0; i--) {
      acc = ge10_add_ge10(acc, ge10_load_strided(base + t * K + (uint32_t)i, B));
      wt = ge10_add_ge10(wt, acc);
    }
    const uint32_t m = t * K;  // the lane's buckets weigh m + 1 .. m + K: m times their plain sum on top of the running sums
    if (m) {
      ge10 u = acc;
#pragma unroll 1
      for (int bit = 30 - __clz(m); bit >= 0; bit--) {
        u = ge10_double(u);
        if ((m >> bit) & 1u) u = ge10_add_ge10(u, acc);
      }
      wt = ge10_add_ge10(wt, u);
    }
  }
  sh[t] = ge10_to_ext(wt);
  __syncthreads();
  ge_tree_quad(sh, kBktBlock);
  if (t == 0) ge_store(wsum + w, sh[0]);
}

// one wave: sum_w 2^(c w) wsum[w] -> compressed and canonical X|Y|Z|T
__global__ __launch_bounds__(kVarBlock) void bkt_finish_kernel(const ge_ext* __restrict__ wsum, int W, int c, int wide, fp* __restrict__ out32,
                                                               fp* __restrict__ out_xyzt) {
  if (threadIdx.x != 0) return;
  const ge_ext r = ge10_to_ext(ge10_horner_windows(wsum, W, [=](int w) { return w < wide ? c : c - 1; }));  // window w: c or c - 1 bits
  ge_store_result(out32, out_xyzt, r);
}

}  // namespace vpin

using namespace vpin;

// What vpin_msm and vpin_msm_bucket share: the argument checks, the scalars and points to the device, the `bad` flag of a
// point that does not decode, and the result (compressed | X|Y|Z|T) home.  launch(scalars, points, out32, out_xyzt, bad)
// enqueues the kernels between; n_limit: the first n the method cannot take.
template <class Launch>
static int msm_var_run(vpin_ctx* c, const uint8_t* scalars_mont, const uint8_t* points_compressed, size_t n, size_t n_limit,
                       uint8_t* out_compressed, uint8_t* out_xyzt, Launch launch) {
  if (!c || !scalars_mont || !points_compressed || n == 0 || (!out_compressed && !out_xyzt)) return VPIN_EINVAL;
  if (n >= n_limit) return VPIN_ESHAPE;
  (void)hipSetDevice(c->device);
  DevBuf ds(c), dp(c), dout(c), dbad(c);
  if (ds.alloc(n * 32) || dp.alloc(n * 32) || dout.alloc(32 + 128) || dbad.alloc(4)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(ds.p, scalars_mont, n * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(dp.p, points_compressed, n * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemsetAsync(dbad.p, 0, 4, c->stream));
  if (const int rc = launch((const fq*)ds.p, (const fp*)dp.p, (fp*)dout.p, (fp*)((uint8_t*)dout.p + 32), (uint32_t*)dbad.p)) return rc;
  VPIN_HIP_TRY(hipGetLastError());
  uint8_t host[160];
  uint32_t bad = 0;
  VPIN_HIP_TRY(hipMemcpyAsync(host, dout.p, 160, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(&bad, dbad.p, 4, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  if (bad) return VPIN_EVERIFY;
  if (out_compressed) memcpy(out_compressed, host, 32);
  if (out_xyzt) memcpy(out_xyzt, host + 32, 128);
  return VPIN_OK;
}

extern "C" {

// GroupElement::vartime_multiscalar_mul (Spartan/src/group.rs:103-122) over arbitrary points given in their compressed
// ristretto255 encodings: out = sum_i s_i * decompress(P_i).  VPIN_EVERIFY when an encoding does not decode (the reference
// unwraps CompressedGroup::decompress and panics).
int vpin_msm(vpin_ctx* c, const uint8_t* scalars_mont, const uint8_t* points_compressed, size_t n, uint8_t* out_compressed,
             uint8_t* out_xyzt) {
  return msm_var_run(c, scalars_mont, points_compressed, n, (size_t)-1, out_compressed, out_xyzt,
                     [&](const fq* ds, const fp* dp, fp* out32, fp* out128, uint32_t* dbad) -> int {
    const size_t nb = (n + kVarBlock - 1) / kVarBlock;
    DevBuf dpart(c);
    if (dpart.alloc(nb * sizeof(ge_ext))) return VPIN_ENOMEM;
    ProfScope ps(c, VPIN_K_MSM, 64.0 * (double)n);
    hipLaunchKernelGGL(msm_var_kernel, dim3((unsigned)nb), dim3(kVarBlock), 0, c->stream, ds, dp, n, 1, (ge_ext*)dpart.p, dbad);
    hipLaunchKernelGGL(msm_var_finish_kernel, dim3(1), dim3(kVarBlock), 0, c->stream, (const ge_ext*)dpart.p, nb, out32, out128);
    return VPIN_OK;
  });
}

// vpin_msm by the bucket method (see the kernels above): the same contract; the batch verifier's kernel from 2^17 terms on.
// n < 2^31: a list entry is a 31-bit index and a sign
int vpin_msm_bucket(vpin_ctx* c, const uint8_t* scalars_mont, const uint8_t* points_compressed, size_t n, uint8_t* out_compressed,
                    uint8_t* out_xyzt) {
  return msm_var_run(c, scalars_mont, points_compressed, n, (size_t)1 << 31, out_compressed, out_xyzt,
                     [&](const fq* ds, const fp* dp, fp* out32, fp* out128, uint32_t* dbad) -> int {
    const BktShape sh = bkt_shape(n);
    const size_t W = (size_t)sh.W, B = sh.B;
    DevBuf dgn(c), ddig(c), dstart(c), dsorted(c), dbkt(c), dws(c);
    if (dgn.alloc(n * sizeof(ge_niels)) || ddig.alloc(W * n * 2) || dstart.alloc(W * (B + 1) * 4) || dsorted.alloc(W * n * 4) ||
        dbkt.alloc(W * B * kBktLimbs * 4) || dws.alloc(W * sizeof(ge_ext)))
      return VPIN_ENOMEM;
    ProfScope ps(c, VPIN_K_MSM, 64.0 * (double)n);
    hipLaunchKernelGGL(bkt_prep_kernel, dim3((unsigned)((n + kVarBlock - 1) / kVarBlock)), dim3(kVarBlock), 0, c->stream, ds, dp, n, sh.c,
                       sh.W, sh.wide, (ge_niels*)dgn.p, (uint16_t*)ddig.p, dbad);
    hipLaunchKernelGGL(bkt_sort_kernel, dim3((unsigned)W), dim3(kBktSortBlock), 0, c->stream, (const uint16_t*)ddig.p, n, sh.B,
                       (uint32_t*)dstart.p, (uint32_t*)dsorted.p);
    hipLaunchKernelGGL(bkt_accum_kernel, dim3((unsigned)((W * B + kVarBlock - 1) / kVarBlock)), dim3(kVarBlock), 0, c->stream,
                       (const ge_niels*)dgn.p, (const uint32_t*)dstart.p, (const uint32_t*)dsorted.p, n, sh.B, sh.W, (uint32_t*)dbkt.p);
    hipLaunchKernelGGL(bkt_reduce_kernel, dim3((unsigned)W), dim3(kBktBlock), 0, c->stream, (const uint32_t*)dbkt.p, sh.B, (ge_ext*)dws.p);
    hipLaunchKernelGGL(bkt_finish_kernel, dim3(1), dim3(kVarBlock), 0, c->stream, (const ge_ext*)dws.p, sh.W, sh.c, sh.wide, out32, out128);
    return VPIN_OK;
  });
}

// out[i] = compress(decompress(a[i]) + decompress(b[i])): the row-wise sum of two Hyrax commitments
// (vPIN_proof_generation/src/commit_test.rs:340-361 on the verifier's side, proof_point_mult.rs:75-80 on the prover's)
int vpin_points_add(vpin_ctx* c, const uint8_t* a_compressed, const uint8_t* b_compressed, size_t n, uint8_t* out_compressed) {
  if (!c || !a_compressed || !b_compressed || !out_compressed || n == 0) return VPIN_EINVAL;
  (void)hipSetDevice(c->device);
  DevBuf da(c), db(c), dout(c), dbad(c);
  if (da.alloc(n * 32) || db.alloc(n * 32) || dout.alloc(n * 32) || dbad.alloc(4)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(da.p, a_compressed, n * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(db.p, b_compressed, n * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemsetAsync(dbad.p, 0, 4, c->stream));
  hipLaunchKernelGGL(points_add_kernel, dim3((unsigned)((n + kVarBlock - 1) / kVarBlock)), dim3(kVarBlock), 0, c->stream, (const fp*)da.p,
                     (const fp*)db.p, n, (fp*)dout.p, (uint32_t*)dbad.p);
  VPIN_HIP_TRY(hipGetLastError());
  uint32_t bad = 0;
  VPIN_HIP_TRY(hipMemcpyAsync(out_compressed, dout.p, n * 32, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(&bad, dbad.p, 4, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return bad ? VPIN_EVERIFY : VPIN_OK;
}

}  // extern "C"
