// enc_fc.hip -- the device stages of the encrypted fully connected layer and of the encrypted average pooling (driven by
// enc_fc.cpp), beside enc_conv.hip whose load, convolution, normalisation, RLC and reduce kernels they reuse.
//
//   e2_matvec_kernel      C[p][j] = sum_k W[k][j] * X[p][k]: one lane per (k, j) term on grid (blocks of k, N, P), double-and-add
//                         over the lane's own 32-bit weight (mixed addition), then the workgroup's LDS tree with the complete
//                         addition; e2_reduce_kernel sums over the blocks of k.  A template over the weights' type: <false> takes
//                         u32 words, <true> int32 words (vpin_enc_fc_signed): the lane multiplies by |w| and takes the negated
//                         point (x, q - y) for w < 0; the same tree, so X[k] under w and -w cancels to the flagged identity
//   e2_scalar_mul_kernel  T_i = s_i * X_i, one lane per point, s_i a u128: the multiplications of the layer's RLC check
//   e2_pool_sums_kernel   one lane per pooled output: the k*k - 1 accumulators e_0, e_0 + e_1, ... of its window (the first
//                         operands of the pooling's additions) and a flag when one of them is the identity
//   e2_chain_scan_kernel  one workgroup per chain of K Jacobian points: the inclusive prefixes T_0 + .. + T_k as a scan in LDS
//                         with the complete addition, in tiles of kE2Block with a carried prefix; with e2_scalar_mul_kernel
//                         before it and ONE e2_to_affine_kernel launch over products and prefixes after it, this is the tail
//                         of a layer's RLC check (mul_chain, over any E2Points): one shared inversion per 256 points instead of
//                         one per addition
// As in enc_conv.hip the accumulators are named registers (one e2_jac, the scalar as shifted words): no per-lane arrays.
#include "e2_dev.h"
#include "enc_conv.h"

namespace vpin {

namespace {

// grid: x = blocks of k, y = output j, z = row p; W is K x N row-major, u32 or (Signed) int32 words: a negative weight
// multiplies the negated point by |w|, and |INT32_MIN| = 2^31 is taken in unsigned arithmetic
template <bool Signed>
__global__ __launch_bounds__(kE2Block) void e2_matvec_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                             const uint8_t* __restrict__ inf, const uint32_t* __restrict__ W,
                                                             size_t K, size_t N, fq a, e2_jac* __restrict__ parts) {
  __shared__ e2_jac sh[kE2Block];
  const size_t k = (size_t)blockIdx.x * kE2Block + threadIdx.x, j = blockIdx.y, p = blockIdx.z;
  e2_jac acc = e2_identity();
  if (k < K && !inf[p * K + k]) {  // a zero weight gives the identity inside e2_mul_affine
    const uint32_t w = W[k * N + j];
    const bool minus = Signed && (int32_t)w < 0;
    const uint32_t m = minus ? 0u - w : w;
    const fq y = fq_load(Y + p * K + k);
    acc = e2_mul_affine(fq_load(X + p * K + k), minus ? fq_neg(y) : y, 0u, 0u, 0u, m, 32, a);
  }
  e2_block_tree(sh, acc, a);
  if (threadIdx.x == 0) e2_store(parts + ((p * N + j) * gridDim.x + blockIdx.x), e2_load(&sh[0]));
}

__global__ __launch_bounds__(kE2Block) void e2_scalar_mul_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                                 const uint8_t* __restrict__ inf, const uint4* __restrict__ s,
                                                                 size_t n, fq a, e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  e2_jac acc = e2_identity();
  if (!inf[i]) {
    const uint4 ss = s[i];
    acc = e2_mul_affine(fq_load(X + i), fq_load(Y + i), ss.x, ss.y, ss.z, ss.w, 128, a);
  }
  e2_store(out + i, acc);
}

// grid: x = blocks of outputs, y = plane.  acc[(plane * n_out + t) * (taps - 1) + m] = e_0 + .. + e_m for m < taps - 1: the
// accumulator BEFORE element m + 1 is added; acc_identity[plane * n_out + t] = 1 when one of them is the identity
__global__ __launch_bounds__(64) void e2_pool_sums_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                          const uint8_t* __restrict__ inf, E2Geom g, fq a,
                                                          e2_jac* __restrict__ acc_out, uint8_t* __restrict__ acc_identity) {
  const int t = (int)(blockIdx.x * 64 + threadIdx.x), n_out = g.oh * g.ow;
  if (t >= n_out) return;
  const size_t plane = blockIdx.y, base = plane * (size_t)g.H * g.W, o = plane * (size_t)n_out + t;
  const int taps = g.fh * g.fw;
  e2_jac acc = e2_identity();
  uint8_t bad = 0;
  for (int m = 0; m + 1 < taps; m++) {
    const size_t idx = base + (size_t)e2_window_index(g, t, m);  // no padding: every window lies inside the plane
    if (!inf[idx]) acc = e2_add_mixed(acc, fq_load(X + idx), fq_load(Y + idx), a);
    if (e2_is_identity(acc)) bad = 1;
    e2_store(acc_out + o * (size_t)(taps - 1) + m, acc);
  }
  acc_identity[o] = bad;
}

// grid: x = chain.  acc[p * K + k] = T[p * K] + .. + T[p * K + k].  A scan associates differently from a left-to-right loop;
// the group elements are the same, and every addition is complete: an identity term or prefix adds nothing, equal segment sums
// double, opposite ones give the identity, from which the chain goes on
__global__ __launch_bounds__(kE2Block) void e2_chain_scan_kernel(const e2_jac* __restrict__ T, size_t K, fq a,
                                                                 e2_jac* __restrict__ acc) {
  __shared__ e2_jac sh[kE2Block];
  const int tid = threadIdx.x;
  const e2_jac* t = T + (size_t)blockIdx.x * K;
  e2_jac* o = acc + (size_t)blockIdx.x * K;
  e2_jac carry = e2_identity();
  for (size_t base = 0; base < K; base += kE2Block) {
    const size_t k = base + tid;
    const int live = (int)(K - base < (size_t)kE2Block ? K - base : (size_t)kE2Block);  // a short tile is the last one
    e2_jac v = e2_identity();
    if (k < K) v = e2_load(t + k);
    e2_store(&sh[tid], v);
    __syncthreads();
    for (int d = 1; d < live; d <<= 1) {
      const bool on = tid >= d;
      e2_jac left = e2_identity();
      if (on) left = e2_load(&sh[tid - d]);
      __syncthreads();
      if (on) {
        v = e2_add(left, v, a);
        e2_store(&sh[tid], v);
      }
      __syncthreads();
    }
    v = e2_add(carry, v, a);
    if (k < K) e2_store(o + k, v);
    if (tid == kE2Block - 1) e2_store(&sh[tid], v);  // the next tile's carry; nobody reads this slot after the last step
    __syncthreads();
    carry = e2_load(&sh[kE2Block - 1]);
    __syncthreads();
  }
}

}  // namespace

// C = X * W per row over the loaded points (P x K), normalised: canonical bytes to the host, Montgomery coordinates resident
// as `out` with the geometry "P planes of 1 x N and no taps", so that rlc() returns sum_j r[p][j] * C[p][j]
int EncConvDev::matvec(size_t P, size_t K, size_t N, const void* weights, bool is_signed, uint8_t* c_x, uint8_t* c_y, uint8_t* c_inf) {
  (void)hipSetDevice(c->device);
  g = ConvGeom();
  g.P = P; g.oh = 1; g.ow = N;
  const size_t nblk = blocks_of(K, kE2Block), n_out = P * N;
  DevBuf w(c), parts(c), jac(c);
  if (w.alloc(K * N * 4) || parts.alloc(n_out * nblk * sizeof(e2_jac)) || jac.alloc(n_out * sizeof(e2_jac))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(w.p, weights, K * N * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(is_signed ? e2_matvec_kernel<true> : e2_matvec_kernel<false>, dim3((unsigned)nblk, (unsigned)N, (unsigned)P),
                     dim3(kE2Block), 0, c->stream, in.X(), in.Y(), in.F(), (const uint32_t*)w.p, K, N, e2_curve_a(), (e2_jac*)parts.p);
  VPIN_HIP_TRY(hipGetLastError());
  const int rc = e2_reduce(c, (const e2_jac*)parts.p, n_out, nblk, (e2_jac*)jac.p);
  if (rc) return rc;
  return e2_emit(c, (const e2_jac*)jac.p, n_out, c_x, c_y, c_inf, &out);
}

// the tail over pts, P chains of K terms: T = s * X (Jacobian), the prefixes of every chain, and both normalised by ONE launch
// over the 2 P K points; canonical bytes and flags to the host
int mul_chain(vpin_ctx* c, const E2Points& pts, const uint8_t* s_le16, size_t P, size_t K, uint8_t* t_x, uint8_t* t_y, uint8_t* t_inf,
              uint8_t* acc_x, uint8_t* acc_y, uint8_t* acc_inf) {
  (void)hipSetDevice(c->device);
  const size_t n = P * K;
  DevBuf s(c), jac(c);
  if (s.alloc(n * 16) || jac.alloc(2 * n * sizeof(e2_jac))) return VPIN_ENOMEM;
  const fq a = e2_curve_a();
  e2_jac* prod = (e2_jac*)jac.p;
  VPIN_HIP_TRY(hipMemcpyAsync(s.p, s_le16, n * 16, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_scalar_mul_kernel, dim3(blocks_of(n, kE2Block)), dim3(kE2Block), 0, c->stream, pts.X(), pts.Y(), pts.F(),
                     (const uint4*)s.p, n, a, prod);
  VPIN_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(e2_chain_scan_kernel, dim3((unsigned)P), dim3(kE2Block), 0, c->stream, (const e2_jac*)prod, K, a, prod + n);
  VPIN_HIP_TRY(hipGetLastError());
  E2Affine aff(c);
  int rc = aff.normalise(c, prod, 2 * n);
  if (!rc) rc = aff.copy_out(c, 0, n, t_x, t_y, t_inf);
  if (!rc) rc = aff.copy_out(c, n, n, acc_x, acc_y, acc_inf);
  if (rc) return rc;
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

// the accumulators of every pooled output's additions (geom: fh = fw = k, pad 0), normalised, as canonical bytes in the
// order of the addition list: outputs() x (taps() - 1) points; acc_identity: one byte per output
int EncConvDev::pool_sums(const ConvGeom& geom, uint8_t* acc_x, uint8_t* acc_y, uint8_t* acc_identity) {
  (void)hipSetDevice(c->device);
  const size_t n_out = geom.outputs(), n = n_out * (geom.taps() - 1);
  DevBuf jac(c), bad(c);
  if (jac.alloc(n * sizeof(e2_jac)) || bad.alloc(n_out)) return VPIN_ENOMEM;
  hipLaunchKernelGGL(e2_pool_sums_kernel, dim3(blocks_of(geom.oh * geom.ow, 64), (unsigned)geom.P), dim3(64), 0, c->stream, in.X(), in.Y(),
                     in.F(), e2_geom(geom), e2_curve_a(), (e2_jac*)jac.p, (uint8_t*)bad.p);
  VPIN_HIP_TRY(hipGetLastError());
  E2Affine aff(c);  // the flags that matter are the kernel's, per output: the points' own are not copied
  int rc = aff.normalise(c, (const e2_jac*)jac.p, n);
  if (!rc) rc = aff.copy_out(c, 0, n, acc_x, acc_y, nullptr);
  if (rc) return rc;
  VPIN_HIP_TRY(hipMemcpyAsync(acc_identity, bad.p, n_out, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

}  // namespace vpin
