// enc_convmc.hip -- the device stages of the trained convolution layer (driven by enc_convmc.cpp): one signed filter per
// (output channel, input channel) over groups x C ciphertext planes on E2, and the sums of its random-linear-combination check.
// Beside enc_conv.hip and enc_fc.hip, whose load, normalisation (e2_emit), reduce, scalar-multiplication and chain-scan kernels it
// reuses.
//
//   e2_convmc_kernel   one workgroup per (block of output pixels, output channel o, group): the weights of one o are uniform
//                      per workgroup.  A workgroup is slots x px lanes, lane = slot * px + pixel: slot s walks the input
//                      channels s, s + slots, .. of its pixel with a joint double-and-add over their taps, from the top set bit
//                      of the largest |w| of o down, adding the pixel for a positive weight and the negated pixel (x, q - y) for
//                      a negative one; the slots' partial sums of a pixel are joined by a tree in LDS with the complete addition
//                      (as e2_matvec_kernel joins over k).  slots = min(C, 16), px = min(64, 256 / slots): up to four channels a
//                      slot is a whole wave, so a wave diverges only on padding and identity pixels; above, the lanes of a wave
//                      hold up to four channels and diverge on their weights' bits
//   e2_rlc_mc_kernel   e2_rlc_kernel with a descriptor per sum: the term's plane (or the outputs), its tap and the pair (g, o)
//                      whose r vector weighs it; one lane per (sum, term), S lanes a sum: a sum of 256 terms or more takes whole
//                      workgroups (e2_reduce_kernel adds their partials), shorter sums share one
//   e2_bias_add_kernel out[g][o][t] = C[g][o][t] + bias[g][o] (vpin_enc_conv2d_mc_bias): one lane per output over the resident,
//                      normalised C (EncConvDev::out), one mixed addition each, complete by case; one normalisation follows
//   e2_negate_kernel   S = -B' where the weight is negative: Y -> q - Y on the Jacobian sums, before the one normalisation
// Exactness: every addition is complete by case (e2_dev.h): two channels that hold the same pixel under the same weight double
// in the tree, a pixel and its negative cancel to the flagged identity.  The accumulators are named registers: no per-lane arrays.
#include "e2_dev.h"
#include "enc_conv.h"

namespace vpin {

namespace {

constexpr int kMcMaxSlots = 16;
constexpr int kBiasBlock = 64;  // one wave: a lane is one mixed addition

// grid: x = blocks of px output pixels, y = output channel, z = group; block = slots * px <= kE2Block lanes
__global__ __launch_bounds__(kE2Block) void e2_convmc_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                             const uint8_t* __restrict__ inf, E2Geom g, int C, int slots, int px,
                                                             const int32_t* __restrict__ W, const uint8_t* __restrict__ connect,
                                                             const int32_t* __restrict__ top_bit, fq a, e2_jac* __restrict__ out) {
  __shared__ e2_jac sh[kE2Block];
  const int tid = threadIdx.x, s = tid / px, p = tid % px;
  const int n_pix = g.oh * g.ow, t = (int)blockIdx.x * px + p, taps = g.fh * g.fw;
  const size_t o = blockIdx.y, n_out = gridDim.y, grp = blockIdx.z;
  e2_jac acc = e2_identity();
  if (t < n_pix) {
    for (int bit = top_bit[o]; bit >= 0; bit--) {
      if (!e2_is_identity(acc)) acc = e2_dbl(acc, a);
      for (int c = s; c < C; c += slots) {
        if (!connect[o * C + c]) continue;  // its weights are not read
        const int32_t* w = W + (o * C + c) * (size_t)taps;
        const size_t base = (grp * C + c) * (size_t)g.H * g.W;
        for (int k = 0; k < taps; k++) {
          const int32_t wk = w[k];
          const uint32_t m = wk < 0 ? 0u - (uint32_t)wk : (uint32_t)wk;
          if (!((m >> bit) & 1u)) continue;
          const long wi = e2_window_index(g, t, k);
          if (wi < 0 || inf[base + wi]) continue;  // padding and flagged pixels are the identity
          const fq y = fq_load(Y + base + wi);
          acc = e2_add_mixed(acc, fq_load(X + base + wi), wk < 0 ? fq_neg(y) : y, a);
        }
      }
    }
  }
  e2_store(&sh[tid], acc);
  __syncthreads();
  for (int width = 1; width < slots; width <<= 1) {  // neighbours first; slot s takes slot s + width: (s + width) * px + p < slots * px
    if (s % (2 * width) == 0 && s + width < slots) e2_store(&sh[tid], e2_add(e2_load(&sh[tid]), e2_load(&sh[tid + width * px]), a));
    __syncthreads();
  }
  if (s == 0 && t < n_pix) e2_store(out + ((grp * n_out + o) * (size_t)n_pix + t), e2_load(&sh[tid]));
}

// desc[sum] = {plane, tap, pair, 0}: plane >= 0 a plane of X, -1 the outputs of the pair, -2 no terms; r and the outputs are
// indexed pair * n_terms + t.  S lanes per sum, a power of two: kE2Block with nblk blocks per sum, or the least S >= n_terms with
// nblk = 1 and kE2Block / S sums per workgroup (a 1 x 1 output plane has one term per sum: 256 sums a workgroup, not one).
// grid: x = (sums in groups of kE2Block / S) * nblk + block of terms
__global__ __launch_bounds__(kE2Block) void e2_rlc_mc_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                             const uint8_t* __restrict__ inf, const fq* __restrict__ OX,
                                                             const fq* __restrict__ OY, const uint8_t* __restrict__ oinf, E2Geom g,
                                                             const int4* __restrict__ desc, size_t n_sums, unsigned nblk, int S,
                                                             size_t n_terms, const uint4* __restrict__ r, fq a,
                                                             e2_jac* __restrict__ parts) {
  __shared__ e2_jac sh[kE2Block];
  const int tid = threadIdx.x, j = tid % S;
  const size_t sum = (size_t)(blockIdx.x / nblk) * (kE2Block / S) + tid / S, t = (size_t)(blockIdx.x % nblk) * S + j;
  const bool live = sum < n_sums;
  int4 d = make_int4(-2, 0, 0, 0);
  if (live) d = desc[sum];
  bool have = false;
  fq x = fq_zero(), y = fq_zero();
  if (t < n_terms && d.x >= -1) {
    if (d.x < 0) {
      const size_t idx = (size_t)d.z * n_terms + t;
      if (!oinf[idx]) { have = true; x = fq_load(OX + idx); y = fq_load(OY + idx); }
    } else {
      const long wi = e2_window_index(g, (int)t, d.y);
      const size_t idx = (size_t)d.x * g.H * g.W + (size_t)(wi < 0 ? 0 : wi);
      if (wi >= 0 && !inf[idx]) { have = true; x = fq_load(X + idx); y = fq_load(Y + idx); }
    }
  }
  e2_jac acc = e2_identity();
  if (have) {
    const uint4 rr = r[(size_t)d.z * n_terms + t];
    acc = e2_mul_affine(x, y, rr.x, rr.y, rr.z, rr.w, 128, a);
  }
  e2_store(&sh[tid], acc);
  __syncthreads();
  for (int wdt = S / 2; wdt >= 1; wdt >>= 1) {  // within the sum's S lanes: j + wdt < S
    if (j < wdt) e2_store(&sh[tid], e2_add(e2_load(&sh[tid]), e2_load(&sh[tid + wdt]), a));
    __syncthreads();
  }
  if (j == 0 && live) e2_store(parts + sum * nblk + blockIdx.x % nblk, e2_load(&sh[tid]));
}

__global__ __launch_bounds__(kE2Block) void e2_negate_kernel(e2_jac* __restrict__ p, const uint8_t* __restrict__ neg, size_t n) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n || !neg[i]) return;
  fq_store(&p[i].Y, fq_neg(fq_load(&p[i].Y)));  // the identity (Z = 0) stays the identity
}

// grid: x = blocks of kBiasBlock output pixels, y = output channel, z = group: the plane's bias is uniform per workgroup.
// out = C + bias with the complete addition: C[t] = bias doubles, bias = -C[t] gives the identity, a flagged operand adds nothing
__global__ __launch_bounds__(kBiasBlock) void e2_bias_add_kernel(const fq* __restrict__ CX, const fq* __restrict__ CY,
                                                               const uint8_t* __restrict__ cinf, const fq* __restrict__ BX,
                                                               const fq* __restrict__ BY, const uint8_t* __restrict__ binf, size_t n_pix,
                                                               fq a, e2_jac* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * kBiasBlock + threadIdx.x, plane = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  if (t >= n_pix) return;
  const size_t i = plane * n_pix + t;
  e2_jac acc = e2_identity();
  if (!binf[plane]) { acc.X = fq_load(BX + plane); acc.Y = fq_load(BY + plane); acc.Z = fq_one(); }
  if (!cinf[i]) acc = e2_add_mixed(acc, fq_load(CX + i), fq_load(CY + i), a);
  e2_store(out + i, acc);
}

}  // namespace

int EncConvDev::add_bias(const E2Points& bias, size_t groups, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  (void)hipSetDevice(c->device);
  const size_t per_plane = g.oh * g.ow, n = groups * n_out * per_plane;
  DevBuf jac(c);
  if (jac.alloc(n * sizeof(e2_jac))) return VPIN_ENOMEM;
  hipLaunchKernelGGL(e2_bias_add_kernel, dim3(blocks_of(per_plane, kBiasBlock), (unsigned)n_out, (unsigned)groups), dim3(kBiasBlock), 0, c->stream,
                     out.X(), out.Y(), out.F(), bias.X(), bias.Y(), bias.F(), per_plane, e2_curve_a(), (e2_jac*)jac.p);
  VPIN_HIP_TRY(hipGetLastError());
  return e2_emit(c, (const e2_jac*)jac.p, n, out_x, out_y, out_inf);
}

int EncConvDev::conv_mc(const ConvGeom& geom, size_t groups, size_t C, size_t n_out, const int32_t* w, const uint8_t* connect,
                        const int32_t* top_bit, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  (void)hipSetDevice(c->device);
  g = geom;
  const size_t taps = g.taps(), per_plane = g.oh * g.ow, n = groups * n_out * per_plane;
  const int slots = (int)(C < (size_t)kMcMaxSlots ? C : (size_t)kMcMaxSlots), lanes = kE2Block / slots < 64 ? kE2Block / slots : 64;
  DevBuf jac(c), wd(c), cn(c), tb(c);
  if (jac.alloc(n * sizeof(e2_jac)) || wd.alloc(n_out * C * taps * 4) || cn.alloc(n_out * C) || tb.alloc(n_out * 4)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(wd.p, w, n_out * C * taps * 4, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(cn.p, connect, n_out * C, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(tb.p, top_bit, n_out * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_convmc_kernel, dim3(blocks_of(per_plane, lanes), (unsigned)n_out, (unsigned)groups), dim3(slots * lanes), 0, c->stream,
                     in.X(), in.Y(), in.F(), e2_geom(g), (int)C, slots, lanes, (const int32_t*)wd.p, (const uint8_t*)cn.p,
                     (const int32_t*)tb.p, e2_curve_a(), (e2_jac*)jac.p);
  VPIN_HIP_TRY(hipGetLastError());
  return e2_emit(c, (const e2_jac*)jac.p, n, out_x, out_y, out_inf, &out);
}

int EncConvDev::rlc_mc(size_t n_pairs, const int32_t* desc, const uint8_t* neg, size_t n_sums, const uint8_t* r_le16, E2Points* sums_out,
                       uint8_t* s_x, uint8_t* s_y, uint8_t* s_inf, int scalar_bits) {
  (void)hipSetDevice(c->device);
  const size_t n_terms = g.oh * g.ow, total = n_pairs * n_terms;
  if (e2_rlc_shared_wins(n_sums / n_pairs, n_terms, scalar_bits)) {  // the sums of a pair share its r: the bucket walk
    DevBuf r(c), ng(c), sums(c);
    if (r.alloc(total * 16) || ng.alloc(n_sums) || sums.alloc(n_sums * sizeof(e2_jac))) return VPIN_ENOMEM;
    VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le16, total * 16, hipMemcpyHostToDevice, c->stream));
    VPIN_HIP_TRY(hipMemcpyAsync(ng.p, neg, n_sums, hipMemcpyHostToDevice, c->stream));
    const int rc = e2_rlc_shared(c, in, out, g, desc, n_sums, n_pairs, r.p, scalar_bits, (e2_jac*)sums.p);
    if (rc) return rc;
    hipLaunchKernelGGL(e2_negate_kernel, dim3(blocks_of(n_sums, kE2Block)), dim3(kE2Block), 0, c->stream, (e2_jac*)sums.p, (const uint8_t*)ng.p,
                       n_sums);
    VPIN_HIP_TRY(hipGetLastError());
    return e2_emit(c, (const e2_jac*)sums.p, n_sums, s_x, s_y, s_inf, sums_out);
  }
  int S = kE2Block;  // lanes per sum
  while (S / 2 >= 1 && (size_t)(S / 2) >= n_terms) S /= 2;
  const size_t nblk = blocks_of(n_terms, S);  // 1 below kE2Block terms
  DevBuf r(c), ds(c), ng(c), parts(c), sums(c);
  if (r.alloc(total * 16) || ds.alloc(n_sums * 16) || ng.alloc(n_sums) || parts.alloc(n_sums * nblk * sizeof(e2_jac)) ||
      sums.alloc(n_sums * sizeof(e2_jac)))
    return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le16, total * 16, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ds.p, desc, n_sums * 16, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ng.p, neg, n_sums, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_rlc_mc_kernel, dim3((unsigned)(blocks_of(n_sums, kE2Block / S) * nblk)), dim3(kE2Block), 0, c->stream, in.X(), in.Y(),
                     in.F(), out.X(), out.Y(), out.F(), e2_geom(g), (const int4*)ds.p, n_sums, (unsigned)nblk, S, n_terms, (const uint4*)r.p,
                     e2_curve_a(), (e2_jac*)parts.p);
  VPIN_HIP_TRY(hipGetLastError());
  const int rc = e2_reduce(c, (const e2_jac*)parts.p, n_sums, nblk, (e2_jac*)sums.p);
  if (rc) return rc;
  hipLaunchKernelGGL(e2_negate_kernel, dim3(blocks_of(n_sums, kE2Block)), dim3(kE2Block), 0, c->stream, (e2_jac*)sums.p, (const uint8_t*)ng.p,
                     n_sums);
  VPIN_HIP_TRY(hipGetLastError());
  return e2_emit(c, (const e2_jac*)sums.p, n_sums, s_x, s_y, s_inf, sums_out);
}

}  // namespace vpin
