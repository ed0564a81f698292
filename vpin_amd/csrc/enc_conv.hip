// enc_conv.hip -- the server side of vPIN's encrypted convolution on the device: the homomorphic convolution over
// exponential-ElGamal ciphertext planes on E2 and the sums of its random-linear-combination check.
//
//   e2_load_kernel       pixel bytes -> Montgomery coordinates; range (< q) and curve-equation checks, one lane per pixel
//   e2_conv_kernel       one lane per output pixel: joint double-and-add over the taps, from the top set bit of the largest
//                        weight down (the weights are launch-wide, so a wave diverges only on padding and identity pixels)
//   e2_to_affine_kernel  Jacobian -> affine, 256 points per workgroup with ONE Fermat inversion: Montgomery's trick as a
//                        product tree in LDS (up-sweep of products, inverse of the root, down-sweep of inverses)
//   e2_rlc_kernel        one lane per (sum, term): 128-step double-and-add of r_t times the term's point (mixed addition:
//                        window pixels and normalised outputs are affine), then an LDS tree with the complete addition
//   e2_reduce_kernel     the second launch: one workgroup per sum over the partials of the first
// Also the plumbing every E2 stage of the library uses (enc_conv.h): E2Points::load around e2_load_kernel, and E2Affine /
// e2_emit around e2_to_affine_kernel, the one place where normalised points are copied to the host.
// Exactness: every addition is complete by case (e2_dev.h), so repeated pixels, P / -P pairs and identities are summed
// correctly.  The accumulators are named registers (e2_jac locals, the scalar as four shifted words): no per-lane arrays.
#include "e2_dev.h"
#include "enc_conv.h"

#include <cstring>
#include <string>
#include <vector>

#include "host/field.h"
#include "host/gadget_ops.h"

namespace vpin {

namespace {

__global__ __launch_bounds__(kE2Block) void e2_load_kernel(const fq* __restrict__ xb, const fq* __restrict__ yb,
                                                           const uint8_t* __restrict__ inf, size_t n, fq a, fq b,
                                                           fq* __restrict__ X, fq* __restrict__ Y, uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  const fq xr = fq_load(xb + i), yr = fq_load(yb + i);
  unsigned bx = 0, by = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    (void)__builtin_subc(xr.v[k], fq_modulus_limb(k), bx, &bx);
    (void)__builtin_subc(yr.v[k], fq_modulus_limb(k), by, &by);
  }
  uint32_t f = (bx && by) ? 0u : kE2FlagRange;  // no borrow: the value is >= q
  const fq x = e2_fqm(xr, e2_fq_r2()), y = e2_fqm(yr, e2_fq_r2());
  if (!f && !inf[i]) {
    const fq lhs = e2_fqm(y, y);
    const fq rhs = fq_add(e2_fqm(fq_add(e2_fqm(x, x), a), x), b);
    if (!fq_eq(lhs, rhs)) f = kE2FlagOffCurve;
  }
  fq_store(X + i, x);
  fq_store(Y + i, y);
  if (f) atomicOr(flags, f);
}

__global__ __launch_bounds__(64) void e2_conv_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                     const uint8_t* __restrict__ inf, E2Geom g,
                                                     const uint32_t* __restrict__ w, int top_bit, fq a,
                                                     e2_jac* __restrict__ out) {
  const int t = (int)(blockIdx.x * 64 + threadIdx.x), n_out = g.oh * g.ow;
  if (t >= n_out) return;
  const size_t plane = blockIdx.y, base = plane * (size_t)g.H * g.W;
  const int taps = g.fh * g.fw;
  e2_jac acc = e2_identity();
  for (int bit = top_bit; bit >= 0; bit--) {
    if (!e2_is_identity(acc)) acc = e2_dbl(acc, a);
    for (int k = 0; k < taps; k++) {
      if (!((w[4 * k + (bit >> 5)] >> (bit & 31)) & 1u)) continue;  // the same for every lane
      const long wi = e2_window_index(g, t, k);
      if (wi < 0 || inf[base + wi]) continue;  // padding and flagged pixels are the identity
      acc = e2_add_mixed(acc, fq_load(X + base + wi), fq_load(Y + base + wi), a);
    }
  }
  e2_store(out + plane * (size_t)n_out + t, acc);
}

// mx, my: Montgomery (for e2_rlc_kernel); cx, cy: canonical little-endian (the caller's bytes); identity: zeros and flag 1
__global__ __launch_bounds__(kE2Block) void e2_to_affine_kernel(const e2_jac* __restrict__ in, size_t n, fq* __restrict__ mx,
                                                                fq* __restrict__ my, fq* __restrict__ cx, fq* __restrict__ cy,
                                                                uint8_t* __restrict__ oinf) {
  __shared__ fq tree[2 * kE2Block];  // node j has children 2j and 2j + 1; the leaves are tree[kE2Block ..]
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kE2Block + tid;
  e2_jac p = e2_identity();
  if (i < n) p = e2_load(in + i);
  const bool idn = e2_is_identity(p);
  fq_store(&tree[kE2Block + tid], idn ? fq_one() : p.Z);
  __syncthreads();
  for (int wdt = kE2Block / 2; wdt >= 1; wdt >>= 1) {
    if (tid < wdt) {
      const int j = wdt + tid;
      fq_store(&tree[j], e2_fqm(fq_load(&tree[2 * j]), fq_load(&tree[2 * j + 1])));
    }
    __syncthreads();
  }
  if (tid == 0) fq_store(&tree[1], e2_fq_inv(fq_load(&tree[1])));
  __syncthreads();
  for (int wdt = 1; wdt <= kE2Block / 2; wdt <<= 1) {
    if (tid < wdt) {
      const int j = wdt + tid;
      const fq pi = fq_load(&tree[j]), l = fq_load(&tree[2 * j]), r = fq_load(&tree[2 * j + 1]);
      fq_store(&tree[2 * j], e2_fqm(pi, r));
      fq_store(&tree[2 * j + 1], e2_fqm(pi, l));
    }
    __syncthreads();
  }
  if (i >= n) return;
  fq x = fq_zero(), y = fq_zero();
  if (!idn) {
    const fq zi = fq_load(&tree[kE2Block + tid]), zi2 = e2_fqm(zi, zi);
    x = e2_fqm(p.X, zi2);
    y = e2_fqm(p.Y, e2_fqm(zi2, zi));
  }
  fq_store(mx + i, x);
  fq_store(my + i, y);
  fq_store(cx + i, fq_from_mont(x));
  fq_store(cy + i, fq_from_mont(y));
  oinf[i] = idn ? 1 : 0;
}

// grid: x = blocks of terms, y = sum (tap k, or taps = the outputs themselves), z = plane
__global__ __launch_bounds__(kE2Block) void e2_rlc_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                          const uint8_t* __restrict__ inf, const fq* __restrict__ OX,
                                                          const fq* __restrict__ OY, const uint8_t* __restrict__ oinf, E2Geom g,
                                                          int taps, size_t n_terms, const uint4* __restrict__ r, fq a,
                                                          e2_jac* __restrict__ parts) {
  __shared__ e2_jac sh[kE2Block];
  const size_t t = (size_t)blockIdx.x * kE2Block + threadIdx.x, plane = blockIdx.z;
  const int s = (int)blockIdx.y;
  bool have = false;
  fq x = fq_zero(), y = fq_zero();
  if (t < n_terms) {
    if (s == taps) {
      const size_t idx = plane * n_terms + t;
      if (!oinf[idx]) { have = true; x = fq_load(OX + idx); y = fq_load(OY + idx); }
    } else {
      const long wi = e2_window_index(g, (int)t, s);
      const size_t idx = plane * (size_t)g.H * g.W + (size_t)(wi < 0 ? 0 : wi);
      if (wi >= 0 && !inf[idx]) { have = true; x = fq_load(X + idx); y = fq_load(Y + idx); }
    }
  }
  e2_jac acc = e2_identity();
  if (have) {
    const uint4 rr = r[plane * n_terms + t];
    acc = e2_mul_affine(x, y, rr.x, rr.y, rr.z, rr.w, 128, a);
  }
  e2_block_tree(sh, acc, a);
  if (threadIdx.x == 0)
    e2_store(parts + ((plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x), e2_load(&sh[0]));
}

// one workgroup per sum: out[b] = sum of parts[b * n_parts ..][0 .. n_parts)
__global__ __launch_bounds__(kE2Block) void e2_reduce_kernel(const e2_jac* __restrict__ parts, size_t n_parts, fq a,
                                                             e2_jac* __restrict__ out) {
  __shared__ e2_jac sh[kE2Block];
  const e2_jac* p = parts + (size_t)blockIdx.x * n_parts;
  e2_jac acc = e2_identity();
  for (size_t i = threadIdx.x; i < n_parts; i += kE2Block) acc = e2_add(acc, e2_load(p + i), a);
  e2_block_tree(sh, acc, a);
  if (threadIdx.x == 0) e2_store(out + blockIdx.x, e2_load(&sh[0]));
}

using vpin_host::Fq;

// the curve coefficient b of E2, little-endian (a: host/gadget_ops.h kAPdBytes)
const uint8_t kE2BBytes[32] = {86, 83, 202, 68, 110, 236, 64, 249, 56, 118, 236, 1, 191, 143, 126, 100,
                               4, 149, 41, 137, 111, 171, 93, 146, 250, 112, 171, 90, 44, 184, 8, 8};

// the sums of e2_rlc_kernel + e2_reduce_kernel: P x (taps + 1) Jacobian triples to the host
int run_rlc(vpin_ctx* c, const fq* X, const fq* Y, const uint8_t* inf, const fq* OX, const fq* OY, const uint8_t* oinf,
            const ConvGeom& g, size_t n_terms, const uint8_t* r_le16, uint8_t* sums_jac) {
  const size_t nsum = g.taps() + 1, nblk = (n_terms + kE2Block - 1) / kE2Block, total = g.P * n_terms;
  DevBuf r(c), parts(c), sums(c);
  if (r.alloc(total * 16) || parts.alloc(g.P * nsum * nblk * sizeof(e2_jac)) || sums.alloc(g.P * nsum * sizeof(e2_jac)))
    return VPIN_ENOMEM;
  const fq a = e2_curve_a();
  VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le16, total * 16, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_rlc_kernel, dim3((unsigned)nblk, (unsigned)nsum, (unsigned)g.P), dim3(kE2Block), 0, c->stream, X, Y, inf, OX, OY,
                     oinf, e2_geom(g), (int)g.taps(), n_terms, (const uint4*)r.p, a, (e2_jac*)parts.p);
  VPIN_HIP_TRY(hipGetLastError());
  const int rc = e2_reduce(c, (const e2_jac*)parts.p, g.P * nsum, nblk, (e2_jac*)sums.p);
  if (rc) return rc;
  VPIN_HIP_TRY(hipMemcpyAsync(sums_jac, sums.p, g.P * nsum * sizeof(e2_jac), hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

}  // namespace

E2Geom e2_geom(const ConvGeom& g) {
  return E2Geom{(int)g.H, (int)g.W, (int)g.fh, (int)g.fw, (int)g.pad, (int)g.stride, (int)g.oh, (int)g.ow};
}

fq fq_of_le32(const uint8_t* le32) {
  Fq t;
  memcpy(t.l, le32, 32);
  t = t * Fq::r2();
  fq r;
  memcpy(r.v, t.l, 32);
  return r;
}

fq e2_curve_a() { return fq_of_le32(vpin_gadgets::kAPdBytes); }

int e2_to_affine(vpin_ctx* c, const e2_jac* in, size_t n, fq* mx, fq* my, fq* cx, fq* cy, uint8_t* oinf) {
  hipLaunchKernelGGL(e2_to_affine_kernel, dim3(blocks_of(n, kE2Block)), dim3(kE2Block), 0, c->stream, in, n, mx, my, cx, cy, oinf);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

int e2_reduce(vpin_ctx* c, const e2_jac* parts, size_t n_sums, size_t n_parts, e2_jac* out) {
  hipLaunchKernelGGL(e2_reduce_kernel, dim3((unsigned)n_sums), dim3(kE2Block), 0, c->stream, parts, n_parts, e2_curve_a(), out);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

int E2Points::resize(size_t count) {
  n = count;
  VPIN_EC_ALLOC(x, n * 32);
  VPIN_EC_ALLOC(y, n * 32);
  VPIN_EC_ALLOC(inf, n);
  return VPIN_OK;
}

int E2Points::load(vpin_ctx* c, const uint8_t* bx, const uint8_t* by, const uint8_t* binf, size_t count, const char* who, const char* what) {
  (void)hipSetDevice(c->device);
  DevBuf rx(c), ry(c), fl(c);
  if (rx.alloc(count * 32) || ry.alloc(count * 32) || fl.alloc(16)) return VPIN_ENOMEM;
  const int rc = resize(count);
  if (rc) return rc;
  uint32_t flags = 0;
  VPIN_HIP_TRY(hipMemcpyAsync(rx.p, bx, n * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ry.p, by, n * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(inf.p, binf, n, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemsetAsync(fl.p, 0, 4, c->stream));
  hipLaunchKernelGGL(e2_load_kernel, dim3(blocks_of(n, kE2Block)), dim3(kE2Block), 0, c->stream, (const fq*)rx.p, (const fq*)ry.p, F(), n,
                     e2_curve_a(), fq_of_le32(kE2BBytes), (fq*)x.p, (fq*)y.p, (uint32_t*)fl.p);
  VPIN_HIP_TRY(hipGetLastError());
  VPIN_HIP_TRY(hipMemcpyAsync(&flags, fl.p, 4, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  if (flags & kE2FlagRange) return enc::fail(VPIN_EINVAL, (std::string(who) + ": a coordinate is not below q").c_str());
  if (flags & kE2FlagOffCurve) return enc::fail(VPIN_EINVAL, (std::string(who) + ": a " + what + " is not on the curve E2").c_str());
  return VPIN_OK;
}

int E2Affine::normalise(vpin_ctx* c, const e2_jac* jac, size_t n, E2Points* keep) {
  if (cx.alloc(n * 32) || cy.alloc(n * 32)) return VPIN_ENOMEM;
  if (keep) {
    const int rc = keep->resize(n);
    if (rc) return rc;
  } else if (mx.alloc(n * 32) || my.alloc(n * 32) || fl.alloc(n)) {
    return VPIN_ENOMEM;
  }
  flags = keep ? keep->F() : (const uint8_t*)fl.p;
  return e2_to_affine(c, jac, n, (fq*)(keep ? keep->x.p : mx.p), (fq*)(keep ? keep->y.p : my.p), (fq*)cx.p, (fq*)cy.p, (uint8_t*)flags);
}

int E2Affine::copy_out(vpin_ctx* c, size_t first, size_t count, uint8_t* ox, uint8_t* oy, uint8_t* oinf) const {
  VPIN_HIP_TRY(hipMemcpyAsync(ox, (const uint8_t*)cx.p + first * 32, count * 32, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(oy, (const uint8_t*)cy.p + first * 32, count * 32, hipMemcpyDeviceToHost, c->stream));
  if (oinf) VPIN_HIP_TRY(hipMemcpyAsync(oinf, flags + first, count, hipMemcpyDeviceToHost, c->stream));
  return VPIN_OK;
}

int e2_emit(vpin_ctx* c, const e2_jac* jac, size_t n, uint8_t* ox, uint8_t* oy, uint8_t* oinf, E2Points* keep) {
  E2Affine aff(c);
  int rc = aff.normalise(c, jac, n, keep);
  if (!rc) rc = aff.copy_out(c, 0, n, ox, oy, oinf);
  if (rc) return rc;
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

int EncConvDev::conv(const ConvGeom& geom, const uint8_t* filter_le16, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  (void)hipSetDevice(c->device);
  g = geom;
  const size_t taps = g.taps(), n_out = g.outputs(), per_plane = g.oh * g.ow;
  int top_bit = -1;
  for (size_t k = 0; k < taps; k++)
    for (int b = 127; b > top_bit; b--)
      if ((filter_le16[16 * k + (b >> 3)] >> (b & 7)) & 1) { top_bit = b; break; }
  DevBuf jac(c), filt(c);
  if (jac.alloc(n_out * sizeof(e2_jac)) || filt.alloc(taps * 16)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(filt.p, filter_le16, taps * 16, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_conv_kernel, dim3(blocks_of(per_plane, 64), (unsigned)g.P), dim3(64), 0, c->stream, in.X(), in.Y(), in.F(),
                     e2_geom(g), (const uint32_t*)filt.p, top_bit, e2_curve_a(), (e2_jac*)jac.p);
  VPIN_HIP_TRY(hipGetLastError());
  return e2_emit(c, (const e2_jac*)jac.p, n_out, out_x, out_y, out_inf, &out);
}

int EncConvDev::rlc(const uint8_t* r_le16, uint8_t* sums_jac, int scalar_bits) {
  (void)hipSetDevice(c->device);
  const size_t nsum = g.taps() + 1, n_terms = g.oh * g.ow, n = g.P * nsum;
  if (e2_rlc_shared_wins(nsum, n_terms, scalar_bits)) {  // the taps + 1 sums of a plane share its r: the bucket walk
    std::vector<int32_t> desc(4 * n, 0);  // as rlc_mc's: {plane, tap, pair, 0}, the last sum of a plane over its outputs
    for (size_t p = 0; p < g.P; p++)
      for (size_t k = 0; k < nsum; k++) {
        int32_t* d = &desc[4 * (p * nsum + k)];
        d[0] = k < g.taps() ? (int32_t)p : -1; d[1] = (int32_t)k; d[2] = (int32_t)p;
      }
    DevBuf r(c), sums(c);
    if (r.alloc(g.P * n_terms * 16) || sums.alloc(n * sizeof(e2_jac))) return VPIN_ENOMEM;
    VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le16, g.P * n_terms * 16, hipMemcpyHostToDevice, c->stream));
    const int rc = e2_rlc_shared(c, in, out, g, desc.data(), n, g.P, r.p, scalar_bits, (e2_jac*)sums.p);
    if (rc) return rc;
    VPIN_HIP_TRY(hipMemcpyAsync(sums_jac, sums.p, n * sizeof(e2_jac), hipMemcpyDeviceToHost, c->stream));
    VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
    return VPIN_OK;
  }
  return run_rlc(c, in.X(), in.Y(), in.F(), out.X(), out.Y(), out.F(), g, g.oh * g.ow, r_le16, sums_jac);
}

int EncConvDev::msm(const uint8_t* r_le16, size_t n, uint8_t sum_jac[96]) {
  (void)hipSetDevice(c->device);
  ConvGeom one;  // no taps: the single sum runs over the loaded points themselves
  return run_rlc(c, nullptr, nullptr, nullptr, in.X(), in.Y(), in.F(), one, n, r_le16, sum_jac);
}

}  // namespace vpin
