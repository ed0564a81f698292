// e2_dev.h -- device-side arithmetic on the curve E2: y^2 = x^3 + a x + b over F_q (the curve of vPIN's
// exponential-ElGamal ciphertexts; a is the gadget's public input, host/gadget_ops.h kAPdBytes).
//
// Points are Jacobian (X : Y : Z), x = X / Z^2, y = Y / Z^3, over fq_dev.h's Montgomery field; Z == 0 is the identity.
// The additions are complete BY CASE: an identity operand, P == Q (falls to the doubling) and P == -Q (the identity)
// are recognised from H = U2 - U1 and R = S2 - S1, so sums over arbitrary ciphertext planes (repeated pixels, P and -P,
// flagged identities) are exact.  The field product is called, not inlined: a point operation is 10-16 products, and
// the kernels of enc_conv.hip chain hundreds of them.
#pragma once
#include "fq_dev.h"

namespace vpin {

struct e2_jac {
  fq X, Y, Z;
};

static __device__ __noinline__ fq e2_fqm(fq a, fq b) { return fq_mul(a, b); }

__device__ __forceinline__ e2_jac e2_identity() {
  e2_jac r;
  r.X = fq_zero(); r.Y = fq_one(); r.Z = fq_zero();
  return r;
}

__device__ __forceinline__ bool e2_is_identity(const e2_jac& p) { return fq_is_zero(p.Z); }

// R^2 mod q: raw integer -> Montgomery form by one product
__device__ __forceinline__ fq e2_fq_r2() {
  fq r;
  r.v[0] = 0x449c0f01u; r.v[1] = 0xa40611e3u; r.v[2] = 0x68859347u; r.v[3] = 0xd00e1ba7u;
  r.v[4] = 0x17f5be65u; r.v[5] = 0xceec73d2u; r.v[6] = 0x7c309a3du; r.v[7] = 0x0399411bu;
  return r;
}

// limb i of q - 2
__device__ __forceinline__ constexpr uint32_t e2_qm2_limb(int i) { return i == 0 ? VPIN_Q0 - 2u : fq_modulus_limb(i); }

// a^(q-2), plain square-and-multiply from the top bit (bit 252) down: no per-lane table
__device__ __noinline__ fq e2_fq_inv(fq a) {
  fq acc = a;
#pragma unroll
  for (int w = 7; w >= 0; w--) {
    const uint32_t e = e2_qm2_limb(w);
#pragma nounroll
    for (int b = (w == 7 ? 27 : 31); b >= 0; b--) {
      acc = e2_fqm(acc, acc);
      if ((e >> b) & 1u) acc = e2_fqm(acc, a);
    }
  }
  return acc;
}

// 2P for any a (dbl-2007-bl without the a = -3 / a = 0 shortcuts).  Z = 0 stays Z = 0; Y = 0 gives Z = 0.
__device__ __forceinline__ e2_jac e2_dbl(const e2_jac& p, const fq& a) {
  const fq XX = e2_fqm(p.X, p.X), YY = e2_fqm(p.Y, p.Y), YYYY = e2_fqm(YY, YY), ZZ = e2_fqm(p.Z, p.Z);
  const fq S = fq_dbl(fq_dbl(e2_fqm(p.X, YY)));
  const fq M = fq_add(fq_add(fq_dbl(XX), XX), e2_fqm(a, e2_fqm(ZZ, ZZ)));
  e2_jac r;
  r.X = fq_sub(e2_fqm(M, M), fq_dbl(S));
  r.Y = fq_sub(e2_fqm(M, fq_sub(S, r.X)), fq_dbl(fq_dbl(fq_dbl(YYYY))));
  r.Z = fq_dbl(e2_fqm(p.Y, p.Z));
  return r;
}

// P + (x2, y2), the second operand affine and not the identity
__device__ __forceinline__ e2_jac e2_add_mixed(const e2_jac& p, const fq& x2, const fq& y2, const fq& a) {
  if (e2_is_identity(p)) {
    e2_jac r;
    r.X = x2; r.Y = y2; r.Z = fq_one();
    return r;
  }
  const fq Z1Z1 = e2_fqm(p.Z, p.Z), U2 = e2_fqm(x2, Z1Z1), S2 = e2_fqm(y2, e2_fqm(p.Z, Z1Z1));
  const fq H = fq_sub(U2, p.X), R = fq_sub(S2, p.Y);
  if (fq_is_zero(H)) return fq_is_zero(R) ? e2_dbl(p, a) : e2_identity();
  const fq HH = e2_fqm(H, H), HHH = e2_fqm(H, HH), V = e2_fqm(p.X, HH);
  e2_jac r;
  r.X = fq_sub(fq_sub(e2_fqm(R, R), HHH), fq_dbl(V));
  r.Y = fq_sub(e2_fqm(R, fq_sub(V, r.X)), e2_fqm(p.Y, HHH));
  r.Z = e2_fqm(p.Z, H);
  return r;
}

// P + Q, both Jacobian
__device__ __forceinline__ e2_jac e2_add(const e2_jac& p, const e2_jac& q, const fq& a) {
  if (e2_is_identity(p)) return q;
  if (e2_is_identity(q)) return p;
  const fq Z1Z1 = e2_fqm(p.Z, p.Z), Z2Z2 = e2_fqm(q.Z, q.Z);
  const fq U1 = e2_fqm(p.X, Z2Z2), U2 = e2_fqm(q.X, Z1Z1);
  const fq S1 = e2_fqm(p.Y, e2_fqm(q.Z, Z2Z2)), S2 = e2_fqm(q.Y, e2_fqm(p.Z, Z1Z1));
  const fq H = fq_sub(U2, U1), R = fq_sub(S2, S1);
  if (fq_is_zero(H)) return fq_is_zero(R) ? e2_dbl(p, a) : e2_identity();
  const fq HH = e2_fqm(H, H), HHH = e2_fqm(H, HH), V = e2_fqm(U1, HH);
  e2_jac r;
  r.X = fq_sub(fq_sub(e2_fqm(R, R), HHH), fq_dbl(V));
  r.Y = fq_sub(e2_fqm(R, fq_sub(V, r.X)), e2_fqm(S1, HHH));
  r.Z = e2_fqm(e2_fqm(p.Z, q.Z), H);
  return r;
}

__device__ __forceinline__ e2_jac e2_load(const e2_jac* __restrict__ p) {
  e2_jac r;
  r.X = fq_load(&p->X); r.Y = fq_load(&p->Y); r.Z = fq_load(&p->Z);
  return r;
}

__device__ __forceinline__ void e2_store(e2_jac* __restrict__ p, const e2_jac& v) {
  fq_store(&p->X, v.X); fq_store(&p->Y, v.Y); fq_store(&p->Z, v.Z);
}

// ---- shared by the kernels of enc_conv.hip and enc_fc.hip ------------------------------------------------------------

// s * (x, y) for an affine point that is not the identity: double-and-add from the top set bit down.  The scalar is the nb-bit
// number at the top of r3:r2:r1:r0 (a u128: nb = 128; a u32 passed as r3: nb = 32), kept as four shifted words
__device__ __forceinline__ e2_jac e2_mul_affine(const fq& x, const fq& y, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, int nb,
                                                const fq& a) {
  e2_jac acc = e2_identity();
  if (r0 | r1 | r2 | r3) {
#define VPIN_E2_SHL1() do { r3 = (r3 << 1) | (r2 >> 31); r2 = (r2 << 1) | (r1 >> 31); r1 = (r1 << 1) | (r0 >> 31); r0 <<= 1; nb--; } while (0)
    while (!(r3 >> 31)) VPIN_E2_SHL1();
    acc.X = x; acc.Y = y; acc.Z = fq_one();  // the top set bit
    VPIN_E2_SHL1();
    for (; nb > 0;) {
      acc = e2_dbl(acc, a);
      if (r3 >> 31) acc = e2_add_mixed(acc, x, y, a);
      VPIN_E2_SHL1();
    }
#undef VPIN_E2_SHL1
  }
  return acc;
}

// s * (x, y) for a scalar of up to 256 bits (the ElGamal key, a scalar mod the group order): e2_mul_affine's walk with eight
// shifted words.  A function of its own, so that the 128-bit kernels keep their four scalar registers
struct e2_scalar256 {
  uint32_t w0, w1, w2, w3, w4, w5, w6, w7;
};

__device__ __forceinline__ e2_scalar256 e2_scalar256_load(const uint32_t* __restrict__ p) {
  const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
  return e2_scalar256{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

__device__ __forceinline__ bool e2_scalar256_is_zero(const e2_scalar256& s) {
  return !(s.w0 | s.w1 | s.w2 | s.w3 | s.w4 | s.w5 | s.w6 | s.w7);
}

__device__ __forceinline__ e2_jac e2_mul_affine256(const fq& x, const fq& y, e2_scalar256 s, const fq& a) {
  e2_jac acc = e2_identity();
  if (!e2_scalar256_is_zero(s)) {
    int nb = 256;
#define VPIN_E2_SHL1() do { s.w7 = (s.w7 << 1) | (s.w6 >> 31); s.w6 = (s.w6 << 1) | (s.w5 >> 31); s.w5 = (s.w5 << 1) | (s.w4 >> 31); \
                            s.w4 = (s.w4 << 1) | (s.w3 >> 31); s.w3 = (s.w3 << 1) | (s.w2 >> 31); s.w2 = (s.w2 << 1) | (s.w1 >> 31); \
                            s.w1 = (s.w1 << 1) | (s.w0 >> 31); s.w0 <<= 1; nb--; } while (0)
    while (!(s.w7 >> 31)) VPIN_E2_SHL1();
    acc.X = x; acc.Y = y; acc.Z = fq_one();  // the top set bit
    VPIN_E2_SHL1();
    for (; nb > 0;) {
      acc = e2_dbl(acc, a);
      if (s.w7 >> 31) acc = e2_add_mixed(acc, x, y, a);
      VPIN_E2_SHL1();
    }
#undef VPIN_E2_SHL1
  }
  return acc;
}

// s * B from B's window table (e2_client.hip): entry k * (2^w - 1) + d - 1 is the affine point d * 2^(w k) * B, so the
// product is one mixed addition per non-zero digit and no doubling.  Stops when the remaining digits are zero; the additions
// are complete, so a small scalar that lands on acc == +-entry is exact
__device__ __forceinline__ e2_jac e2_mul_base(const fq* __restrict__ tx, const fq* __restrict__ ty, int w, e2_scalar256 s, const fq& a) {
  e2_jac acc = e2_identity();
  const uint32_t mask = (1u << w) - 1u;
  const int up = 32 - w;
  for (uint32_t row = 0; !e2_scalar256_is_zero(s); row += mask) {
    const uint32_t d = s.w0 & mask;
    if (d) acc = e2_add_mixed(acc, fq_load(tx + row + d - 1), fq_load(ty + row + d - 1), a);
    s.w0 = (s.w0 >> w) | (s.w1 << up); s.w1 = (s.w1 >> w) | (s.w2 << up); s.w2 = (s.w2 >> w) | (s.w3 << up);
    s.w3 = (s.w3 >> w) | (s.w4 << up); s.w4 = (s.w4 >> w) | (s.w5 << up); s.w5 = (s.w5 >> w) | (s.w6 << up);
    s.w6 = (s.w6 >> w) | (s.w7 << up); s.w7 >>= w;
  }
  return acc;
}

constexpr int kE2Block = 256;

// 1 / v for every lane of a workgroup of kE2Block with ONE Fermat inversion: Montgomery's trick as the product tree of
// e2_to_affine_kernel (up-sweep of products, inverse of the root, down-sweep).  v must not be zero; tree: 2 * kE2Block elements
// of LDS.  Every lane of the workgroup calls it
__device__ __forceinline__ fq e2_block_inverse(fq* tree, const fq& v) {
  const int tid = threadIdx.x;
  fq_store(&tree[kE2Block + tid], v);
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
  const fq inv = fq_load(&tree[kE2Block + tid]);
  __syncthreads();  // the next call overwrites the leaves
  return inv;
}

// sum of the workgroup's kE2Block points into sh[0]
__device__ __forceinline__ void e2_block_tree(e2_jac* sh, const e2_jac& mine, const fq& a) {
  const int tid = threadIdx.x;
  e2_store(&sh[tid], mine);
  __syncthreads();
  for (int wdt = kE2Block / 2; wdt >= 1; wdt >>= 1) {
    if (tid < wdt) e2_store(&sh[tid], e2_add(e2_load(&sh[tid]), e2_load(&sh[tid + wdt]), a));
    __syncthreads();
  }
}

struct E2Geom {
  int H, W, fh, fw, pad, stride, oh, ow;
};

// index of tap k of output t's window inside its plane, or -1 in the padding
__device__ __forceinline__ long e2_window_index(const E2Geom& g, int t, int k) {
  const int i = t / g.ow, j = t % g.ow, ii = k / g.fw, jj = k % g.fw;
  const int r = i * g.stride + ii - g.pad, c = j * g.stride + jj - g.pad;
  if (r < 0 || r >= g.H || c < 0 || c >= g.W) return -1;
  return (long)r * g.W + c;
}

}  // namespace vpin
