// e2_client.hip -- the client side of vPIN's exponential ElGamal on E2 on the device (driven by e2_client.cpp): fixed-base
// multiplication from a window table, batched encryption, the 252-bit variable-base multiplication of decryption, and the
// discrete logarithm of small messages by baby steps / giant steps with the baby-step table resident in HBM.
//
//   e2_base_rows_kernel    window table of a base point B: lane k doubles B w k times and adds along the digits d = 1 .. 2^w - 1
//   e2_base_mul_kernel     s_i * B, one lane per scalar: a mixed addition per non-zero digit, no doubling; optional negation
//   e2_add_pairs_kernel    A_i + B_i, complete (the last addition of a ciphertext's c2)
//   e2_mul256_kernel       s_i * P_i (or one s for all): double-and-add over eight shifted words
//   e2_mul_keyed_kernel    s_i * H[key_of[i]] over a few resident points H: the r * H of an encryption under a key per element
//   e2_sub_kernel          C_i - T_i, complete (M = c2 - sk * c1)
//   e2_dlog_steps_kernel   baby steps: lane l starts at (j0 + l * chunk) * G from G's window table and steps by + G
//   e2_dlog_insert_kernel  parity of y and the open-addressing index keyed on x (64-bit compare-and-swap)
//   e2_dlog_walk_kernel    the walkers P - i D and P + i D in AFFINE coordinates: the 256 lanes of a workgroup share one
//                          inversion per step (e2_block_inverse); every step is looked up by x and confirmed on the stored
//                          coordinates.  A point has up to 64 lanes, which take the giant steps in turn (the step's latency
//                          is that one inversion, so a walk is as long as its deepest lane)
//   e2_act_kernel          the client's activation between the walk and the next encryption: ReLU and the reference's
//                          `shifting`, which goes through float32, one lane per element
//   e2_act_pool_kernel     the same behind a maximum over k x k windows: one lane per output element (vpin_e2_client_round_pool)
// Points come in through E2Points::load and results go out through E2Affine / e2_emit (enc_conv.h): e2_to_affine_kernel
// normalises every output and the baby steps.  As in the layers' kernels the accumulators
// are named registers: no per-lane arrays.
#include "e2_dev.h"
#include "e2_client.h"
#include "enc_conv.h"

#include <cstring>
#include <new>
#include <vector>

namespace vpin {

namespace {

constexpr int kStepsBlock = 64;       // lanes of a workgroup of e2_dlog_steps_kernel
constexpr int kStepsChunk = 64;       // baby steps one lane takes
constexpr size_t kTile = (size_t)1 << 20;  // baby steps normalised and inserted at a time: bounds the Jacobian scratch (96 MiB)

// grid: one workgroup of 64; lane k < nwin writes the 2^w - 1 entries of window k, Jacobian
__global__ __launch_bounds__(64) void e2_base_rows_kernel(fq bx, fq by, int w, int nwin, fq a, e2_jac* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= nwin) return;
  e2_jac p;
  p.X = bx; p.Y = by; p.Z = fq_one();
  for (int i = 0; i < k * w; i++) p = e2_dbl(p, a);
  const size_t m = ((size_t)1 << w) - 1;
  e2_jac acc = p;
  for (size_t d = 0; d < m; d++) {
    e2_store(out + (size_t)k * m + d, acc);
    acc = e2_add(acc, p, a);
  }
}

__global__ __launch_bounds__(kE2Block) void e2_base_mul_kernel(const fq* __restrict__ tx, const fq* __restrict__ ty, int w,
                                                               const uint32_t* __restrict__ s, const uint8_t* __restrict__ neg, size_t n,
                                                               fq a, e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  e2_jac acc = e2_mul_base(tx, ty, w, e2_scalar256_load(s + 8 * i), a);
  if (neg && neg[i]) acc.Y = fq_neg(acc.Y);
  e2_store(out + i, acc);
}

__global__ __launch_bounds__(kE2Block) void e2_add_pairs_kernel(const e2_jac* __restrict__ A, const e2_jac* __restrict__ B, size_t n, fq a,
                                                                e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  e2_store(out + i, e2_add(e2_load(A + i), e2_load(B + i), a));
}

// stride = 8: a scalar per point; stride = 0: one scalar for all
__global__ __launch_bounds__(kE2Block) void e2_mul256_kernel(const fq* __restrict__ X, const fq* __restrict__ Y, const uint8_t* __restrict__ inf,
                                                             const uint32_t* __restrict__ s, size_t stride, size_t n, fq a,
                                                             e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  e2_jac acc = e2_identity();
  if (!inf[i]) acc = e2_mul_affine256(fq_load(X + i), fq_load(Y + i), e2_scalar256_load(s + stride * i), a);
  e2_store(out + i, acc);
}

// out_i = s_i * (HX, HY)[key_of[i]]: every key_of[i] indexes a loaded point that is not the identity (checked by the host)
__global__ __launch_bounds__(kE2Block) void e2_mul_keyed_kernel(const fq* __restrict__ HX, const fq* __restrict__ HY,
                                                                const uint32_t* __restrict__ key_of, const uint32_t* __restrict__ s, size_t n, fq a,
                                                                e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = key_of[i];
  e2_store(out + i, e2_mul_affine256(fq_load(HX + k), fq_load(HY + k), e2_scalar256_load(s + 8 * i), a));
}

// out_i = (X_i, Y_i) - T_i
__global__ __launch_bounds__(kE2Block) void e2_sub_kernel(const e2_jac* __restrict__ T, const fq* __restrict__ X, const fq* __restrict__ Y,
                                                          const uint8_t* __restrict__ inf, size_t n, fq a, e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  e2_jac t = e2_load(T + i);
  t.Y = fq_neg(t.Y);
  if (!inf[i]) t = e2_add_mixed(t, fq_load(X + i), fq_load(Y + i), a);
  e2_store(out + i, t);
}

// out[l * kStepsChunk + t] = (j0 + l * kStepsChunk + t) * G for the n_lanes lanes of one tile
__global__ __launch_bounds__(kStepsBlock) void e2_dlog_steps_kernel(const fq* __restrict__ gtx, const fq* __restrict__ gty, int w, uint64_t j0,
                                                                    size_t n_lanes, fq gx, fq gy, fq a, e2_jac* __restrict__ out) {
  const size_t l = (size_t)blockIdx.x * kStepsBlock + threadIdx.x;
  if (l >= n_lanes) return;
  const uint64_t j = j0 + l * kStepsChunk;
  e2_jac acc = e2_mul_base(gtx, gty, w, e2_scalar256{(uint32_t)j, (uint32_t)(j >> 32), 0u, 0u, 0u, 0u, 0u, 0u}, a);
  for (int t = 0; t < kStepsChunk; t++) {
    e2_store(out + l * kStepsChunk + t, acc);
    acc = e2_add_mixed(acc, gx, gy, a);
  }
}

__device__ __forceinline__ uint64_t dlog_slot(const fq& x, uint64_t mask) {
  return (((uint64_t)(x.v[1] * 0x9e3779b1u) << 32) | x.v[0]) & mask;  // Montgomery limbs of an x coordinate: already spread
}
__device__ __forceinline__ uint32_t dlog_tag(const fq& x) { return x.v[2]; }

// entries j0 .. j0 + count of the table (their x is in place): parity of y from the tile's canonical y, and the index
__global__ __launch_bounds__(kE2Block) void e2_dlog_insert_kernel(const fq* __restrict__ tx, const fq* __restrict__ cy, uint64_t j0, size_t count,
                                                                  uint8_t* __restrict__ par, unsigned long long* __restrict__ idx,
                                                                  uint64_t mask) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= count) return;
  const uint64_t j = j0 + i;
  if (j == 0) return;  // the identity: a case of the walk, not an entry
  par[j] = (uint8_t)(cy[i].v[0] & 1u);
  const fq x = fq_load(tx + j);
  const unsigned long long e = ((unsigned long long)dlog_tag(x) << 32) | j;
  for (uint64_t slot = dlog_slot(x, mask);; slot = (slot + 1) & mask)  // load factor <= 1/2: an empty slot exists
    if (atomicCAS(idx + slot, 0ull, e) == 0ull) break;
}

// (x, y) == +- j * G for a stored j?  *j_out = +j or -j.  A tag match is confirmed on the full x; the sign is the parity of y
__device__ __forceinline__ bool dlog_lookup(const fq& x, const fq& y, bool idn, const fq* __restrict__ tx, const uint8_t* __restrict__ par,
                                            const unsigned long long* __restrict__ idx, uint64_t mask, long long* j_out) {
  if (idn) { *j_out = 0; return true; }
  const uint32_t tag = dlog_tag(x);
  for (uint64_t slot = dlog_slot(x, mask);; slot = (slot + 1) & mask) {
    const unsigned long long e = idx[slot];
    if (!e) return false;
    if ((uint32_t)(e >> 32) != tag) continue;
    const uint64_t j = e & 0xffffffffull;
    if (!fq_eq(fq_load(tx + j), x)) continue;
    const uint32_t p = fq_from_mont(y).v[0] & 1u;
    *j_out = p == par[j] ? (long long)j : -(long long)j;
    return true;
  }
}

// One affine step W += (ex, ey), split around the shared inversion.  By case, never a division by zero:
//   0  W is the identity: the sum is (ex, ey)            2  W == (ex, ey): the doubling, lambda = (3 x^2 + a) / (2 y)
//   1  the chord, lambda = (ey - y) / (ex - x)           3  W == -(ex, ey): the sum is the identity
struct e2_walker {
  fq x, y;
  bool idn;
};

__device__ __forceinline__ int walk_prepare(const e2_walker& W, const fq& ex, const fq& ey, const fq& a, fq* num, fq* den) {
  *den = fq_one();
  *num = fq_zero();
  if (W.idn) return 0;
  if (fq_eq(W.x, ex)) {
    if (!fq_eq(W.y, ey)) return 3;
    const fq xx = e2_fqm(W.x, W.x);
    *num = fq_add(fq_add(fq_dbl(xx), xx), a);
    *den = fq_dbl(W.y);  // not zero: the group has odd order
    return 2;
  }
  *num = fq_sub(ey, W.y);
  *den = fq_sub(ex, W.x);
  return 1;
}

__device__ __forceinline__ void walk_apply(e2_walker& W, const fq& ex, const fq& ey, int kase, const fq& num, const fq& inv_den) {
  if (kase == 0) { W.x = ex; W.y = ey; W.idn = false; return; }
  if (kase == 3) { W.idn = true; return; }
  const fq lam = e2_fqm(num, inv_den);
  const fq x3 = fq_sub(fq_sub(e2_fqm(lam, lam), W.x), ex);
  W.y = fq_sub(e2_fqm(lam, fq_sub(W.x, x3)), W.y);
  W.x = x3;
}

// v_out[i] = the v with P_i = v * G, |v| <= max_giant * nb + nb - 1.  Giant step i looks up Wm = P - i D (v = i nb +- j) and
// Wp = P + i D (v = -i nb +- j), D = nb G.  A point has L = 2^lpp_log lanes of one workgroup: lane l starts at P -+ l D (one
// shared inversion, l D from the table's multiples dmx / dmy) and visits i = l, l + L, l + 2 L, .. by strides of L D, so the
// walk is max_giant / L shared inversions deep.  The value is unique in range, so whichever lane meets it writes it (the
// outputs are zeroed before the launch).  Lanes that are done keep feeding a one into the shared inversion until the
// workgroup votes that all are
__global__ __launch_bounds__(kE2Block) void e2_dlog_walk_kernel(const fq* __restrict__ X, const fq* __restrict__ Y, const uint8_t* __restrict__ inf,
                                                                size_t n, const fq* __restrict__ tx, const uint8_t* __restrict__ par,
                                                                const unsigned long long* __restrict__ idx, uint64_t mask, uint64_t nb,
                                                                const fq* __restrict__ dmx, const fq* __restrict__ dmy, int lpp_log,
                                                                uint64_t max_giant, fq a, long long* __restrict__ v_out,
                                                                uint8_t* __restrict__ found_out) {
  __shared__ fq tree[2 * kE2Block];
  __shared__ int pt_done[kE2Block];  // per point of this workgroup: a lane has met the value
  const int tid = threadIdx.x, lanes = 1 << lpp_log, pt = tid >> lpp_log;
  const size_t g = (size_t)blockIdx.x * kE2Block + tid, i = g >> lpp_log;
  uint64_t step = g & (uint64_t)(lanes - 1);  // the giant step this lane is at
  pt_done[tid] = 0;
  bool done = i >= n || step > max_giant;
  long long j = 0;
  e2_walker Wm, Wp;
  Wm.x = fq_zero(); Wm.y = fq_zero(); Wm.idn = true;
  if (!done) { Wm.x = fq_load(X + i); Wm.y = fq_load(Y + i); Wm.idn = inf[i] != 0; }
  Wp = Wm;
  fq num_m, den_m, num_p, den_p;
  int km, kp;
  // (ex, ey): what this lane adds to Wp and, negated, to Wm: first its offset l D, then the stride L D
  fq ex = fq_load(dmx + (step ? step - 1 : 0)), ey = fq_load(dmy + (step ? step - 1 : 0));
  bool first = true;
  for (;;) {
    const bool move = !done && (!first || step != 0);  // lane 0 starts on P itself
    num_m = fq_zero(); den_m = fq_one(); num_p = fq_zero(); den_p = fq_one();
    km = kp = 0;
    if (move) {
      km = walk_prepare(Wm, ex, fq_neg(ey), a, &num_m, &den_m);
      kp = walk_prepare(Wp, ex, ey, a, &num_p, &den_p);
    }
    const fq inv = e2_block_inverse(tree, e2_fqm(den_m, den_p));
    if (move) {
      walk_apply(Wm, ex, fq_neg(ey), km, num_m, e2_fqm(inv, den_p));
      walk_apply(Wp, ex, ey, kp, num_p, e2_fqm(inv, den_m));
    }
    if (!done) {
      const long long far = (long long)(step * nb);
      bool hit = dlog_lookup(Wm.x, Wm.y, Wm.idn, tx, par, idx, mask, &j);
      long long v = far + j;
      if (!hit && step != 0) {
        hit = dlog_lookup(Wp.x, Wp.y, Wp.idn, tx, par, idx, mask, &j);
        v = j - far;
      }
      if (hit) { v_out[i] = v; found_out[i] = 1; pt_done[pt] = 1; }
      step += (uint64_t)lanes;
      if (first) { ex = fq_load(dmx + lanes - 1); ey = fq_load(dmy + lanes - 1); }
    }
    first = false;
    __syncthreads();
    done = done || pt_done[pt] != 0 || step > max_giant;
    if (__syncthreads_and(done)) break;
  }
}

// The client's activation (src/LeNet/Client.py relu :278-283, shifting :285-289) on the walk's value v, then the message of
// the next encryption as cl::encrypt takes it: the magnitude as a 32-byte scalar and a sign byte.  shifting(v, bits) is
// (float32(v) / 2^bits * 2^16).astype(int32): v rounded to nearest-even into float32, an exact power-of-two scale, truncation
// toward zero.  An integer shift of v is NOT the same number (the rounding into 24 bits of mantissa comes first and can carry).
// bad[i]: kActNotFound when the walk met no value, kActRange when the shifted value does not fit int32 (numpy's result is
// undefined there) or the message is not below 2^62 in magnitude
constexpr uint8_t kActNotFound = 1, kActRange = 2;

// everything after the value a to activate is known, for e2_act_kernel and e2_act_pool_kernel alike: ReLU, the shift, the range
// check, and the message (magnitude and sign) of output element i.  b: kActNotFound or 0 as the caller found it.  The ONE copy of
// the float32 rule
__device__ __forceinline__ void act_emit(long long a, uint8_t b, size_t i, int relu, int shift_bits, uint32_t* __restrict__ m,
                                         uint8_t* __restrict__ neg, long long* __restrict__ act, uint8_t* __restrict__ bad) {
  if (relu && a < 0) a = 0;
  if (shift_bits) {
    const float s = truncf(ldexpf(__ll2float_rn(a), 16 - shift_bits));  // |a| < 2^63, 16 - bits >= -47: the scale is exact
    if (s >= 2147483648.0f || s < -2147483648.0f) { b |= kActRange; a = 0; }
    else a = (long long)s;
  }
  const unsigned long long mag = a < 0 ? 0ull - (unsigned long long)a : (unsigned long long)a;
  if (mag >= (1ull << 62)) b |= kActRange;
  if (b) a = 0;
  const unsigned long long mg = b ? 0ull : mag;
  uint4* mo = reinterpret_cast<uint4*>(m + 8 * i);
  mo[0] = make_uint4((uint32_t)mg, (uint32_t)(mg >> 32), 0u, 0u);
  mo[1] = make_uint4(0u, 0u, 0u, 0u);
  neg[i] = a < 0 ? 1 : 0;
  act[i] = a;
  bad[i] = b;
}

__global__ __launch_bounds__(kE2Block) void e2_act_kernel(const long long* __restrict__ v, const uint8_t* __restrict__ found, size_t n, int relu,
                                                          int shift_bits, uint32_t* __restrict__ m, uint8_t* __restrict__ neg,
                                                          long long* __restrict__ act, uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  act_emit(v[i], found[i] ? 0 : kActNotFound, i, relu, shift_bits, m, neg, act, bad);
}

// The activation of a round that pools by maximum: one lane per OUTPUT element (p, oy, ox) of planes x Ho x Wo, which reads the
// k x k raw decryptions of its window in plane p of H x W and their found bytes; a is their maximum, kActNotFound when any of
// them has no value, and the rest is act_emit.  A window never crosses a plane: oy * stride + k <= H and ox * stride + k <= W
// by Ho = (H - k) / stride + 1 (the host's), so every index is below planes * H * W.  ReLU, the rounding to float32, the
// power-of-two scale and the truncation are all non-decreasing, so act(max v) = max act(v)
__global__ __launch_bounds__(kE2Block) void e2_act_pool_kernel(const long long* __restrict__ v, const uint8_t* __restrict__ found, size_t n_out,
                                                               uint32_t H, uint32_t W, uint32_t Ho, uint32_t Wo, uint32_t k, uint32_t stride,
                                                               int relu, int shift_bits, uint32_t* __restrict__ m, uint8_t* __restrict__ neg,
                                                               long long* __restrict__ act, uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n_out) return;
  const size_t per = (size_t)Ho * Wo, p = i / per, t = i % per;
  const size_t base = p * H * W + (t / Wo) * stride * W + (t % Wo) * stride;
  long long a = v[base];
  uint8_t all = found[base];
  for (uint32_t y = 0; y < k; y++)
    for (uint32_t x = 0; x < k; x++) {
      const size_t at = base + (size_t)y * W + x;
      const long long c = v[at];
      a = c > a ? c : a;
      all &= found[at];
    }
  act_emit(a, all ? 0 : kActNotFound, i, relu, shift_bits, m, neg, act, bad);
}

// the generator G of E2, canonical little-endian
const uint8_t kGx[32] = {0x74, 0xa7, 0xeb, 0x7c, 0x9d, 0xce, 0x1e, 0x21, 0x93, 0x6a, 0x35, 0x97, 0x79, 0x50, 0x40, 0x24,
                         0x72, 0x67, 0xcd, 0xa5, 0x3c, 0xba, 0x65, 0xf5, 0x70, 0xab, 0xb3, 0x3b, 0x6b, 0xfd, 0x15, 0x0a};
const uint8_t kGy[32] = {0x96, 0xbb, 0x87, 0x62, 0x3d, 0xaf, 0x8a, 0x1f, 0xbe, 0xfd, 0x07, 0xa8, 0x82, 0x88, 0x01, 0x59,
                         0xc5, 0x7c, 0x0a, 0x85, 0x5b, 0x90, 0x8f, 0xb3, 0x7f, 0x29, 0x12, 0x66, 0xc7, 0x32, 0x83, 0x01};

int launch_base_mul(vpin_ctx* c, const vpin_e2_base* b, const uint32_t* d_s, const uint8_t* d_neg, size_t n, e2_jac* out) {
  hipLaunchKernelGGL(e2_base_mul_kernel, dim3(blocks_of(n, kE2Block)), dim3(kE2Block), 0, c->stream, (const fq*)b->tx, (const fq*)b->ty, b->w,
                     d_s, d_neg, n, e2_curve_a(), out);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

// lanes per point, as a power of two: no more than kDlogLanes, than the giant steps there are, or than keeps the launch
// within what the device holds at once (2 workgroups on each of its 256 compute units)
int walk_lanes_log(size_t n, uint64_t max_giant) {
  int l = 0;
  while ((2 << l) <= client::kDlogLanes && ((uint64_t)2 << l) <= max_giant + 1 && (n << (l + 1)) <= (size_t)2 * 256 * kE2Block) l++;
  return l;
}

// the walk over n points resident as Montgomery coordinates into the device words v (n x 8 bytes) and f (n bytes), not synchronised
int launch_walk(vpin_ctx* c, const vpin_e2_dlog* t, const fq* X, const fq* Y, const uint8_t* inf, size_t n, uint64_t max_giant, void* v, void* f) {
  VPIN_HIP_TRY(hipMemsetAsync(v, 0, n * 8, c->stream));
  VPIN_HIP_TRY(hipMemsetAsync(f, 0, n, c->stream));
  const int ll = walk_lanes_log(n, max_giant);
  hipLaunchKernelGGL(e2_dlog_walk_kernel, dim3(blocks_of(n << ll, kE2Block)), dim3(kE2Block), 0, c->stream, X, Y, inf, n, (const fq*)t->tx,
                     (const uint8_t*)t->par, (const unsigned long long*)t->idx, t->slots - 1, t->nb, (const fq*)t->dmx, (const fq*)t->dmy, ll,
                     max_giant, e2_curve_a(), (long long*)v, (uint8_t*)f);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

// the walk, its values and flags to the host; synchronises
int run_walk(vpin_ctx* c, const vpin_e2_dlog* t, const fq* X, const fq* Y, const uint8_t* inf, size_t n, uint64_t max_giant, int64_t* v_out,
             uint8_t* found_out) {
  DevBuf v(c), f(c);
  if (v.alloc(n * 8) || f.alloc(n)) return VPIN_ENOMEM;
  const int rc = launch_walk(c, t, X, Y, inf, n, max_giant, v.p, f.p);
  if (rc) return rc;
  VPIN_HIP_TRY(hipMemcpyAsync(v_out, v.p, n * 8, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(found_out, f.p, n, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

}  // namespace

namespace client {

void base_free(vpin_e2_base* b) {
  if (!b) return;
  dev_free_owned(b->owner, nullptr, b->tx);
  dev_free_owned(b->owner, nullptr, b->ty);
  delete b;
}

int base_build(vpin_ctx* c, const uint8_t x[32], const uint8_t y[32], int w, vpin_e2_base** out) {
  (void)hipSetDevice(c->device);
  const uint8_t* bx = x ? x : kGx;
  const uint8_t* by = x ? y : kGy;
  E2Points base(c);  // the range and curve checks of every loaded point
  const uint8_t not_inf = 0;
  int rc = base.load(c, bx, by, &not_inf, 1, "vpin_e2_base_create", "base point");
  if (rc) return rc;
  vpin_e2_base* b = new (std::nothrow) vpin_e2_base();
  if (!b) return VPIN_ENOMEM;
  b->owner = c;
  b->w = w;
  b->nwin = (252 + w - 1) / w;  // the group order has 252 bits
  const size_t n = (size_t)b->nwin * (((size_t)1 << w) - 1);
  DevBuf jac(c), cx(c), cy(c), fl(c);
  if (jac.alloc(n * sizeof(e2_jac)) || cx.alloc(n * 32) || cy.alloc(n * 32) || fl.alloc(n) || dev_alloc(c, n * 32, &b->tx) ||
      dev_alloc(c, n * 32, &b->ty)) {
    base_free(b);
    return VPIN_ENOMEM;
  }
  hipLaunchKernelGGL(e2_base_rows_kernel, dim3(1), dim3(64), 0, c->stream, fq_of_le32(bx), fq_of_le32(by), w, b->nwin, e2_curve_a(), (e2_jac*)jac.p);
  rc = hipGetLastError() == hipSuccess ? VPIN_OK : VPIN_EHIP;
  // no entry is the identity: the group order is prime and d * 2^(w k) is not a multiple of it
  if (!rc) rc = e2_to_affine(c, (const e2_jac*)jac.p, n, (fq*)b->tx, (fq*)b->ty, (fq*)cx.p, (fq*)cy.p, (uint8_t*)fl.p);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = VPIN_EHIP;
  if (rc) {
    base_free(b);
    return rc;
  }
  *out = b;
  return VPIN_OK;
}

int base_mul(vpin_ctx* c, const vpin_e2_base* b, const uint8_t* scalars_le32, size_t cnt, uint8_t* ox, uint8_t* oy, uint8_t* oinf) {
  (void)hipSetDevice(c->device);
  DevBuf s(c), jac(c);
  if (s.alloc(cnt * 32) || jac.alloc(cnt * sizeof(e2_jac))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(s.p, scalars_le32, cnt * 32, hipMemcpyHostToDevice, c->stream));
  const int rc = launch_base_mul(c, b, (const uint32_t*)s.p, nullptr, cnt, (e2_jac*)jac.p);
  if (rc) return rc;
  return e2_emit(c, (const e2_jac*)jac.p, cnt, ox, oy, oinf);
}

// The device side of an encryption over cnt elements whose r (cnt x 32 bytes), message magnitudes (cnt x 32 bytes) and sign bytes
// are resident: the three multiplications, the last addition, one normalisation of c1 | c2 and the copies of the canonical bytes
// to the host.  r * H comes from h's table, or, with pub, from the loaded public keys by double-and-add: element i under pub's
// point d_key_of[i] (h is then not read).  Not synchronised; the buffers live until the caller has synchronised
struct EncryptChain {
  DevBuf ct, rh, mg;  // ct = c1 | c2 (one normalisation for both); rh = r * H, mg = msg * G
  E2Affine aff;
  explicit EncryptChain(vpin_ctx* c) : ct(c), rh(c), mg(c), aff(c) {}
  int run(vpin_ctx* c, const vpin_e2_base* g, const vpin_e2_base* h, const void* d_r, const void* d_m, const void* d_neg, size_t cnt,
          uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf, const E2Points* pub = nullptr,
          const void* d_key_of = nullptr);
};

int encrypt(vpin_ctx* c, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t* r_le32, const uint8_t* m_le32, const uint8_t* neg,
            size_t cnt, uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf) {
  (void)hipSetDevice(c->device);
  DevBuf r(c), m(c), ng(c);
  if (r.alloc(cnt * 32) || m.alloc(cnt * 32) || ng.alloc(cnt)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le32, cnt * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(m.p, m_le32, cnt * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ng.p, neg, cnt, hipMemcpyHostToDevice, c->stream));
  EncryptChain e(c);
  const int rc = e.run(c, g, h, r.p, m.p, ng.p, cnt, c1x, c1y, c1inf, c2x, c2y, c2inf);
  if (rc) return rc;
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

int EncryptChain::run(vpin_ctx* c, const vpin_e2_base* g, const vpin_e2_base* h, const void* d_r, const void* d_m, const void* d_neg, size_t cnt,
                      uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf, const E2Points* pub,
                      const void* d_key_of) {
  if (ct.alloc(2 * cnt * sizeof(e2_jac)) || rh.alloc(cnt * sizeof(e2_jac)) || mg.alloc(cnt * sizeof(e2_jac))) return VPIN_ENOMEM;
  e2_jac* c1 = (e2_jac*)ct.p;
  int rc = launch_base_mul(c, g, (const uint32_t*)d_r, nullptr, cnt, c1);
  if (!rc && !pub) rc = launch_base_mul(c, h, (const uint32_t*)d_r, nullptr, cnt, (e2_jac*)rh.p);
  if (!rc && pub) {
    hipLaunchKernelGGL(e2_mul_keyed_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, pub->X(), pub->Y(),
                       (const uint32_t*)d_key_of, (const uint32_t*)d_r, cnt, e2_curve_a(), (e2_jac*)rh.p);
    VPIN_HIP_TRY(hipGetLastError());
  }
  if (!rc) rc = launch_base_mul(c, g, (const uint32_t*)d_m, (const uint8_t*)d_neg, cnt, (e2_jac*)mg.p);
  if (rc) return rc;
  hipLaunchKernelGGL(e2_add_pairs_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, (const e2_jac*)mg.p, (const e2_jac*)rh.p,
                     cnt, e2_curve_a(), c1 + cnt);
  VPIN_HIP_TRY(hipGetLastError());
  if ((rc = aff.normalise(c, c1, 2 * cnt))) return rc;
  if ((rc = aff.copy_out(c, 0, cnt, c1x, c1y, c1inf))) return rc;
  return aff.copy_out(c, cnt, cnt, c2x, c2y, c2inf);
}

int encrypt_keyed(vpin_ctx* c, const vpin_e2_base* g, const uint8_t* hx, const uint8_t* hy, size_t n_pub, const uint32_t* key_of,
                  const uint8_t* r_le32, const uint8_t* m_le32, const uint8_t* neg, size_t cnt, size_t* bad_key, uint8_t* c1x, uint8_t* c1y,
                  uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf) {
  (void)hipSetDevice(c->device);
  *bad_key = n_pub;
  E2Points pub(c);
  const std::vector<uint8_t> not_inf(n_pub, 0);
  int rc = pub.load(c, hx, hy, not_inf.data(), n_pub, "vpin_e2_encrypt_keyed", "public key");
  if (rc == VPIN_EINVAL) {
    // which key: the rejection does not say, so on this path the keys go through the checks again one at a time; the first one
    // refused is named, and its own rule is the text
    for (size_t k = 0; k < n_pub && *bad_key == n_pub; k++) {
      E2Points one(c);
      if (one.load(c, hx + 32 * k, hy + 32 * k, not_inf.data(), 1, "vpin_e2_encrypt_keyed", "public key") == VPIN_EINVAL) *bad_key = k;
    }
  }
  if (rc) return rc;
  DevBuf r(c), m(c), ng(c), ko(c);
  if (r.alloc(cnt * 32) || m.alloc(cnt * 32) || ng.alloc(cnt) || ko.alloc(cnt * 4)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le32, cnt * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(m.p, m_le32, cnt * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ng.p, neg, cnt, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ko.p, key_of, cnt * 4, hipMemcpyHostToDevice, c->stream));
  EncryptChain e(c);
  if ((rc = e.run(c, g, nullptr, r.p, m.p, ng.p, cnt, c1x, c1y, c1inf, c2x, c2y, c2inf, &pub, ko.p))) return rc;
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

// T_i = s * P_i over the loaded points, Jacobian, not synchronised
static int launch_mul256(vpin_ctx* c, const E2Points& pts, const uint32_t* d_s, bool one_scalar, size_t cnt, e2_jac* out) {
  hipLaunchKernelGGL(e2_mul256_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, pts.X(), pts.Y(), pts.F(), d_s,
                     (size_t)(one_scalar ? 0 : 8), cnt, e2_curve_a(), out);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

int mul256(vpin_ctx* c, const uint8_t* scalars_le32, bool one_scalar, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt,
           uint8_t* ox, uint8_t* oy, uint8_t* oinf) {
  (void)hipSetDevice(c->device);
  E2Points pts(c);
  int rc = pts.load(c, px, py, pinf, cnt, "vpin_e2_mul256", "point");
  if (rc) return rc;
  const size_t ns = one_scalar ? 1 : cnt;
  DevBuf s(c), jac(c);
  if (s.alloc(ns * 32) || jac.alloc(cnt * sizeof(e2_jac))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(s.p, scalars_le32, ns * 32, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_mul256(c, pts, (const uint32_t*)s.p, one_scalar, cnt, (e2_jac*)jac.p))) return rc;
  return e2_emit(c, (const e2_jac*)jac.p, cnt, ox, oy, oinf);
}

void dlog_free(vpin_e2_dlog* t) {
  if (!t) return;
  dev_free_owned(t->owner, nullptr, t->tx);
  dev_free_owned(t->owner, nullptr, t->par);
  dev_free_owned(t->owner, nullptr, t->idx);
  dev_free_owned(t->owner, nullptr, t->dmx);
  dev_free_owned(t->owner, nullptr, t->dmy);
  delete t;
}

int dlog_build(vpin_ctx* c, uint64_t nb, vpin_e2_dlog** out) {
  (void)hipSetDevice(c->device);
  vpin_e2_dlog* t = new (std::nothrow) vpin_e2_dlog();
  if (!t) return VPIN_ENOMEM;
  t->owner = c;
  t->nb = nb;
  t->slots = 16;
  while (t->slots < 2 * nb) t->slots <<= 1;
  t->bytes = nb * 32 + nb + t->slots * 8 + 2 * kDlogLanes * 32;
  vpin_e2_base* g = nullptr;
  int rc = base_build(c, nullptr, nullptr, kDefaultWindow, &g);
  if (rc) { dlog_free(t); return rc; }
  struct Guard {
    vpin_e2_base* g;
    vpin_e2_dlog* t;
    ~Guard() { base_free(g); dlog_free(t); }
  } guard{g, t};
  const size_t tile = (size_t)(nb < kTile ? (nb + kStepsChunk - 1) / kStepsChunk * kStepsChunk : kTile);
  DevBuf jac(c), my(c), cx(c), cy(c), fl(c), s(c);
  if (dev_alloc(c, nb * 32, &t->tx) || dev_alloc(c, nb, &t->par) || dev_alloc(c, t->slots * 8, &t->idx) || jac.alloc(tile * sizeof(e2_jac)) ||
      my.alloc(tile * 32) || cx.alloc(tile * 32) || cy.alloc(tile * 32) || fl.alloc(tile) || s.alloc(kDlogLanes * 32) ||
      dev_alloc(c, kDlogLanes * 32, &t->dmx) || dev_alloc(c, kDlogLanes * 32, &t->dmy)) {
    set_last_error_text("vpin_e2_dlog_create: the baby-step table does not fit the device memory");
    return VPIN_ENOMEM;
  }
  VPIN_HIP_TRY(hipMemsetAsync(t->idx, 0, t->slots * 8, c->stream));
  VPIN_HIP_TRY(hipMemsetAsync(t->par, 0, nb, c->stream));
  const fq a = e2_curve_a(), gx = fq_of_le32(kGx), gy = fq_of_le32(kGy);
  for (uint64_t j0 = 0; j0 < nb; j0 += tile) {
    const size_t count = (size_t)(nb - j0 < tile ? nb - j0 : tile), lanes = (count + kStepsChunk - 1) / kStepsChunk;
    hipLaunchKernelGGL(e2_dlog_steps_kernel, dim3(blocks_of(lanes, kStepsBlock)), dim3(kStepsBlock), 0, c->stream, (const fq*)g->tx,
                       (const fq*)g->ty, g->w, j0, lanes, gx, gy, a, (e2_jac*)jac.p);
    VPIN_HIP_TRY(hipGetLastError());
    if ((rc = e2_to_affine(c, (const e2_jac*)jac.p, count, (fq*)t->tx + j0, (fq*)my.p, (fq*)cx.p, (fq*)cy.p, (uint8_t*)fl.p))) return rc;
    hipLaunchKernelGGL(e2_dlog_insert_kernel, dim3(blocks_of(count, kE2Block)), dim3(kE2Block), 0, c->stream, (const fq*)t->tx, (const fq*)cy.p,
                       j0, count, (uint8_t*)t->par, (unsigned long long*)t->idx, t->slots - 1);
    VPIN_HIP_TRY(hipGetLastError());
  }
  // the multiples l * D, l = 1 .. kDlogLanes, of the giant step D = nb * G, kept in Montgomery form (l * nb <= 2^34)
  uint8_t mult_le32[kDlogLanes * 32] = {};
  for (uint64_t l = 1; l <= (uint64_t)kDlogLanes; l++) {
    const uint64_t m = l * nb;
    memcpy(mult_le32 + 32 * (l - 1), &m, 8);
  }
  VPIN_HIP_TRY(hipMemcpyAsync(s.p, mult_le32, sizeof(mult_le32), hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_base_mul(c, g, (const uint32_t*)s.p, nullptr, kDlogLanes, (e2_jac*)jac.p))) return rc;
  if ((rc = e2_to_affine(c, (const e2_jac*)jac.p, kDlogLanes, (fq*)t->dmx, (fq*)t->dmy, (fq*)cx.p, (fq*)cy.p, (uint8_t*)fl.p))) return rc;
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  guard.t = nullptr;
  *out = t;
  return VPIN_OK;
}

int dlog_solve(vpin_ctx* c, const vpin_e2_dlog* t, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt, uint64_t max_giant,
               int64_t* v_out, uint8_t* found_out) {
  (void)hipSetDevice(c->device);
  E2Points pts(c);
  const int rc = pts.load(c, px, py, pinf, cnt, "vpin_e2_dlog_solve", "point");
  if (rc) return rc;
  return run_walk(c, t, pts.X(), pts.Y(), pts.F(), cnt, max_giant, v_out, found_out);
}

// The device side of a decryption up to the walk's input: the two ciphertext halves through the range and curve checks (who: the
// entry point the rejection names), T = sk * c1, M = c2 - T normalised into m.  Not synchronised past the checks
struct DecryptChain {
  E2Points c1, c2, m;
  DevBuf s, T, M;
  E2Affine aff;
  explicit DecryptChain(vpin_ctx* c) : c1(c), c2(c), m(c), s(c), T(c), M(c), aff(c) {}
  int run(vpin_ctx* c, const char* who, const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
          const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt) {
    int rc = c1.load(c, c1x, c1y, c1inf, cnt, who, "c1 point");
    if (!rc) rc = c2.load(c, c2x, c2y, c2inf, cnt, who, "c2 point");
    if (rc) return rc;
    if (s.alloc(32) || T.alloc(cnt * sizeof(e2_jac)) || M.alloc(cnt * sizeof(e2_jac))) return VPIN_ENOMEM;
    VPIN_HIP_TRY(hipMemcpyAsync(s.p, sk_le32, 32, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_mul256(c, c1, (const uint32_t*)s.p, true, cnt, (e2_jac*)T.p))) return rc;
    hipLaunchKernelGGL(e2_sub_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, (const e2_jac*)T.p, c2.X(), c2.Y(), c2.F(),
                       cnt, e2_curve_a(), (e2_jac*)M.p);
    VPIN_HIP_TRY(hipGetLastError());
    return aff.normalise(c, (const e2_jac*)M.p, cnt, &m);
  }
};

int decrypt(vpin_ctx* c, const vpin_e2_dlog* t, const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
            const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint64_t max_giant, int64_t* v_out,
            uint8_t* found_out) {
  (void)hipSetDevice(c->device);
  DecryptChain d(c);
  const int rc = d.run(c, "vpin_e2_decrypt", sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt);
  if (rc) return rc;
  return run_walk(c, t, d.m.X(), d.m.Y(), d.m.F(), cnt, max_giant, v_out, found_out);
}

// round and round_pool: pool = NULL activates element by element (cnt_out = cnt)
static int run_round(vpin_ctx* c, const char* who, const vpin_e2_dlog* t, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t sk_le32[32],
                     const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf,
                     size_t cnt, const PoolShape* pool, uint64_t max_giant, bool relu, int shift_bits, const uint8_t* r_le32, int64_t* v_out,
                     int64_t* act_out, uint8_t* bad_out, uint8_t* found_out, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x,
                     uint8_t* o2y, uint8_t* o2inf) {
  (void)hipSetDevice(c->device);
  const size_t n_out = pool ? pool->planes * pool->Ho() * pool->Wo() : cnt;
  DevBuf r(c), v(c), f(c), m(c), ng(c), act(c), bad(c);
  if (v.alloc(cnt * 8) || f.alloc(cnt) || m.alloc(n_out * 32) || ng.alloc(n_out) || act.alloc(n_out * 8) || bad.alloc(n_out)) return VPIN_ENOMEM;
  if (r_le32) {
    if (r.alloc(n_out * 32)) return VPIN_ENOMEM;
    VPIN_HIP_TRY(hipMemcpyAsync(r.p, r_le32, n_out * 32, hipMemcpyHostToDevice, c->stream));
  }
  DecryptChain d(c);
  int rc = d.run(c, who, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt);
  if (!rc) rc = launch_walk(c, t, d.m.X(), d.m.Y(), d.m.F(), cnt, max_giant, v.p, f.p);
  if (rc) return rc;
  if (pool)
    hipLaunchKernelGGL(e2_act_pool_kernel, dim3(blocks_of(n_out, kE2Block)), dim3(kE2Block), 0, c->stream, (const long long*)v.p,
                       (const uint8_t*)f.p, n_out, (uint32_t)pool->H, (uint32_t)pool->W, (uint32_t)pool->Ho(), (uint32_t)pool->Wo(),
                       (uint32_t)pool->k, (uint32_t)pool->stride, relu ? 1 : 0, shift_bits, (uint32_t*)m.p, (uint8_t*)ng.p, (long long*)act.p,
                       (uint8_t*)bad.p);
  else
    hipLaunchKernelGGL(e2_act_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, (const long long*)v.p, (const uint8_t*)f.p, cnt,
                       relu ? 1 : 0, shift_bits, (uint32_t*)m.p, (uint8_t*)ng.p, (long long*)act.p, (uint8_t*)bad.p);
  VPIN_HIP_TRY(hipGetLastError());
  EncryptChain e(c);
  if (r_le32 && (rc = e.run(c, g, h, r.p, m.p, ng.p, n_out, o1x, o1y, o1inf, o2x, o2y, o2inf))) return rc;
  VPIN_HIP_TRY(hipMemcpyAsync(v_out, v.p, cnt * 8, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(act_out, act.p, n_out * 8, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(bad_out, bad.p, n_out, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  if (found_out) {  // the failure path of a pooled round: which input element it was
    bool any = false;
    for (size_t i = 0; i < n_out && !any; i++) any = (bad_out[i] & 1) != 0;
    if (any) {
      VPIN_HIP_TRY(hipMemcpyAsync(found_out, f.p, cnt, hipMemcpyDeviceToHost, c->stream));
      VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
    }
  }
  return VPIN_OK;
}

int round(vpin_ctx* c, const vpin_e2_dlog* t, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t sk_le32[32], const uint8_t* c1x,
          const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt,
          uint64_t max_giant, bool relu, int shift_bits, const uint8_t* r_le32, int64_t* v_out, int64_t* act_out, uint8_t* bad_out,
          uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  return run_round(c, "vpin_e2_client_round", t, g, h, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, nullptr, max_giant, relu, shift_bits, r_le32,
                   v_out, act_out, bad_out, nullptr, o1x, o1y, o1inf, o2x, o2y, o2inf);
}

int round_pool(vpin_ctx* c, const vpin_e2_dlog* t, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t sk_le32[32], const uint8_t* c1x,
               const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const PoolShape& pool,
               uint64_t max_giant, bool relu, int shift_bits, const uint8_t* r_le32, int64_t* v_out, int64_t* act_out, uint8_t* bad_out,
               uint8_t* found_out, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  return run_round(c, "vpin_e2_client_round_pool", t, g, h, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, pool.planes * pool.H * pool.W, &pool,
                   max_giant, relu, shift_bits, r_le32, v_out, act_out, bad_out, found_out, o1x, o1y, o1inf, o2x, o2y, o2inf);
}

}  // namespace client

}  // namespace vpin
