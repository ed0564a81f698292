// ge_tree_dev.h -- the group-element layer the MSM files share (msm.hip, msm_pip.hip, msm_var.hip): points to and from
// global memory, the limb-strided ten-limb form, the signed-window recoding of every MSM (bucket methods, table walks, row
// table) and the Horner sum of the bucket methods, and
// the block tree that sums the points of a workgroup with four lanes per addition
#pragma once
#include "fp10_dev.h"

namespace vpin {

// ---- points to and from global memory ----------------------------------------------------------------------------------
__device__ __forceinline__ ge_ext ge_load(const ge_ext* p) {
  ge_ext e;
  e.X = fp_load(&p->X); e.Y = fp_load(&p->Y); e.Z = fp_load(&p->Z); e.T = fp_load(&p->T);
  return e;
}
__device__ __forceinline__ void ge_store(ge_ext* o, const ge_ext& a) {
  fp_store(&o->X, a.X); fp_store(&o->Y, a.Y); fp_store(&o->Z, a.Z); fp_store(&o->T, a.T);
}
__device__ __forceinline__ void ge_store_identity(ge_ext* o) { ge_store(o, ge_identity()); }
__device__ __forceinline__ ge_niels ge_load(const ge_niels* p) {
  ge_niels e;
  e.ypx = fp_load(&p->ypx); e.ymx = fp_load(&p->ymx); e.xy2d = fp_load(&p->xy2d);
  return e;
}
__device__ __forceinline__ void ge_store(ge_niels* o, const ge_niels& a) {
  fp_store(&o->ypx, a.ypx); fp_store(&o->ymx, a.ymx); fp_store(&o->xy2d, a.xy2d);
}
__device__ __forceinline__ ge_cached ge_load(const ge_cached* p) {
  ge_cached e;
  e.YpX = fp_load(&p->YpX); e.YmX = fp_load(&p->YmX); e.Z = fp_load(&p->Z); e.T2d = fp_load(&p->T2d);
  return e;
}
__device__ __forceinline__ void ge_store(ge_cached* o, const ge_cached& a) {
  fp_store(&o->YpX, a.YpX); fp_store(&o->YmX, a.YmX); fp_store(&o->Z, a.Z); fp_store(&o->T2d, a.T2d);
}
// a point as X | Y | Z | T, four consecutive field elements (the form the host holds): as stored, or canonical
__device__ __forceinline__ ge_ext ge_load(const fp* xyzt) { return ge_load(reinterpret_cast<const ge_ext*>(xyzt)); }
__device__ __forceinline__ void ge_store(fp* xyzt, const ge_ext& a) { ge_store(reinterpret_cast<ge_ext*>(xyzt), a); }
__device__ __forceinline__ void ge_store_frozen(fp* xyzt, const ge_ext& a) {
  fp_store(xyzt, fp_freeze(a.X)); fp_store(xyzt + 1, fp_freeze(a.Y)); fp_store(xyzt + 2, fp_freeze(a.Z)); fp_store(xyzt + 3, fp_freeze(a.T));
}
// the end of a variable-base MSM: the compressed encoding and the canonical X | Y | Z | T
__device__ __forceinline__ void ge_store_result(fp* out32, fp* out_xyzt, const ge_ext& r) {
  fp_store(out32, ge_compress(r));
  ge_store_frozen(out_xyzt, r);
}

// ---- ten-limb points, limb-strided: limb l of coordinate k at p[(10 k + l) stride] (lane- or bucket-major arrays) --------
__device__ __forceinline__ void ge10_store_strided(uint32_t* __restrict__ p, size_t stride, const ge10& a) {
#pragma unroll
  for (int l = 0; l < 10; l++) {
    p[(size_t)l * stride] = a.X.v[l]; p[(size_t)(10 + l) * stride] = a.Y.v[l];
    p[(size_t)(20 + l) * stride] = a.Z.v[l]; p[(size_t)(30 + l) * stride] = a.T.v[l];
  }
}
__device__ __forceinline__ ge10 ge10_load_strided(const uint32_t* __restrict__ p, size_t stride) {
  ge10 a;
#pragma unroll
  for (int l = 0; l < 10; l++) {
    a.X.v[l] = p[(size_t)l * stride]; a.Y.v[l] = p[(size_t)(10 + l) * stride];
    a.Z.v[l] = p[(size_t)(20 + l) * stride]; a.T.v[l] = p[(size_t)(30 + l) * stride];
  }
  return a;
}

// ---- signed windows of a scalar ------------------------------------------------------------------------------------------
// Every method cuts a canonical scalar into windows of c bits, low end first, and turns a window value past half = 2^(c-1)
// into the negative digit v - 2^c with a carry into the window above.  ONE primitive takes a window; three rules say when
// a value is negated and how the digit is written: fq_signed_window (bucket methods), walk_digit (table walks), row_digit
// (row table).

// s -> q - s when s is in the upper half (bit 251 or 252 set): s*g = -((q - s)*g).  Nothing for a random scalar,
// but the R1CS values -1, -2 (a fifth of comb_ops' val slices) become one table add instead of W.
__device__ __forceinline__ bool fq_fold_sign(fq& s) {
  if (s.v[7] < 0x08000000u) return false;
  fq d;
  unsigned bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d.v[i] = __builtin_subc(fq_modulus_limb(i), s.v[i], bw, &bw);
  s = d;
  return true;
}

// The primitive: the low cw bits of s plus the carry of the window below; s is shifted right by cw bits (static register
// indices only).  cw in 1..31.  The bits are taken with one bit-field extract: a mask (1 << cw) - 1 would be a loop invariant
// that the walks keep in a register of its own, and the row kernels have none to spare (__launch_bounds__(256, 3)).
__device__ __forceinline__ uint32_t fq_take_window(fq& s, uint32_t carry, uint32_t cw) {
  const uint32_t v = __builtin_amdgcn_ubfe(s.v[0], 0u, cw) + carry;
#pragma unroll
  for (int i = 0; i < 7; i++) s.v[i] = __builtin_amdgcn_alignbit(s.v[i + 1], s.v[i], cw);
  s.v[7] >>= cw;
  return v;
}

// The bucket methods' rule: v > half negates, but never in the top window, and nothing is folded (walk_digit negates every
// window alike and applies the fold; row_digit lets a tie follow the fold).  The digit comes back as sign and magnitude (|d|
// in bits 0..14, sign in bit 15, 0 for a zero digit); carry <- 1 when the digit was negated.
__device__ __forceinline__ uint16_t fq_signed_window(fq& s, uint32_t& carry, uint32_t cw, bool top) {
  uint32_t v = fq_take_window(s, carry, cw);
  const bool neg = !top && v > (1u << (cw - 1));
  if (neg) v = (1u << cw) - v;
  carry = neg ? 1u : 0u;
  return (uint16_t)(v | (neg && v ? 0x8000u : 0u));
}

// The table walks' rule, for a window value v (digit + carry) of a sign-folded scalar: v > half negates in every window, a
// tie stays positive, then the fold's flip is applied (fq_signed_window spares the top window and knows no fold; row_digit
// breaks the tie by the fold).  Returns the magnitude (0: nothing to add; the table entry is magnitude - 1), neg <- the
// digit's sign, carry <- 1 when v was negated.
__device__ __forceinline__ uint32_t walk_digit(uint32_t v, uint32_t c, bool flip, uint32_t& carry, bool& neg) {
  const bool past = v > (1u << (c - 1));
  carry = past ? 1u : 0u;
  neg = past != flip;
  return past ? (1u << c) - v : v;
}

// digit w (c bits) of a canonical scalar, for the kernels that split one scalar over several lanes
__device__ __forceinline__ uint32_t scalar_digit(const fq& s, int w, int c) {
  int off = w * c, word = off >> 5, sh = off & 31;
  uint32_t lo = s.v[word], hi = (word + 1 < 8) ? s.v[word + 1] : 0u;
  uint64_t both = ((uint64_t)hi << 32) | lo;
  return (uint32_t)(both >> sh) & ((1u << c) - 1u);
}

// walk_digit's carry into window w0 without the windows below having been walked: decided by the nearest lower digit that
// is not exactly 2^(c-1)
__device__ __forceinline__ uint32_t carry_into(const fq& s, int w0, int c) {
  const uint32_t half = 1u << (c - 1);
  for (int w = w0 - 1; w >= 0; w--) {
    uint32_t d = scalar_digit(s, w, c);
    if (d != half) return d > half ? 1u : 0u;
  }
  return 0u;
}

// The row table's rule, one digit of a sign-folded scalar in a 16-bit word: magnitude - 1 in bits 0..14, the sign in bit 15,
// kNoDigit for a zero digit.  Unlike walk_digit a tie at 2^(c-1) follows the fold -- +2^(c-1) without it, -2^(c-1) (carrying)
// with it -- so that AFTER the flip the negative magnitudes stay below 2^(c-1) and 16 bits hold a 16-bit window's digits; like
// fq_signed_window the top window is never negated (its value is at most 2^(c-1), see row_windows in msm.hip).
constexpr uint16_t kNoDigit = 0xffffu;  // never a digit: a negative digit's magnitude is below 2^(c-1), c <= 16
__device__ __forceinline__ uint16_t row_digit(fq& s, uint32_t& carry, int c, bool flip, bool top) {
  const uint32_t half = 1u << (c - 1);
  const uint32_t v = fq_take_window(s, carry, (uint32_t)c);
  const bool neg = !top && (flip ? v >= half : v > half);
  const uint32_t mag = neg ? (1u << c) - v : v;
  carry = neg ? 1u : 0u;
  return mag ? (uint16_t)((mag - 1u) | ((neg != flip) ? 0x8000u : 0u)) : kNoDigit;
}

// sum_w 2^(offset of window w) wsum[w] over W windows, window w being width(w) bits wide: Horner from the top window down,
// one lane
template <class Width>
__device__ __forceinline__ ge10 ge10_horner_windows(const ge_ext* wsum, int W, Width width) {
  ge10 acc = ge10_from_ext(ge_load(wsum + W - 1));
#pragma unroll 1
  for (int w = W - 2; w >= 0; w--) {
#pragma unroll 1
    for (int k = 0, cw = width(w); k < cw; k++) acc = ge10_double(acc);
    acc = ge10_add_ge10(acc, ge10_from_ext(ge_load(wsum + w)));
  }
  return acc;
}

// ---- block tree with four lanes per addition -----------------------------------------------------------------
// The few-row MSMs are latency bound: one wave per SIMD issues a modular product in ~0.5 us, and an addition of two
// extended points is nine of them in a row on one lane.  Here the four products of each half of the addition
// (add-2008-hwcd-3: A,B,C,D then X3,Y3,Z3,T3) run on the four lanes of a quad -- same code path, operands picked by the
// lane's role, the halves exchanged with lane shuffles -- so a level costs three products instead of nine.
__device__ __forceinline__ fp fp_shfl_from(const fp& a, int src) {
  fp r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = __shfl(a.v[i], src, 64);
  return r;
}
__device__ __forceinline__ fp fp_pick(bool c, const fp& a, const fp& b) {
  fp r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
// sh[0] = sum of sh[0..n) (n a power of two, n <= blockDim.x); every thread of the block calls it.
// split > 0 (a power of two below n): the entries alternate in runs of `split` between two sums (index & split); the
// level that would mix them is skipped and the levels below it reduce both runs: sh[0] = sum of the entries with
// (index & split) == 0, sh[split] = sum of the others.
// sh[i] += sh[j] by the four lanes of a quad (role = lane & 3, qbase = the quad's first lane in its wave); all four call it
__device__ __forceinline__ void ge_quad_add_into(ge_ext* sh, int i, int j, int role, int qbase) {
  const fp* shf = reinterpret_cast<const fp*>(sh);
  fp* shw = reinterpret_cast<fp*>(sh);
  // role 0: (Y1-X1)(Y2-X2)   role 1: (Y1+X1)(Y2+X2)   role 2: 2d T1 T2   role 3: 2 Z1 Z2
  const int f0 = role < 2 ? 1 : (role == 2 ? 3 : 2);  // Y | T | Z
  const fp p0 = shf[4 * i + f0], q0 = shf[4 * j + f0];
  fp u = p0, v = q0;
  if (role < 2) {  // uniform per quad pair: both take the same instructions, the select below is per lane
    const fp p1 = shf[4 * i], q1 = shf[4 * j];
    u = fp_pick(role == 0, fp_sub(p0, p1), fp_add(p0, p1));
    v = fp_pick(role == 0, fp_sub(q0, q1), fp_add(q0, q1));
  }
  fp m = fp_mul(u, v);
  m = fp_mul(m, fp_pick(role == 2, FP_D2(), fp_one()));
  m = fp_pick(role == 3, fp_add(m, m), m);
  const fp a = fp_shfl_from(m, qbase), b = fp_shfl_from(m, qbase + 1), c = fp_shfl_from(m, qbase + 2),
           d = fp_shfl_from(m, qbase + 3);
  const fp E = fp_sub(b, a), H = fp_add(b, a), F = fp_sub(d, c), G = fp_add(d, c);
  // X3 = E F, Y3 = G H, Z3 = F G, T3 = E H
  u = fp_pick(role == 0 || role == 3, E, fp_pick(role == 1, G, F));
  v = fp_pick(role == 0, F, fp_pick(role == 2, G, H));
  shw[4 * i + role] = fp_mul(u, v);
}
__device__ __forceinline__ void ge_tree_quad(ge_ext* sh, int n, int split = 0) {
  const int role = threadIdx.x & 3, qbase = (threadIdx.x & 63) & ~3;
  for (int s = n / 2; s >= 1; s >>= 1) {
    if (s == split) continue;
    const int items = s < split ? 2 * s : s;
    for (int w = threadIdx.x >> 2; w < items; w += (int)(blockDim.x >> 2)) {
      const int i = w < s ? w : split + (w - s);
      ge_quad_add_into(sh, i, i + s, role, qbase);
    }
    __syncthreads();
  }
}
// The same tree over entries that belong to W interleaved sums, entry t to sum t mod W (the lanes of the row-table kernel:
// lane t accumulates window t mod W): sh[w] = sum of sh[w], sh[w + W], sh[w + 2W], .. below n, for every w < W.  Any W >= 1.
__device__ __forceinline__ void ge_tree_quad_strided(ge_ext* sh, int n, int W) {
  const int role = threadIdx.x & 3, qbase = (threadIdx.x & 63) & ~3;
  int P = 1;
  while (P * W < n) P <<= 1;  // the entries of a sum: at most P
  for (int s = P / 2; s >= 1; s >>= 1) {
    const int items = s * W;  // entry i < s W takes entry i + s W (the live entries are those below 2 s W)
    for (int i = threadIdx.x >> 2; i < items; i += (int)(blockDim.x >> 2))
      if (i + items < n) ge_quad_add_into(sh, i, i + items, role, qbase);
    __syncthreads();
  }
}

}  // namespace vpin
