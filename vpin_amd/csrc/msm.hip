// msm.hip -- fixed-base multi-scalar multiplication over the Pedersen generators, gfx950.
//
// Replaces the reference's polynomial-commitment MSMs:
//   DensePolynomial::commit_inner   Spartan/src/dense_mlpoly.rs:160-175  (L row commitments)
//   Commitments for [Scalar]        Spartan/src/commitments.rs:93-98     (MSM + blind*h)
//   vartime_multiscalar_mul         Spartan/src/group.rs:103-122         (dalek Straus/Pippenger)
//
// MI355X-first design: every MSM of the sat proof is over the SAME generator stream
// g[0..R+2) (MultiCommitGens::new, commitments.rs:20-38), so instead of per-row Pippenger
// buckets we spend HBM (288 GB) on a window table  T[w][j][k] = (k+1) * 2^(c*w) * g_j  of
// AFFINE points (y+x, y-x, 2dxy; 96 B) with c = 11 or 12 bit signed windows (W = 24 / 22
// windows, 1024 / 2048 multiples each: 2.4-4.3 MB per generator, 9 GB for R = 2048, 19 GB for
// R = 8192) and turn each row commitment into a pure gather-and-add: a non-zero scalar costs
// at most W table additions of 7 field multiplies, no doublings, no bucket reduction, no atomics.  Zero scalars and zero
// digits are skipped (the witness is ~40% zero padding and full of 0/1 bits), like dalek's
// vartime MSM.  One 256-thread workgroup per row; per-thread partial sums are combined by
// an LDS tree.  Integer-ALU bound (~8 field multiplies per table add); no MFMA.
//
// Beside it, where the provers' budget holds one, a ROW TABLE of a single window per generator: T1[j][k] = (k+1) * g_j with 13..16
// bit windows (64 GiB for 16386 generators at 16 bits in 128-byte slots).  A row commitment is C_i = sum_w 2^(c w) A_iw with
// A_iw = sum_j digit_w(s_ij) g_j, and the sums A_iw need the multiples of g_j alone: msm_rows_win_kernel keeps one accumulator per
// lane and window, msm_rows_finish_kernel applies the powers of two once per ROW (c (W - 1) doublings against the 2^13..2^14
// scalars x 16 additions of the row: free).  A folded scalar then costs 16 additions instead of 21, and the multi-window table,
// narrowed to 8 bits, is left to the kernels that multiply one scalar by one base (bullet rounds, few-row MSMs, blind terms,
// hot-column tables, constant rows).  Commitments below row_table_min_scalars (2^20 scalars), a rank's share of a split commitment and tables built
// through the public entry points keep the multi-window walk.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.h"
#include "fp_dev.h"
#include "fp10_dev.h"
#include "ge_tree_dev.h"
#include "mailbox_dev.h"

#ifndef VPIN_NIELS_SLOT
// bytes per table entry: 96 (packed; the default) or 128 (one entry per 128-byte line: a gather is one aligned line, never two
// half-used ones).  Round 6 re-measured the pair with the spatial split and the strip kernel in place, both libraries built on the box
// and the 16386 generators of the derefs commitments at 12-bit windows in both (VPIN_SPARK_GENS_BUDGET_GB=100,
// VPIN_GENS_FREE_FRACTION=0.45): LeNet step 358.4 against 366.3 ms (-2.2 %, 12 W less) for 109 instead of 95 GiB of tables
// (profiles/r06_ab_slot128.txt).  NOT the default: with 14 GiB less headroom a 2^25 proof split over two rank-threads of ONE GPU
// (tests, rehearsals) runs out of memory once anything else is resident, and that out-of-memory hipMalloc took the process down
// inside the HIP runtime instead of returning an error.  Build with -DVPIN_NIELS_SLOT=128 (and the two budgets above) to trade
// the memory for the time on a part that proves single-GPU traces only.
#define VPIN_NIELS_SLOT 96
#endif
static_assert(VPIN_NIELS_SLOT == 96 || VPIN_NIELS_SLOT == 128, "table entry size");
// Round 6: the slot size is a property of a TABLE (decided when it is built: VPIN_TABLE_SLOT = 96 | 128, default VPIN_NIELS_SLOT), not
// of the build: an entry is three field elements (y+x, y-x, 2dxy) at the start of a slot of s32 = 3 or 4 32-byte units.

struct vpin_gens {
  // Two segments: bases [0, split) in `table` with wide windows (the generators every large commitment of a proof
  // walks), bases [split, nbt) in `table_hi` with narrow ones (the upper half of the 32k-generator stream, touched by
  // SNARK::encode and one evaluation proof, and the prefix sums).  split == nbt: a single segment.
  vpin::fp* table = nullptr;        // [W][split][E] slots of s32 field elements
  vpin::fp* table_hi = nullptr;     // [W_hi][nbt - split][E_hi]
  int s32 = VPIN_NIELS_SLOT / 32;   // 32-byte units per slot: 3 (96 B, packed) or 4 (128 B, a line per entry)
  size_t nb = 0;                    // number of bases in the stream
  size_t nbt = 0;                   // bases in the table: the stream, then the prefix sums S_k = g_0 + ... + g_{2^k - 1}
  size_t split = 0;
  int c = 12, W = 22, E = 2048;     // window bits, windows, entries per window (= 2^(c-1)) of the first segment
  int c_hi = 8, W_hi = 32, E_hi = 128;
  // Row table (optional): T1[j][k] = (k + 1) * g_j for the first n_row bases, k < E_row = 2^(c_row - 1), in the same slots.  The
  // row commitments walk it (msm_rows_win_kernel); everything that multiplies ONE scalar by one base stays on the table above.
  vpin::fp* table_row = nullptr;
  size_t n_row = 0;
  int c_row = 0, W_row = 0, E_row = 0;
  bool narrowed = false;  // the multi-window table gave way to the row table (8-bit windows): not what the public entry points build
};

namespace vpin {

struct TableView {
  const fp* t;     // first segment
  const fp* t_hi;  // second segment
  size_t split, nbt;       // bases [0, split) | [split, nbt)
  int c, W, E, c_hi, W_hi, E_hi;
  size_t sum0;  // table index of S_0; S_k = g_0 + ... + g_{2^k - 1} sits at sum0 + k
  int s32;      // field elements per slot (3 or 4)
};

// the segment of base j: table, index inside it, bases per window, window parameters
struct TableSeg {
  const fp* t;
  size_t j, nb;
  int c, W, E, s32;
  // entry d (multiple d + 1) of window w of this base
  __device__ __forceinline__ const ge_niels* entry(int w, uint32_t d) const {
    return reinterpret_cast<const ge_niels*>(t + (((size_t)w * nb + j) * (size_t)E + d) * (size_t)s32);
  }
};
__device__ __forceinline__ TableSeg table_seg(const TableView& tv, size_t j) {
  if (j < tv.split) return TableSeg{tv.t, j, tv.split, tv.c, tv.W, tv.E, tv.s32};
  return TableSeg{tv.t_hi, j - tv.split, tv.nbt - tv.split, tv.c_hi, tv.W_hi, tv.E_hi, tv.s32};
}

// The row table: one window per generator.  A row commitment is sum_w 2^(c w) A_w with A_w = sum_j digit_w(s_j) g_j, and every
// A_w needs the multiples of g_j itself only; the powers of two are applied once per row (msm_rows_finish_kernel).
struct RowTable {
  const fp* t;  // [n][E] slots
  size_t n;     // bases [0, n)
  int c, W, E, s32;
  __device__ __forceinline__ const ge_niels* entry(size_t j, uint32_t d) const {  // multiple d + 1 of base j
    return reinterpret_cast<const ge_niels*>(t + (j * (size_t)E + d) * (size_t)s32);
  }
};
// windows of c bits for a sign-folded scalar (below 2^252): the top digit, carry included, must not exceed 2^(c-1), the last entry
constexpr int row_windows(int c) { return (253 + c - 1) / c; }

// ---- table construction ---------------------------------------------------------------

// Prefix sums of the stream over power-of-two lengths, kept in the table as extra bases: a commitment row whose
// scalars are all one value s (the padding tails of the SPARK polynomials are runs of a single eq value, a
// quarter of the derefs polynomial for vPIN's instances) is s * S_k, one scalar multiplication instead of 2^k.
// Block k sums g_j over [2^(k-1), 2^k) (block 0: g_0) into xyzt[nb + k]; gens_sum_scan_kernel then accumulates.
__global__ __launch_bounds__(256) void gens_sum_kernel(fp* __restrict__ xyzt, size_t nb) {
  const int k = blockIdx.x;
  const size_t lo = k ? ((size_t)1 << (k - 1)) : 0, hi = (size_t)1 << k;
  ge_ext acc = ge_identity();
  for (size_t j = lo + threadIdx.x; j < hi && j < nb; j += 256) {
    acc = ge_add(acc, ge_load(xyzt + 4 * j));
  }
  __shared__ ge_ext sh[256];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st) {
      acc = ge_add(acc, sh[threadIdx.x + st]);
      sh[threadIdx.x] = acc;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ge_store(xyzt + 4 * (nb + k), acc);
}
__global__ void gens_sum_scan_kernel(fp* __restrict__ xyzt, size_t nb, int nsum) {
  if (threadIdx.x || blockIdx.x) return;
  ge_ext acc = ge_load(xyzt + 4 * nb);
  for (int k = 1; k < nsum; k++) {
    fp* q = xyzt + 4 * (nb + k);
    acc = ge_add(acc, ge_load(q));
    ge_store(q, acc);
  }
}

// one thread per base: shifts[j][w] = 2^(c*w) * g_j
__global__ __launch_bounds__(64) void gens_shift_kernel(const fp* __restrict__ xyzt, size_t nb, int W, int c,
                                                        ge_ext* __restrict__ shifts) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb) return;
  ge_ext p = ge_load(xyzt + 4 * j);
  for (int w = 0; w < W; w++) {
    ge_store(shifts + j * W + w, p);
    for (int k = 0; k < c; k++) p = ge_double(p);
  }
}

// one thread per (base, window): the E multiples of the shifted base, normalised to affine with
// one inversion per thread (Montgomery's trick): forward pass stores X,Y,Z in the entry slots and
// the running product of the Z's in `prefix`; the backward pass peels the inverses off.
__global__ __launch_bounds__(64) void gens_table_kernel(const ge_ext* __restrict__ shifts, size_t nb, int W, int E,
                                                        fp* __restrict__ table, int s32, fp* __restrict__ prefix) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nb * (size_t)W) return;
  size_t j = idx / W;
  int w = (int)(idx % W);
  const ge_ext p = ge_load(shifts + j * W + w);
  ge_cached pc = ge_to_cached(p);
  fp* out = table + (((size_t)w * nb + j) * E) * (size_t)s32;  // slot k at out + k * s32: {ypx, ymx, xy2d}
  fp* pre = prefix + ((size_t)w * nb + j) * E;
  ge_ext q = p;
  fp run = fp_one();
  for (int k = 0; k < E; k++) {
    fp_store(out + (size_t)k * s32, q.X); fp_store(out + (size_t)k * s32 + 1, q.Y); fp_store(out + (size_t)k * s32 + 2, q.Z);
    run = fp_mul(run, q.Z);
    fp_store(pre + k, run);
    if (k + 1 < E) q = ge_add_cached(q, pc);
  }
  fp acc = fp_invert(run);
  const fp d2 = FP_D2();
  for (int k = E - 1; k >= 0; k--) {
    fp X = fp_load(out + (size_t)k * s32), Y = fp_load(out + (size_t)k * s32 + 1), Z = fp_load(out + (size_t)k * s32 + 2);
    fp zinv = (k > 0) ? fp_mul(acc, fp_load(pre + k - 1)) : acc;
    acc = fp_mul(acc, Z);
    fp x = fp_mul(X, zinv), y = fp_mul(Y, zinv);
    fp_store(out + (size_t)k * s32, fp_add(y, x));
    fp_store(out + (size_t)k * s32 + 1, fp_sub(y, x));
    fp_store(out + (size_t)k * s32 + 2, fp_mul(fp_mul(x, y), d2));
  }
}

// ---- scalar handling --------------------------------------------------------------------

// accumulate s * g_j into acc through the window table; s canonical, non-zero.  One walk for both accumulators: ge_ext
// (ge_add_niels), and the ten-limb form (fp10_dev.h: the product of two field elements is 142 VALU instructions instead of 197
// and the additions between products carry nothing) of the row-commitment kernels, where a lane adds hundreds of table entries
// to one accumulator; the entries stay in the packed 96-byte form in HBM.  The digits: fq_fold_sign, then walk_digit per window.
__device__ __forceinline__ ge_ext acc_add_niels(const ge_ext& a, const ge_niels& e, bool neg) { return ge_add_niels(a, e, neg); }
__device__ __forceinline__ ge10 acc_add_niels(const ge10& a, const ge_niels& e, bool neg) { return ge10_add_niels(a, e, neg); }
template <class Acc>
__device__ __forceinline__ void table_mul_acc(Acc& acc, fq s, const TableView& tv, size_t j) {
  const bool flip = fq_fold_sign(s);
  const TableSeg sg = table_seg(tv, j);
  uint32_t carry = 0;
  // software pipeline: the (random, 96-byte) table entry of window w+1 is requested before the
  // 7-multiply add of window w, so the gather latency hides behind arithmetic
  ge_niels e_cur;
  bool have_cur = false, neg_cur = false;
#pragma unroll 1
  for (int w = 0; w <= sg.W; w++) {
    ge_niels e_next;
    bool have_next = false, neg_next = false;
    if (w < sg.W) {
      const uint32_t mag = walk_digit(fq_take_window(s, carry, (uint32_t)sg.c), (uint32_t)sg.c, flip, carry, neg_next);
      if (mag != 0) {
        e_next = ge_load(sg.entry(w, mag - 1));
        have_next = true;
      }
    }
    if (have_cur) acc = acc_add_niels(acc, e_cur, neg_cur);
    e_cur = e_next;
    have_cur = have_next;
    neg_cur = neg_next;
  }
}

// accumulator of the row kernels, in the ten-limb form (fp10_dev.h)
struct RowAcc {
  ge10 a = ge10_identity();
  __device__ __forceinline__ void mul_acc(const fq& s, const TableView& tv, size_t j) { table_mul_acc(a, s, tv, j); }
  __device__ __forceinline__ void add_cached(const ge_cached& q) { a = ge10_add_cached(a, q); }
  __device__ __forceinline__ ge_ext ext() const { return ge10_to_ext(a); }
};

// windows [w0, w1) of s * g_j (sg = table_seg(tv, j)), for the kernels that split one scalar over several lanes
__device__ __forceinline__ void table_mul_acc_range(ge_ext& acc, const fq& s_in, const TableSeg& sg, int w0, int w1) {
  fq s = s_in;
  const bool flip = fq_fold_sign(s);
  uint32_t carry = carry_into(s, w0, sg.c);
#pragma unroll 1
  for (int w = w0; w < w1; w++) {
    bool neg;
    const uint32_t mag = walk_digit(scalar_digit(s, w, sg.c) + carry, (uint32_t)sg.c, flip, carry, neg);
    if (mag != 0) acc = ge_add_niels(acc, ge_load(sg.entry(w, mag - 1)), neg);
  }
}

// ---- row-batched commitment -------------------------------------------------------------

constexpr int kMsmBlock = 256;
// extra dynamic LDS of the row-commitment kernels when other contexts prove on the device (vpin_ctx_set_shared_device): with
// it one workgroup per CU instead of three (a wave per SIMD), the rest of every CU stays with the other lanes' kernels
constexpr unsigned kSharedPad = 40000u;
constexpr int kSeg = 8192;  // scalars per compaction segment (uint16 indices, 16 KiB of LDS)

// "These rows of this polynomial", as every row kernel takes them: launch row i (a workgroup's blockIdx.x, or an entry of the
// strip list) is row row_base + i * row_step of the polynomial; its ncols scalars go on the generators [0, ncols), its n_extra
// extra scalars (blinds) on the bases [extra_base0, extra_base0 + n_extra).  Results are indexed by the launch row.
struct RowArgs {
  const fq* Z;
  size_t stride, ncols;  // scalars between two rows of Z, scalars per row
  const fq* extra;       // [launch rows][n_extra]
  int n_extra;
  size_t extra_base0;
  size_t row_base, row_step;
  int z_compact;  // Z holds only this launch's rows, densely (a rank's rows of a split commitment gathered on their own)
  __device__ __forceinline__ size_t row(size_t i) const { return row_base + i * row_step; }  // row of the polynomial
  __device__ __forceinline__ const fq* scalars(size_t i) const { return Z + (z_compact ? i : row(i)) * stride; }
  __device__ __forceinline__ const fq* extras(size_t i) const { return extra + i * (size_t)n_extra; }
};

// ---- row commitment with one repeated scalar per row taken out (the derefs commitment) ---------------------------------
// Derefs (sparse_mlpoly.rs:267-283): the col-derefs vector of matrix m is E_ry[col_m[i]], and in an R1CS the column of the
// constant 1 carries a large share of a matrix's entries (37 % of B, 8 % of C for vPIN's point-mult gadget: one in twelve
// scalars of the whole derefs polynomial).  All those entries hold the SAME scalar v = E_ry[hot]: with T_j = v * g_j
// computed once per proof (R table walks), an entry at column j of a row costs one point addition instead of a table walk
// of W.  The entries are recognised by their column INDEX (the decommitment's index slices), never by value.
struct HotRows {
  const uint32_t* idx[3];   // col index slice of matrix m (N entries, the order of the polynomial)
  uint32_t hot[3];          // the hot column of matrix m, 0xffffffff: none
  const ge_cached* T[3];    // T[m][j] = E_ry[hot[m]] * g_j, j < ncols
  size_t row0, rows_per_vec;  // matrix m's vector occupies rows [row0 + m*rows_per_vec, row0 + (m+1)*rows_per_vec)
};
// the hot column of one row: entry j of the row is hot when idx && idx[j] == hot, and then costs T[j]; idx == nullptr: none
// (HotRows{}, a row outside the three vectors, a matrix without a hot column)
struct HotCol {
  const uint32_t* idx = nullptr;
  const ge_cached* T = nullptr;
  uint32_t hot = 0xffffffffu;
  __device__ __forceinline__ bool at(size_t j) const { return idx && idx[j] == hot; }
};
__device__ __forceinline__ HotCol hot_column(const HotRows& hr, size_t row, size_t ncols) {
  HotCol h;
  if (hr.rows_per_vec && row >= hr.row0 && row < hr.row0 + 3 * hr.rows_per_vec) {
    const size_t m = (row - hr.row0) / hr.rows_per_vec;
    if (hr.hot[m] != 0xffffffffu) {
      h.hot = hr.hot[m];
      h.T = hr.T[m];
      h.idx = hr.idx[m] + (row - hr.row0 - m * hr.rows_per_vec) * ncols;
    }
  }
  return h;
}

// A row of one repeated scalar s (padding tails) is s * (g_0 + ... + g_{ncols-1}) from the prefix-sum base (see
// gens_sum_kernel).  The test, the same answer in every lane of the workgroup, all of which call it.  Three
// probes keep ordinary rows from paying for the full comparison pass.
__device__ __forceinline__ bool row_is_constant(const fq* zr, size_t ncols, const TableView& tv) {
  if (!(ncols >= 256 && (ncols & (ncols - 1)) == 0 && ((size_t)1 << (tv.nbt - tv.sum0 - 1)) >= ncols)) return false;
  const fq first = fq_load(zr);
  if (!(fq_eq(first, fq_load(zr + 1)) && fq_eq(first, fq_load(zr + ncols / 2)) && fq_eq(first, fq_load(zr + ncols - 1)))) return false;
  int same = 1;
  for (size_t j = threadIdx.x; j < ncols; j += kMsmBlock) same &= fq_eq(first, fq_load(zr + j)) ? 1 : 0;
  return __syncthreads_and(same) != 0;
}
// the table base of S_k for a constant row of ncols = 2^k scalars
__device__ __forceinline__ size_t constant_row_base(const TableView& tv, size_t ncols) {
  return tv.sum0 + (size_t)(63 - __builtin_clzll((unsigned long long)ncols));
}
// The constant row's point, for lane 0: s * S_k (s = the row's first scalar) plus the n_extra extras of launch row i (ra.n_extra, or a literal 0 in a kernel
// that takes none).  With column chunks every chunk sees the same row: the first one owns it, the others add nothing (the identity).
__device__ __forceinline__ ge_ext constant_row_point(const RowArgs& ra, size_t i, const TableView& tv, int n_extra) {
  RowAcc acc;
  if (blockIdx.y == 0) {
    const fq first = fq_load(ra.scalars(i));
    if (!fq_is_zero(first)) acc.mul_acc(fq_from_mont(first), tv, constant_row_base(tv, ra.ncols));
    for (int e = 0; e < n_extra; e++) {
      const fq x = fq_load(ra.extras(i) + e);
      if (!fq_is_zero(x)) acc.mul_acc(fq_from_mont(x), tv, ra.extra_base0 + e);
    }
  }
  return acc.ext();
}

// the end of a row workgroup: the lanes' partial sums through the LDS tree, lane 0 stores the sum to *o
__device__ __forceinline__ void row_workgroup_end(ge_ext* sh, const ge_ext& a, ge_ext* o) {
  sh[threadIdx.x] = a;
  __syncthreads();
  ge_tree_quad(sh, kMsmBlock);
  if (threadIdx.x == 0) {
    const ge_ext av = sh[0];
    ge_store(o, av);
  }
}

// T[j] = v * g_j for j < n (*vp = v in Montgomery form, read on the device: no round trip), as cached points
__global__ __launch_bounds__(64) void scalar_times_bases_kernel(const fq* __restrict__ vp, size_t n, TableView tv,
                                                                ge_cached* __restrict__ T) {
  const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  const fq v = fq_load(vp);
  ge_ext acc = ge_identity();
  if (!fq_is_zero(v)) table_mul_acc(acc, fq_from_mont(v), tv, j);
  ge_store(T + j, ge_to_cached(acc));
}

// One workgroup per (row, column chunk): out[launch row * gridDim.y + blockIdx.y] = sum_j s[row][j] * g_j over the chunk
// (extended coords).  kHot = false (msm_rows_kernel): the row's extras are appended to its columns.  kHot = true
// (msm_rows_hot_kernel): no extras; the row's hot-column entries are added from hr's T instead of walked, and
// strip_flag[launch row] != 0 says that the table walks of this row are msm_strip_kernel's: only its hot entries are added.
template <bool kHot>
__device__ __forceinline__ void msm_rows_body(const RowArgs& ra, const TableView& tv, const HotRows& hr, ge_ext* __restrict__ out,
                                              const uint8_t* __restrict__ strip_flag) {
  const size_t i = blockIdx.x;
  const fq* zr = ra.scalars(i);
  const size_t ncols = ra.ncols;
  const bool hot_only = kHot && strip_flag && strip_flag[i];
  if (!hot_only && row_is_constant(zr, ncols, tv)) {
    if (threadIdx.x == 0) {
      const ge_ext av = constant_row_point(ra, i, tv, kHot ? 0 : ra.n_extra);
      ge_store(out + i * gridDim.y + blockIdx.y, av);
    }
    return;
  }
  HotCol hc;
  if (kHot) hc = hot_column(hr, ra.row(i), ncols);
  const fq* xr = kHot ? nullptr : ra.extras(i);
  const size_t total = kHot ? ncols : ncols + (size_t)ra.n_extra;
  // gridDim.y column chunks per row: few-row MSMs need more than `rows` workgroups, and a row of 16384 full-width scalars is
  // ~11 ms of one workgroup: a commitment (or a rank's share of one) of a few waves of such workgroups ends in a long, mostly
  // idle tail
  const size_t per = (total + gridDim.y - 1) / gridDim.y;
  const size_t j0 = (size_t)blockIdx.y * per, j1 = (j0 + per < total) ? j0 + per : total;
  // The witness is ~40% zeros in irregular positions; lanes that met a zero scalar would idle
  // while their wave-mates do 32 table adds.  So each segment is first compacted: the indices
  // of its non-zero scalars go to an LDS list (order is irrelevant: the group is commutative),
  // then the threads stride over the dense list.
  // One LDS list, two ends: ordinary non-zero scalars from the front, hot entries from the back.
  __shared__ uint16_t list[kSeg];
  __shared__ uint32_t n_front, n_back;
  RowAcc acc;
  for (size_t seg = j0; seg < j1; seg += kSeg) {
    const size_t seg_end = (seg + kSeg < j1) ? seg + kSeg : j1;
    if (threadIdx.x == 0) { n_front = 0; if (kHot) n_back = 0; }
    __syncthreads();
    for (size_t j = seg + threadIdx.x; j < seg_end; j += kMsmBlock) {
      if (fq_is_zero(fq_load((kHot || j < ncols) ? zr + j : xr + (j - ncols)))) continue;
      if (kHot && hc.at(j)) list[kSeg - 1 - atomicAdd(&n_back, 1u)] = (uint16_t)(j - seg);
      else if (!hot_only) list[atomicAdd(&n_front, 1u)] = (uint16_t)(j - seg);
    }
    __syncthreads();
    const uint32_t nf = n_front, nb = kHot ? n_back : 0u;
    for (uint32_t k = threadIdx.x; k < nf; k += kMsmBlock) {
      const size_t j = seg + list[k];
      fq sc;
      size_t base;
      if (kHot || j < ncols) { sc = fq_load(zr + j); base = j; }
      else { sc = fq_load(xr + (j - ncols)); base = ra.extra_base0 + (j - ncols); }
      acc.mul_acc(fq_from_mont(sc), tv, base);
    }
    if (kHot)
      for (uint32_t k = threadIdx.x; k < nb; k += kMsmBlock) acc.add_cached(ge_load(hc.T + seg + list[kSeg - 1 - k]));
    __syncthreads();
  }
  __shared__ ge_ext sh[kMsmBlock];
  row_workgroup_end(sh, acc.ext(), out + i * gridDim.y + blockIdx.y);
}

__global__ __launch_bounds__(kMsmBlock, 3) void msm_rows_kernel(RowArgs ra, TableView tv, ge_ext* __restrict__ out) {
  msm_rows_body<false>(ra, tv, HotRows{}, out, nullptr);
}
__global__ __launch_bounds__(kMsmBlock, 3) void msm_rows_hot_kernel(RowArgs ra, TableView tv, HotRows hr, ge_ext* __restrict__ out,
                                                                    const uint8_t* __restrict__ strip_flag) {
  msm_rows_body<true>(ra, tv, hr, out, strip_flag);
}

// ---- row per lane: the table walks of a LARGE commitment out of L2 instead of HBM -------------------------------------------
// Under the row kernels above the chip sits at its power limit: tools/ubench_msm_variants (profiles/r04_ubench_msm_variants.txt)
// measured the point addition alone at 31.3 G/s and 2.39 GHz, the same loop with the table walk's gathers at 22.6 G/s with
// the clock down to 1.79 GHz at 1390 W -- a 96-byte entry out of a 71 GB table costs about as much energy as a third of the
// addition it feeds.  Every row of a commitment walks the SAME generators, so the fix is to make thousands of lanes want the
// same 196 KB block (one window of one generator: 2048 multiples) at the same moment: here a LANE is a row, a workgroup is
// 256 rows, and all workgroups of a "strip" (a run of ncols / S generators) step through (generator, window) together, each
// lane adding the multiple its own digit selects.  A block is then read ~rows / 2048 times within microseconds, i.e. once
// from HBM and otherwise from L2 (workgroup b works on strip b mod S; workgroups are dealt round-robin to the 8 XCDs and S is a
// multiple of 8, so a strip stays on one XCD's L2).  Measured on the synthetic walk: 26.4 G additions/s at 2.06 GHz.
// Rows whose walks are irregular stay with msm_rows_hot_kernel (constant rows, rows with many zero scalars or hot entries:
// a lane that skips idles while its wave-mates walk); the hot entries of the rows taken here are added by that kernel too
// (hot_only), and strip_combine_kernel sums the S partial points of a row into it.

// flag[i] = 1: row i of the launch goes to msm_strip_kernel
__global__ __launch_bounds__(kMsmBlock) void strip_classify_kernel(RowArgs ra, HotRows hr, uint8_t* __restrict__ flag) {
  const size_t ncols = ra.ncols;
  const fq* zr = ra.scalars(blockIdx.x);
  const HotCol hc = hot_column(hr, ra.row(blockIdx.x), ncols);
  const fq first = fq_load(zr);
  int same = 1;
  uint32_t skipped = 0;
  for (size_t j = threadIdx.x; j < ncols; j += kMsmBlock) {
    const fq v = fq_load(zr + j);
    same &= fq_eq(first, v) ? 1 : 0;
    skipped += (fq_is_zero(v) || hc.at(j)) ? 1u : 0u;
  }
  __shared__ uint32_t sh[kMsmBlock];
  sh[threadIdx.x] = skipped;
  const int all_same = __syncthreads_and(same);
  for (int st = kMsmBlock / 2; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) flag[blockIdx.x] = (!all_same && sh[0] * 8 <= ncols) ? 1 : 0;
}

// list = the flagged rows in ascending order, *count = how many (one workgroup of 1024 threads; nrows <= 2^20)
__global__ __launch_bounds__(1024) void strip_list_kernel(const uint8_t* __restrict__ flag, size_t nrows, uint32_t* __restrict__ list,
                                                           uint32_t* __restrict__ count) {
  __shared__ uint32_t base[1024];
  const size_t per = (nrows + 1023) / 1024, r0 = (size_t)threadIdx.x * per, r1 = r0 + per < nrows ? r0 + per : nrows;
  uint32_t n = 0;
  for (size_t r = r0; r < r1; r++) n += flag[r] ? 1u : 0u;
  base[threadIdx.x] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < 1024; t++) { const uint32_t v = base[t]; base[t] = run; run += v; }
    *count = run;
  }
  __syncthreads();
  uint32_t o = base[threadIdx.x];
  for (size_t r = r0; r < r1; r++)
    if (flag[r]) list[o++] = (uint32_t)r;
}

// the listed rows from n_use on go back to the row kernel: flags cleared, *count = n_use (launched after strip_list_kernel)
__global__ __launch_bounds__(256) void strip_trim_kernel(const uint32_t* __restrict__ list, uint32_t* __restrict__ count, uint32_t n_use,
                                                          uint32_t n_all, uint8_t* __restrict__ flag) {
  const uint32_t li = n_use + blockIdx.x * 256 + threadIdx.x;
  if (li < n_all) flag[list[li]] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count = n_use;
}

// parts[li * S + s] = sum over strip s of the table walks of listed row li (ten-limb accumulator)
__global__ __launch_bounds__(kMsmBlock, 3) void msm_strip_kernel(RowArgs ra, TableView tv, HotRows hr, const uint32_t* __restrict__ list,
                                                                  const uint32_t* __restrict__ list_count, int S,
                                                                  ge_ext* __restrict__ parts, uint32_t* __restrict__ sync, int lag) {
  const uint32_t n = *list_count;
  const uint32_t s = blockIdx.x % (uint32_t)S, grp = blockIdx.x / (uint32_t)S;
  if (grp * kMsmBlock >= n) return;
  const uint32_t li = grp * kMsmBlock + threadIdx.x;
  const bool live = li < n;
  const uint32_t i = list[live ? li : n - 1];  // this lane's launch row
  const size_t ncols = ra.ncols;
  const fq* zr = ra.scalars(i);
  const HotCol hc = hot_column(hr, ra.row(i), ncols);
  const size_t per = (ncols + (size_t)S - 1) / (size_t)S, j0 = (size_t)s * per, j1 = j0 + per < ncols ? j0 + per : ncols;
  ge10 acc = ge10_identity();
  // Keeping a strip's workgroups in step (sync != nullptr): a workgroup counts every generator it has finished, and starts
  // generator j only when all `groups` workgroups of its strip have finished generator j - lag -- the L2 then holds the few
  // blocks between the slowest and the fastest workgroup instead of losing them.  All workgroups of the launch are resident
  // (2 or 3 per CU by construction); should they not be (another stream on the device), the bounded wait gives up and the
  // workgroup runs on unsynchronised -- the result does not depend on the order.
  const uint32_t groups = (n + kMsmBlock - 1) / kMsmBlock;
  uint32_t* my_sync = sync ? sync + (size_t)s * (per + 1) : nullptr;
  __shared__ int sh_nosync;
  if (threadIdx.x == 0) sh_nosync = 0;
  __syncthreads();
  for (size_t j = j0; j < j1; j++) {
    if (my_sync && j - j0 >= (size_t)lag) {
      if (threadIdx.x == 0 && !sh_nosync) {
        long spin = 0;
        while (__hip_atomic_load(my_sync + (j - j0 - (size_t)lag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < groups)
          if (++spin > (1L << 16)) { sh_nosync = 1; break; }  // ~0.1 s; a legitimate wait is one generator's walk (~150 us)
      }
      __syncthreads();
    }
    fq v = fq_load(zr + j);
    const bool act = live && !fq_is_zero(v) && !hc.at(j);
    if (__builtin_amdgcn_ballot_w64(act) != 0) {  // somebody in the wave walks this generator
      fq sc = fq_from_mont(v);
      if (!act) sc = fq_zero();  // all digits zero: the walk below adds nothing for this lane, in step with its wave-mates
      table_mul_acc(acc, sc, tv, j);
    }
    if (my_sync) {
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_fetch_add(my_sync + (j - j0), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (live) {
    const ge_ext av = ge10_to_ext(acc);
    ge_store(parts + (size_t)li * (size_t)S + s, av);
  }
}

// out[list[li]] += sum_s parts[li * S + s]
__global__ __launch_bounds__(64) void strip_combine_kernel(const ge_ext* __restrict__ parts, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ list_count, int S, ge_ext* __restrict__ out) {
  const uint32_t li = blockIdx.x * 64 + threadIdx.x;
  if (li >= *list_count) return;
  ge_ext* o = out + list[li];
  ge_ext a = ge_load(o);
  for (int s = 0; s < S; s++) a = ge_add(a, ge_load(parts + (size_t)li * (size_t)S + s));
  ge_store(o, a);
}

// ---- row commitment over the row table: one accumulator per lane and WINDOW ------------------------------------------------
// Lane l of a workgroup owns window l mod W and accumulates A_w = sum_j digit_w(s_j) g_j over the workgroup's columns from the
// one-window table T1[j][k] = (k+1) g_j; msm_rows_finish_kernel then forms sum_w 2^(c w) A_w per row (c (W-1) doublings per
// ROW instead of a table of every shifted generator: 16-bit windows fit where the multi-window table stops at 12, and a folded
// scalar is 16 additions instead of 21).  Per segment of `segn` columns:
//   phase 1: every scalar is read, converted out of Montgomery form, sign-folded and recoded ONCE into W signed digits, which go
//            to LDS as dig[w][column]: magnitude - 1 in bits 0..14, sign in bit 15, kNoDigit for a zero digit (and for every
//            digit of a zero scalar or a hot-column entry);
//   phase 2: the lanes of window w stride over dig[w][.]; a lane skips zero digits on its own (a short LDS scan, not an idle
//            addition), and the entry of its next digit is requested before the current addition, as in table_mul_acc.
// The hot-column entries of a derefs row are added afterwards by ALL lanes (add_cached from T[m], as in msm_rows_hot_kernel)
// and tree-summed into window 0; a constant row is s * S_k over the multi-window table, as before.  LDS: 48 KiB of digits,
// which the two reductions at the end reuse -- what msm_rows_kernel takes, so msm_lds_pad keeps its meaning.
constexpr int kRowLdsBytes = 48 * 1024;
// columns per segment for W windows (host and device agree on it)
static inline int row_segment(int W) { return ((kRowLdsBytes / 2) / W) & ~3; }

__global__ __launch_bounds__(kMsmBlock, 3) void msm_rows_win_kernel(RowArgs ra, TableView tv, RowTable rt, HotRows hr, int segn,
                                                                     ge_ext* __restrict__ parts) {
  const size_t i = blockIdx.x;  // parts[] is indexed by the launch row
  const size_t ncols = ra.ncols, extra_base0 = ra.extra_base0;
  const fq* zr = ra.scalars(i);
  const fq* xr = ra.extras(i);
  const int W = rt.W;
  ge_ext* o = parts + (i * gridDim.y + blockIdx.y) * (size_t)W;  // the W window sums of this (row, chunk)
  __shared__ __align__(16) unsigned char lds[kRowLdsBytes];
  __shared__ uint32_t n_hot;
  // a constant row: s * S_k over the multi-window table into window 0, as in msm_rows_kernel
  if (row_is_constant(zr, ncols, tv)) {
    if (threadIdx.x == 0) ge_store(o, constant_row_point(ra, i, tv, ra.n_extra));
    else if ((int)threadIdx.x < W) ge_store_identity(o + threadIdx.x);
    return;
  }
  const HotCol hc = hot_column(hr, ra.row(i), ncols);
  const size_t total = ncols + (size_t)ra.n_extra;
  const size_t per = (total + gridDim.y - 1) / gridDim.y;
  const size_t j0 = (size_t)blockIdx.y * per, j1 = (j0 + per < total) ? j0 + per : total;
  // this lane's window, its rank among the window's lanes and their number
  const int w = (int)threadIdx.x % W, r = (int)threadIdx.x / W, nw = (kMsmBlock - 1 - w + W) / W;
  uint16_t* dig = reinterpret_cast<uint16_t*>(lds);
  ge10 acc = ge10_identity();
  for (size_t seg = j0; seg < j1; seg += (size_t)segn) {
    const uint32_t n = (uint32_t)((seg + (size_t)segn < j1) ? (size_t)segn : j1 - seg);
    for (uint32_t jl = threadIdx.x; jl < n; jl += kMsmBlock) {
      const size_t j = seg + jl;
      fq s = fq_load(j < ncols ? zr + j : xr + (j - ncols));
      const bool live = !fq_is_zero(s) && !(j < ncols && hc.at(j));
      bool flip = false;
      if (live) {
        s = fq_from_mont(s);
        flip = fq_fold_sign(s);
      }
      uint32_t carry = 0;
#pragma unroll 1
      for (int ww = 0; ww < W; ww++) {
        uint16_t d = kNoDigit;
        if (live) d = row_digit(s, carry, rt.c, flip, ww == W - 1);
        dig[(size_t)ww * segn + jl] = d;
      }
    }
    __syncthreads();
    const uint16_t* dg = dig + (size_t)w * segn;
    uint32_t k = (uint32_t)r;
    // the next non-zero digit of this lane's stride: its table entry is requested, false when the list is exhausted
    auto fetch = [&](ge_niels& e, bool& neg) -> bool {
      while (k < n) {
        const uint32_t kk = k;
        k += (uint32_t)nw;
        const uint16_t d = dg[kk];
        if (d != kNoDigit) {
          const size_t j = seg + kk;
          e = ge_load(rt.entry(j < ncols ? j : extra_base0 + (j - ncols), d & 0x7fffu));
          neg = (d >> 15) != 0;
          return true;
        }
      }
      return false;
    };
    ge_niels e_cur;
    bool neg_cur = false;
    bool have_cur = fetch(e_cur, neg_cur);
    while (have_cur) {
      ge_niels e_next;
      bool neg_next = false;
      const bool have_next = fetch(e_next, neg_next);
      acc = ge10_add_niels(acc, e_cur, neg_cur);
      e_cur = e_next;
      neg_cur = neg_next;
      have_cur = have_next;
    }
    __syncthreads();
  }
  // the lanes of each window, summed: sh[w] = A_w of this workgroup
  ge_ext* sh = reinterpret_cast<ge_ext*>(lds);
  sh[threadIdx.x] = ge10_to_ext(acc);
  __syncthreads();
  ge_tree_quad_strided(sh, kMsmBlock, W);
  ge_ext mine = ge_identity();
  if ((int)threadIdx.x < W) mine = sh[threadIdx.x];
  __syncthreads();
  if (hc.idx) {  // uniform over the workgroup: the hot entries of this chunk, all lanes, into window 0
    uint16_t* list = reinterpret_cast<uint16_t*>(lds);
    RowAcc hacc;
    uint32_t any = 0;
    const size_t c1 = j1 < ncols ? j1 : ncols;
    for (size_t seg = j0; seg < c1; seg += kSeg) {
      const size_t seg_end = (seg + kSeg < c1) ? seg + kSeg : c1;
      if (threadIdx.x == 0) n_hot = 0;
      __syncthreads();
      for (size_t j = seg + threadIdx.x; j < seg_end; j += kMsmBlock)
        if (hc.at(j) && !fq_is_zero(fq_load(zr + j))) list[atomicAdd(&n_hot, 1u)] = (uint16_t)(j - seg);
      __syncthreads();
      const uint32_t nh = n_hot;
      any |= nh;
      for (uint32_t kk = threadIdx.x; kk < nh; kk += kMsmBlock) hacc.add_cached(ge_load(hc.T + seg + list[kk]));
      __syncthreads();
    }
    if (any) {  // n_hot is read by every lane between two barriers: uniform
      sh[threadIdx.x] = hacc.ext();
      __syncthreads();
      ge_tree_quad(sh, kMsmBlock);
      if (threadIdx.x == 0) mine = ge_add(mine, sh[0]);
    }
  }
  if ((int)threadIdx.x < W) ge_store(o + threadIdx.x, mine);
}

// out[row] = sum_w 2^(c w) * (sum over the row's chunks of window w's partial point): one lane per row.  The chunk sums are
// written over the first chunk's slots, then Horner runs from the top window down (ge10_horner_windows).
__global__ __launch_bounds__(64) void msm_rows_finish_kernel(ge_ext* __restrict__ parts, size_t rows, int chunks, int W, int c,
                                                             ge_ext* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  ge_ext* p = parts + i * (size_t)chunks * (size_t)W;
  if (chunks > 1)
    for (int w = 0; w < W; w++) {
      ge_ext a = ge_load(p + w);
      for (int k = 1; k < chunks; k++) a = ge_add(a, ge_load(p + (size_t)k * W + w));
      ge_store(p + w, a);
    }
  ge_store(out + i, ge10_to_ext(ge10_horner_windows(p, W, [c](int) { return c; })));
}

// Profiling aid (vpin_prof_enable(ctx, 2)): the affine table additions the row kernels perform for the same arguments --
// non-zero signed digits of every non-zero scalar, one scalar for a constant row -- summed into *count.  The digits are taken
// with the walks' own steps: table_mul_acc's (fq_take_window, walk_digit) ...
__device__ __forceinline__ uint32_t count_digits(fq s, const TableView& tv, size_t j) {
  const bool flip = fq_fold_sign(s);
  const TableSeg sg = table_seg(tv, j);
  uint32_t carry = 0, n = 0;
  bool neg;
  for (int w = 0; w < sg.W; w++) n += walk_digit(fq_take_window(s, carry, (uint32_t)sg.c), (uint32_t)sg.c, flip, carry, neg) != 0;
  return n;
}
// ... and msm_rows_win_kernel's, which recodes a scalar into W digits of c bits (row_digit)
__device__ __forceinline__ uint32_t count_digits_row(fq s, int c, int W) {
  const bool flip = fq_fold_sign(s);
  uint32_t carry = 0, n = 0;
  for (int w = 0; w < W; w++) n += row_digit(s, carry, c, flip, w == W - 1) != kNoDigit;
  return n;
}
// hr: the hot-column entries are not table additions.  c_row != 0: the launch goes to msm_rows_win_kernel with W_row windows of
// c_row bits (constant rows stay on the multi-window table)
__global__ __launch_bounds__(kMsmBlock) void msm_count_adds_kernel(RowArgs ra, TableView tv, HotRows hr, int c_row, int W_row,
                                                                   unsigned long long* __restrict__ count) {
  const size_t i = blockIdx.x, ncols = ra.ncols;
  const fq* zr = ra.scalars(i);
  const HotCol hc = hot_column(hr, ra.row(i), ncols);
  uint32_t n = 0;
  const bool constant = row_is_constant(zr, ncols, tv);
  if (constant && threadIdx.x == 0) {
    const fq first = fq_load(zr);
    if (!fq_is_zero(first)) n += count_digits(fq_from_mont(first), tv, constant_row_base(tv, ncols));
  }
  if (!constant)
    for (size_t j = threadIdx.x; j < ncols; j += kMsmBlock) {
      const fq s = fq_load(zr + j);
      if (!fq_is_zero(s) && !hc.at(j)) n += c_row ? count_digits_row(fq_from_mont(s), c_row, W_row) : count_digits(fq_from_mont(s), tv, j);
    }
  for (int e = threadIdx.x; e < ra.n_extra; e += kMsmBlock) {
    const fq x = fq_load(ra.extras(i) + e);
    if (!fq_is_zero(x)) n += (c_row && !constant) ? count_digits_row(fq_from_mont(x), c_row, W_row) : count_digits(fq_from_mont(x), tv, ra.extra_base0 + e);
  }
  __shared__ uint32_t sh[kMsmBlock];
  sh[threadIdx.x] = n;
  __syncthreads();
  for (int st = kMsmBlock / 2; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0]) atomicAdd(count, (unsigned long long)sh[0]);
}

// Few-row MSMs (the evaluation proof's bullet rounds: 1-2 rows of R+2 scalars) are latency bound,
// so the 32 windows of a scalar are spread over 8 threads (4 table adds each) and a 256-thread
// workgroup covers 32 scalars; the per-workgroup partial points go back to the host, which adds
// the few dozen partials and compresses (microseconds on a CPU core, ~0.4 ms as a GPU tail).
constexpr int kWideScalars = 32;  // scalars per workgroup and pass
// Q passes per workgroup: 32 Q scalars each.  Long rows (>= 8192 scalars) take Q = 4: the 255 tree additions of a
// workgroup are then spread over four times as many table additions, and a row needs a quarter of the workgroups.
template <int Q>
__global__ __launch_bounds__(kMsmBlock) void msm_wide_kernel(const fq* __restrict__ S, size_t ncols, TableView tv,
                                                             fp* __restrict__ parts_xyzt) {
  const size_t row = blockIdx.y;
  const int grp = threadIdx.x & 7;
  ge_ext acc = ge_identity();
#pragma unroll 1
  for (int q = 0; q < Q; q++) {
    const size_t j = ((size_t)blockIdx.x * Q + q) * kWideScalars + (threadIdx.x >> 3);
    if (j < ncols) {
      fq s = fq_load(S + row * ncols + j);
      if (!fq_is_zero(s)) {
        const TableSeg sg = table_seg(tv, j);
        const int wpg = (sg.W + 7) / 8;  // this lane's windows [grp*wpg, (grp+1)*wpg)
        int w0 = grp * wpg, w1 = (w0 + wpg < sg.W) ? w0 + wpg : sg.W;
        if (w0 < w1) table_mul_acc_range(acc, fq_from_mont(s), sg, w0, w1);
      }
    }
  }
  __shared__ ge_ext sh[kMsmBlock];
  sh[threadIdx.x] = acc;
  __syncthreads();
  ge_tree_quad(sh, kMsmBlock);
  if (threadIdx.x == 0) {
    acc = sh[0];
    ge_store_frozen(parts_xyzt + 4 * (row * gridDim.x + blockIdx.x), acc);
  }
}


// ---- one kernel per round of the bullet reduction (host side: bullet.hip) ------------------------------------------
// BulletReductionProof::prove (nizk/bullet.rs:32-132), round with half length n, everything the device does for it:
//   * fold the previous round's challenge into a, b and the generator coefficients s_j (bullet.rs:99-109);
//   * L = <a_L, G_R>, R = <a_R, G_L> over the stream generators as fixed-base MSMs with scalars a'[.] * s'_j
//     (bullet.hip: G is never folded) -- the last nmsm workgroups, 32 generators each, eight lanes per scalar;
//   * the cross inner products c_L = <a_L, b_R>, c_R = <a_R, b_L> and the folded a, b for the next round -- the first
//     workgroups of the grid, published through the pinned mailbox so the host forms c*Q + blind*H while the MSM runs.
// No workgroup reads what another one writes (a, b are double-buffered; s_j belongs to its eight lanes), so one launch
// replaces the fold, rows and MSM launches and both copies of a round.  finish = 1: the last fold only --
// g_hat = sum_j s_j g_j, x_hat, a_hat.
struct BulletStep {
  const fq* a_prev; const fq* b_prev;  // live length 4n when fold (2n otherwise)
  fq* a_next; fq* b_next;              // live length 2n after this launch
  fq* sj;                              // [R]
  size_t n, R;
  int fold, finish, nmsm;
  fq u, u_inv;                         // the previous round's challenge (fold / finish)
  fp* parts;                           // pinned: [2][nmsm] points X|Y|Z|T, row 0 = L, row 1 = R
  uint32_t* up;                        // pinned: two scalars per inner-product workgroup, 12 words each
  uint32_t seq;
};

__global__ __launch_bounds__(kMsmBlock) void bullet_step_kernel(BulletStep a, TableView tv) {
  const size_t n = a.n;
  // the inner-product workgroups come first in the grid: they are dispatched first, so the host has c_L, c_R (and forms
  // c*Q + blind*H) while the MSM workgroups, more than fit the device at once for the longest rows, are still running
  const int nip = (int)gridDim.x - a.nmsm;
  if ((int)blockIdx.x < nip) {
    // ---- inner products + the folded vectors ----
    const int ib = (int)blockIdx.x;
    const size_t i = (size_t)ib * kMsmBlock + threadIdx.x;
    fq pl = fq_zero(), pr = fq_zero();
    if (a.finish) {
      if (ib == 0 && threadIdx.x == 0) {
        pl = fq_add(fq_mul(fq_load(a.a_prev), a.u), fq_mul(a.u_inv, fq_load(a.a_prev + 1)));  // x_hat
        pr = fq_add(fq_mul(fq_load(a.b_prev), a.u_inv), fq_mul(a.u, fq_load(a.b_prev + 1)));  // a_hat
      }
    } else if (i < n) {
      fq a0, a1, b0, b1;
      if (a.fold) {
        a0 = fq_add(fq_mul(fq_load(a.a_prev + i), a.u), fq_mul(a.u_inv, fq_load(a.a_prev + 2 * n + i)));
        a1 = fq_add(fq_mul(fq_load(a.a_prev + n + i), a.u), fq_mul(a.u_inv, fq_load(a.a_prev + 3 * n + i)));
        b0 = fq_add(fq_mul(fq_load(a.b_prev + i), a.u_inv), fq_mul(a.u, fq_load(a.b_prev + 2 * n + i)));
        b1 = fq_add(fq_mul(fq_load(a.b_prev + n + i), a.u_inv), fq_mul(a.u, fq_load(a.b_prev + 3 * n + i)));
      } else {
        a0 = fq_load(a.a_prev + i); a1 = fq_load(a.a_prev + n + i);
        b0 = fq_load(a.b_prev + i); b1 = fq_load(a.b_prev + n + i);
      }
      fq_store(a.a_next + i, a0); fq_store(a.a_next + n + i, a1);
      fq_store(a.b_next + i, b0); fq_store(a.b_next + n + i, b1);
      pl = fq_mul(a0, b1);
      pr = fq_mul(a1, b0);
    }
    __shared__ fq shp[kMsmBlock / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    pl = fq_wave_sum(pl);
    pr = fq_wave_sum(pr);
    if (lane == 0) { shp[wave][0] = pl; shp[wave][1] = pr; }
    __syncthreads();
    if (threadIdx.x < 2) {
      fq t = shp[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kMsmBlock / 64; w++) t = fq_add(t, shp[w][threadIdx.x]);
      publish_scalar(a.up + (2 * (size_t)ib + threadIdx.x) * 12, t, a.seq);
    }
    return;
  }
  // ---- the round's MSM: 32 generators per workgroup, the W windows of a scalar over eight lanes ----
  const int g = threadIdx.x >> 3, grp = threadIdx.x & 7;
  const size_t blk = (size_t)blockIdx.x - nip;  // MSM workgroup index
  const size_t j = blk * kWideScalars + g;
  ge_ext acc = ge_identity();
  if (j < a.R) {
    fq sc = fq_load(a.sj + j);
    if (a.fold || a.finish) {
      const size_t hp = a.finish ? 1 : 2 * n;  // half length of the vectors the challenge folded
      sc = fq_mul(sc, ((j & (2 * hp - 1)) < hp) ? a.u_inv : a.u);
      if (grp == 0) fq_store(a.sj + j, sc);  // the eight lanes of j read s_j in the same instruction, before this store
    }
    if (!a.finish) {
      const size_t pos = j & (2 * n - 1);
      const size_t idx = pos >= n ? pos - n : n + pos;  // L: a_L[pos - n] on G_R; R: a_R[pos] on G_L
      fq av = a.fold ? fq_add(fq_mul(fq_load(a.a_prev + idx), a.u), fq_mul(a.u_inv, fq_load(a.a_prev + 2 * n + idx)))
                     : fq_load(a.a_prev + idx);
      sc = fq_mul(av, sc);
    }
    if (!fq_is_zero(sc)) {
      const TableSeg sg = table_seg(tv, j);
      const int wpg = (sg.W + 7) / 8;
      const int w0 = grp * wpg, w1 = (w0 + wpg < sg.W) ? w0 + wpg : sg.W;
      if (w0 < w1) table_mul_acc_range(acc, fq_from_mont(sc), sg, w0, w1);
    }
  }
  // entry grp*32 + g: the first three levels add up the eight lanes of a generator, the rest runs over the generators
  __shared__ ge_ext sh[kMsmBlock];
  sh[grp * kWideScalars + g] = acc;
  __syncthreads();
  // generators alternate between R (pos < n) and L (pos >= n) in runs of n: one side per workgroup while n >= 32
  const int split = (a.finish || n >= (size_t)kWideScalars) ? 0 : (int)n;
  ge_tree_quad(sh, kMsmBlock, split);
  if (threadIdx.x < 2) {
    // thread 0 stores sh[0]; with a split, thread 1 stores sh[split] (the L run)
    const bool first_is_L = a.finish || ((blk * kWideScalars) & (2 * n - 1)) >= n;
    if (threadIdx.x == 0 || split) {
      const ge_ext p = sh[threadIdx.x ? split : 0];
      const int row = threadIdx.x ? 0 : ((split || !first_is_L) ? 1 : 0);
      ge_store_frozen(a.parts + 4 * ((size_t)row * a.nmsm + blk), p);
    }
  }
}

// More than 128 MSM workgroups (R > 4096): their partial points stay on the device and this second launch sums them per side
// in groups of up to 128 (one tree each), so the host still adds at most 8 points per side.  in: [2][nmsm] as
// bullet_step_kernel left them (a workgroup's slot of the side it does not hold is stale), out: [rows][G] in pinned memory.
__global__ __launch_bounds__(kMsmBlock) void bullet_parts_reduce_kernel(const fp* __restrict__ in, int nmsm, size_t n, int finish,
                                                                        fp* __restrict__ out) {
  const int G = gridDim.x, g = blockIdx.x, row = blockIdx.y, per = nmsm / G;
  __shared__ ge_ext sh[kMsmBlock / 2];
  if ((int)threadIdx.x < kMsmBlock / 2) {
    ge_ext p = ge_identity();
    const int b = g * per + (int)threadIdx.x;
    if ((int)threadIdx.x < per) {
      const bool is_L = finish || (((size_t)b * kWideScalars) & (2 * n - 1)) >= n;
      if (finish || n < (size_t)kWideScalars || is_L == (row == 0)) p = ge_load(in + 4 * ((size_t)row * nmsm + b));
    }
    sh[threadIdx.x] = p;
  }
  __syncthreads();
  ge_tree_quad(sh, kMsmBlock / 2);
  if (threadIdx.x == 0) ge_store_frozen(out + 4 * ((size_t)row * G + g), sh[0]);
}

// second stage for long rows: out[row][p] = sum of parts p, p+P, p+2P, ... of that row (frozen X|Y|Z|T)
__global__ __launch_bounds__(64) void parts_reduce_kernel(const fp* __restrict__ in, size_t rows, size_t nraw, int P,
                                                          fp* __restrict__ out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * (size_t)P) return;
  const size_t row = t / P, p = t % P;
  ge_ext acc = ge_identity();
  for (size_t k = p; k < nraw; k += P) acc = ge_add(acc, ge_load(in + 4 * (row * nraw + k)));
  ge_store_frozen(out + 4 * t, acc);
}

// out[i] = s_i * g[base] for n scalars (the blind terms of the row commitments): 8 threads per
// scalar, ceil(W/8) windows each, 3-level LDS tree -- one wave handles 8 scalars
__global__ __launch_bounds__(64) void single_base_mul_kernel(const fq* __restrict__ S, size_t n, TableView tv, size_t base,
                                                             ge_ext* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 8 + (threadIdx.x >> 3);
  const int grp = threadIdx.x & 7;
  ge_ext acc = ge_identity();
  if (i < n) {
    fq s = fq_load(S + i);
    if (!fq_is_zero(s)) {
      const TableSeg sg = table_seg(tv, base);
      const int wpg = (sg.W + 7) / 8;
      int w0 = grp * wpg, w1 = (w0 + wpg < sg.W) ? w0 + wpg : sg.W;
      if (w0 < w1) table_mul_acc_range(acc, fq_from_mont(s), sg, w0, w1);
    }
  }
  __shared__ ge_ext sh[64];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 4; st >= 1; st >>= 1) {
    if (grp < st) {
      acc = ge_add(acc, sh[threadIdx.x + st]);
      sh[threadIdx.x] = acc;
    }
    __syncthreads();
  }
  if (grp == 0 && i < n) ge_store(out + i, acc);
}

// out[row] = sum of the `chunks` partial points of that row
__global__ __launch_bounds__(64) void ge_sum_chunks_kernel(const ge_ext* __restrict__ parts, size_t rows, int chunks,
                                                           ge_ext* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const ge_ext* p = parts + i * chunks;
  ge_ext acc = ge_load(p);
  for (int k = 1; k < chunks; k++) acc = ge_add(acc, ge_load(p + k));
  ge_store(out + i, acc);
}

// out[i] = a[i] + b[i]  (row-wise commitment combination, proof_point_mult.rs:75-80)
__global__ __launch_bounds__(64) void ge_add_rows_kernel(const ge_ext* __restrict__ a, const ge_ext* __restrict__ b, size_t n,
                                                         ge_ext* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ge_store(out + i, ge_add(ge_load(a + i), ge_load(b + i)));
}

// out[j] = generator j (j < n), out[n] = generator blind_base (n_extra = 1): multiple 1 of window 0 in the base's table row
__global__ __launch_bounds__(256) void pip_gens_kernel(TableView tv, size_t n, size_t blind_base, int n_extra, ge_niels* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n + (size_t)n_extra) return;
  const TableSeg sg = table_seg(tv, i < n ? i : blind_base);
  ge_store(out + i, ge_load(sg.entry(0, 0)));
}

// RistrettoPoint::compress for n points, one thread each; also emits canonical X|Y|Z|T
__global__ __launch_bounds__(64) void ge_compress_kernel(const ge_ext* __restrict__ pts, size_t n, fp* __restrict__ out32,
                                                         fp* __restrict__ out_xyzt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ge_ext p = ge_load(pts + i);
  if (out32) fp_store(out32 + i, ge_compress(p));
  if (out_xyzt) ge_store_frozen(out_xyzt + 4 * i, p);
}

}  // namespace vpin

namespace vpin {

// ---- hash-to-group on the device: RistrettoPoint::from_uniform_bytes (RFC 9496 4.3.4 MAP, twice, added) ------------------
// MultiCommitGens::new (commitments.rs:20-38) maps 64 bytes of a SHAKE256 stream per generator; the host does the (sequential)
// stream and, for a 32 k-generator set, would spend 25-60 ms of eight cores on the two exponentiations per point.  One lane
// per generator here: the whole set in one pass of the chip.
__device__ __forceinline__ fp FP_ONE_MINUS_D_SQ() { return fp_const(0x945fc176u, 0xe27c09c1u, 0xcd5e350fu, 0x2c81a138u, 0xbe70dfe4u, 0x9994abddu, 0xb2b3e0d7u, 0x029072a8u); }
__device__ __forceinline__ fp FP_D_MINUS_ONE_SQ() { return fp_const(0x44ed4d20u, 0x31ad5aaau, 0xb01e1999u, 0xd29e4a2cu, 0x529b4eebu, 0x4cdcd32fu, 0xf66c2241u, 0x5968b37au); }
__device__ __forceinline__ fp FP_SQRT_AD_MINUS_ONE() { return fp_const(0x497b2e1bu, 0x7e97f6a0u, 0x1b7854bdu, 0xaf9d8e0cu, 0x31f5d1fdu, 0x0f3cfcc9u, 0x2b8348acu, 0x376931bfu); }

// RFC 9496 4.2 SQRT_RATIO_M1(u, v)
__device__ __forceinline__ fp fp_sqrt_ratio_m1(const fp& u, const fp& v, bool* was_square) {
  const fp v3 = fp_mul(fp_sqr(v), v), v7 = fp_mul(fp_sqr(v3), v);
  fp r = fp_mul(fp_mul(u, v3), fp_pow_p58(fp_mul(u, v7)));
  const fp check = fp_mul(v, fp_sqr(r));
  const fp nu = fp_neg(u), nu_i = fp_mul(nu, FP_SQRT_M1());
  const bool correct = fp_eq(check, u), flipped = fp_eq(check, nu), flipped_i = fp_eq(check, nu_i);
  r = fp_select(flipped || flipped_i, fp_mul(r, FP_SQRT_M1()), r);
  *was_square = correct || flipped;
  return fp_abs(r);
}

__device__ __noinline__ ge_ext ge_elligator(const fp& t) {
  const fp one = fp_one(), m1 = fp_neg(one), d = FP_D();
  const fp r = fp_mul(FP_SQRT_M1(), fp_sqr(t));
  const fp u = fp_mul(fp_add(r, one), FP_ONE_MINUS_D_SQ());
  const fp v = fp_mul(fp_sub(m1, fp_mul(r, d)), fp_add(r, d));
  bool sq;
  fp s = fp_sqrt_ratio_m1(u, v, &sq);
  const fp sp = fp_neg(fp_abs(fp_mul(s, t)));
  s = fp_select(sq, s, sp);
  const fp c = fp_select(sq, m1, r);
  const fp N = fp_sub(fp_mul(fp_mul(c, fp_sub(r, one)), FP_D_MINUS_ONE_SQ()), v);
  const fp ss = fp_sqr(s);
  const fp w0 = fp_mul(fp_add(s, s), v), w1 = fp_mul(N, FP_SQRT_AD_MINUS_ONE()), w2 = fp_sub(one, ss), w3 = fp_add(one, ss);
  ge_ext p;
  p.X = fp_mul(w0, w3); p.Y = fp_mul(w2, w1); p.Z = fp_mul(w1, w3); p.T = fp_mul(w0, w2);
  return p;
}

// stream: 64 bytes per generator; out: X | Y | Z | T, canonical 32-byte integers (the form Point::to_xyzt has on the host)
__global__ __launch_bounds__(64) void gens_derive_kernel(const uint32_t* __restrict__ stream, size_t nb, fp* __restrict__ xyzt) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= nb) return;
  fp t0, t1;
#pragma unroll
  for (int k = 0; k < 8; k++) { t0.v[k] = stream[16 * i + k]; t1.v[k] = stream[16 * i + 8 + k]; }
  t0.v[7] &= 0x7fffffffu;  // FieldElement::from_bytes ignores bit 255
  t1.v[7] &= 0x7fffffffu;
  const ge_ext p = ge_add(ge_elligator(t0), ge_elligator(t1));
  ge_store_frozen(xyzt + 4 * i, p);
}

}  // namespace vpin

using namespace vpin;

extern "C" {

static int gens_build_once(vpin_ctx* c, const uint8_t* gens_xyzt, size_t nb, size_t budget, int cmax, bool row_policy, vpin_gens** out);

// The table budget is a speed knob (every window bit saves ~8 % of a commitment), so it yields to what the device really has
// at this moment: at most a third of the FREE memory (a co-tenant, another process's tables, a smaller part), and a failed
// allocation halves it instead of failing the proof.  The instance, its decommitment and the proof temporaries need the rest.
static int gens_build(vpin_ctx* c, const uint8_t* gens_xyzt, size_t nb, size_t budget, bool row_policy, vpin_gens** out) {
  (void)hipSetDevice(c->device);
  size_t free_b = 0, total_b = 0;
  // (not asked in a one-shot process: its tables are sized by use, and the first hipMemGetInfo of a process costs 35-50 ms)
  const hipError_t e_info = c->expected_proofs > 0 ? hipErrorUnknown : hipMemGetInfo(&free_b, &total_b);
  if (e_info == hipSuccess && free_b) {
    static const double frac = [] { const char* e = getenv("VPIN_GENS_FREE_FRACTION"); double v = e ? atof(e) : 0.0; return v > 0.0 && v < 1.0 ? v : 1.0 / 3.0; }();
    const size_t cap = (size_t)((double)free_b * frac);
    if (budget > cap) budget = cap;
  }
  const size_t floor_b = (size_t)1 << 28;
  if (budget < floor_b) budget = floor_b;
  // A table that serves a known, small number of proofs (vpin_ctx_set_expected_proofs: a CLI process) is not worth its widest
  // windows: an entry costs ~4x a table addition to construct (projective chain, batched inversion, 96-byte scattered
  // store), so the width minimises entries x 4 + scalars x windows (measured: 142 ms to build the 12-bit table of the 2^25
  // instance, whose one proof then saves 48 ms of additions against the 10-bit one, built in 36 ms).
  // VPIN_GENS_CMAX (experiments): 13-bit windows are 20 instead of 22 additions per scalar for twice the table (129 GB for the
  // first 16386 generators): measured in round 5, see DESIGN.md section 4
  static const int env_cmax = [] { const char* e = getenv("VPIN_GENS_CMAX"); int v = e ? atoi(e) : 12; return v < 8 ? 8 : v > 14 ? 14 : v; }();
  int cmax = env_cmax;
  if (c->expected_proofs > 0 && c->gens_scalars_per_proof > 0.0) {
    const double S = c->gens_scalars_per_proof * (double)c->expected_proofs, n_lo = (double)std::min<size_t>(nb, 16386);
    double best = 0.0;
    for (int cc = 8; cc <= 12; cc++) {  // 8 bits = the narrowest windows the second table segment already uses
      const double W = (double)((254 + cc - 1) / cc), cost = n_lo * W * (double)(1u << (cc - 1)) * 4.0 + S * W;
      if (cc == 8 || cost < best) { best = cost; cmax = cc; }
    }
  }
  for (;;) {
    int rc = gens_build_once(c, gens_xyzt, nb, budget, cmax, row_policy, out);
    if (rc != VPIN_ENOMEM || budget <= floor_b) return rc;
    (void)hipGetLastError();
    budget /= 2;
    if (budget < floor_b) budget = floor_b;
  }
}

// bytes of a table slot for the NEXT table built: VPIN_TABLE_SLOT = 96 | 128 (read per build), default VPIN_NIELS_SLOT.  128 puts every
// entry on a 128-byte line of its own: -2.2 % on the four-lane LeNet step for a third more table memory at the same window width
// (profiles/r06_ab_slot128.txt) -- bench.py asks for it on a single-GPU run, the library's default stays 96 (headroom of split proofs)
static size_t table_slot_bytes() {
  const char* e = getenv("VPIN_TABLE_SLOT");
  const int v = e ? atoi(e) : VPIN_NIELS_SLOT;
  return v == 128 ? 128 : v == 96 ? 96 : (size_t)VPIN_NIELS_SLOT;
}

// The row table of the NEXT table built, forced: VPIN_ROW_TABLE_C = c (4..16) builds one of c-bit windows beside whatever
// multi-window table the build path chooses, whatever the budget (tests: several windows, segments and carries at tiny sizes);
// VPIN_ROW_TABLE = 0 builds none (A/B runs: the layout and the kernels of before).  Read per build.
static int row_table_forced_bits() {
  const char* e = getenv("VPIN_ROW_TABLE_C");
  const int v = e ? atoi(e) : 0;
  return v >= 4 && v <= 16 ? v : 0;
}
static bool row_table_off() {
  const char* e = getenv("VPIN_ROW_TABLE");
  return e && atoi(e) == 0;
}
// generators below which a stream gets no row table by policy.  Such a stream serves polynomials of up to 2^22 scalars, some of
// them above row_table_min_scalars (2^20): the bound is kept as it was because a row table narrows the stream's multi-window
// table to 8 bits for everything else it serves, which has not been measured for a process of small instances alone
constexpr size_t kRowTableMinBases = 4096;

static int gens_build_once(vpin_ctx* c, const uint8_t* gens_xyzt, size_t nb, size_t budget, int cmax, bool row_policy, vpin_gens** out) {
  if (!c || !gens_xyzt || !out || nb == 0) return VPIN_EINVAL;
  const size_t slot = table_slot_bytes();
  (void)hipSetDevice(c->device);
  vpin_gens* g = new (std::nothrow) vpin_gens();
  if (!g) return VPIN_ENOMEM;
  g->nb = nb;
  g->s32 = (int)(slot / 32);
  int nsum = 1;
  while (((size_t)2 << (nsum - 1)) <= nb) nsum++;  // S_0 .. S_floor(log2 nb)
  const size_t nbt = nb + (size_t)nsum;
  g->nbt = nbt;
  // Window widths by table budget.  Up to kSplitBases generators: one segment, the widest windows that fit (12 bits
  // up to ~5k generators under 24 GB, ...).  Longer streams: the first kSplitBases generators -- all that the
  // per-proof commitments of the largest instance walk (R = 2^14 columns + the two blind bases) -- get 12-bit
  // windows when the budget allows, the rest 8-bit ones: 71 + 6.4 GB for 32 786 bases, the 77 GB a uniform 11-bit
  // table took, and 22 instead of 24 table adds per scalar where the time goes.
  constexpr size_t kSplitBases = 16386;
  // the widest windows (<= cmax bits) whose table fits the budget; 6 bits (43 windows of 32 entries: 2.2 GB for 16386
  // generators) at the least, whatever the budget -- that allocation then succeeds or the build fails with VPIN_ENOMEM.
  // W and E always belong to the width returned (round 5: a budget below the 7-bit table used to leave 7-bit W and E beside
  // c = 6 -- a table too short for its scalars and WRONG sums; found by tools/ubench_pippenger.py's 1 GB walk, see
  // test_narrowest_windows_under_a_tiny_budget)
  auto fit = [&](size_t n, size_t bud, int cmax, int* c_, int* W_, int* E_) {
    int cc = cmax;
    for (; cc > 6; cc--)
      if (n * (size_t)((254 + cc - 1) / cc) * ((size_t)1 << (cc - 1)) * slot <= bud) break;
    *c_ = cc;
    *W_ = (254 + cc - 1) / cc;
    *E_ = 1 << (cc - 1);
  };
  g->split = nbt;
  fit(nb, budget, cmax, &g->c, &g->W, &g->E);
  if (nb > kSplitBases) {
    int c2, W2, E2;
    fit(kSplitBases, budget, cmax, &c2, &W2, &E2);
    const size_t lo_bytes = kSplitBases * (size_t)W2 * E2 * slot;
    if (c2 > g->c && lo_bytes < budget) {
      g->split = kSplitBases;
      g->c = c2; g->W = W2; g->E = E2;
      fit(nbt - kSplitBases, budget - lo_bytes, g->c, &g->c_hi, &g->W_hi, &g->E_hi);
    }
  }
  // The row table (see RowTable): the widest windows of 13..16 bits that fit the budget beside an 8-bit multi-window table of the
  // whole stream -- 16 bits for the 16386 generators the derefs commitment walks are 64 GiB in 128-byte slots, 16 additions per
  // folded scalar where the 12-bit multi-window table needs 21 in 88 GiB.  The multi-window table then serves the kernels that
  // multiply ONE scalar by one base (bullet rounds, few-row MSMs, blind terms, hot-column tables, constant rows), which spread
  // a scalar's windows over eight lanes: 32 windows of 8 bits are four per lane, as 29 of 9 bits would be.
  // By policy only for the provers' tables of a long-lived process (vpin::gens_shared_rows: sat_prepare and the SPARK views) and
  // only for streams of kRowTableMinBases generators and more; when no such table fits, the geometry is exactly the one above.
  const size_t n_row = std::min(nb, kSplitBases);
  int c_row = row_table_forced_bits();
  if (!c_row && row_policy && !row_table_off() && c->expected_proofs == 0 && nb >= kRowTableMinBases) {
    const size_t mw8 = nbt * (size_t)32 * 128 * slot;
    for (int cc = 16; cc >= 13 && !c_row; cc--)
      if (n_row * ((size_t)1 << (cc - 1)) * slot + mw8 <= budget) c_row = cc;
    if (c_row) {
      g->split = nbt;
      g->c = 8; g->W = 32; g->E = 128;
      g->narrowed = true;
    }
  }
  if (c_row) {
    g->n_row = n_row;
    g->c_row = c_row; g->W_row = row_windows(c_row); g->E_row = 1 << (c_row - 1);
  }
  const size_t entries_row = g->n_row * (size_t)g->E_row;
  const size_t n_hi = nbt - g->split;
  const size_t entries = g->split * (size_t)g->W * g->E, entries_hi = n_hi * (size_t)g->W_hi * g->E_hi;
  const size_t max_entries = std::max(std::max(entries, entries_hi), entries_row);
  const size_t max_shifts = std::max(g->split * (size_t)g->W, n_hi * (size_t)g->W_hi);
  TraceLap lap(c, "gens_build");
  // temporaries come from the context pool, so the blocks go on to serve proof temporaries instead of being
  // returned to the driver (freed VRAM is wiped before it can be handed out again: tools/ubench_malloc2.hip)
  DevBuf raw(c), b_shifts(c), b_prefix(c);
  if (raw.alloc(nbt * 128) != VPIN_OK || b_shifts.alloc(max_shifts * sizeof(ge_ext)) != VPIN_OK ||
      b_prefix.alloc(max_entries * sizeof(fp)) != VPIN_OK || driver_malloc((void**)&g->table, entries * slot) != hipSuccess ||
      (n_hi && driver_malloc((void**)&g->table_hi, entries_hi * slot) != hipSuccess) ||
      (entries_row && driver_malloc((void**)&g->table_row, entries_row * slot) != hipSuccess)) {
    if (g->table) (void)hipFree(g->table);
    if (g->table_hi) (void)hipFree(g->table_hi);
    if (g->table_row) (void)hipFree(g->table_row);
    delete g;
    return VPIN_ENOMEM;
  }
  ge_ext* shifts = (ge_ext*)b_shifts.p;
  fp* prefix = (fp*)b_prefix.p;
  lap("hipMalloc");
  hipError_t e = hipMemcpyAsync(raw.p, gens_xyzt, nb * 128, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(gens_sum_kernel, dim3((unsigned)nsum), dim3(256), 0, c->stream, (fp*)raw.p, nb);
    hipLaunchKernelGGL(gens_sum_scan_kernel, dim3(1), dim3(64), 0, c->stream, (fp*)raw.p, nb, nsum);
    hipLaunchKernelGGL(gens_shift_kernel, dim3((unsigned)((g->split + 63) / 64)), dim3(64), 0, c->stream, (const fp*)raw.p, g->split,
                       g->W, g->c, shifts);
    hipLaunchKernelGGL(gens_table_kernel, dim3((unsigned)((g->split * g->W + 63) / 64)), dim3(64), 0, c->stream, shifts, g->split, g->W,
                       g->E, g->table, g->s32, prefix);
    if (n_hi) {  // same temporaries, stream-ordered after the first segment
      hipLaunchKernelGGL(gens_shift_kernel, dim3((unsigned)((n_hi + 63) / 64)), dim3(64), 0, c->stream,
                         (const fp*)raw.p + 4 * g->split, n_hi, g->W_hi, g->c_hi, shifts);
      hipLaunchKernelGGL(gens_table_kernel, dim3((unsigned)((n_hi * g->W_hi + 63) / 64)), dim3(64), 0, c->stream, shifts, n_hi,
                         g->W_hi, g->E_hi, g->table_hi, g->s32, prefix);
    }
    // the row table: the generators themselves are the "shifts" of its one window (X | Y | Z | T is a ge_ext)
    if (entries_row)
      hipLaunchKernelGGL(gens_table_kernel, dim3((unsigned)((g->n_row + 63) / 64)), dim3(64), 0, c->stream, (const ge_ext*)raw.p, g->n_row, 1,
                         g->E_row, g->table_row, g->s32, prefix);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  lap("table kernels");
  // A service's table (no expected proof count): the largest build temporary -- a third of the table's size -- goes back to the
  // driver instead of staying in the context's pool, where nothing of its size comes to reuse it: 227.6 -> 219.5 GiB in use after
  // the LeNet step, the step unchanged, 0.8 s more set-up (the freed memory is wiped when it is next handed out).  Not in a one-shot
  // process, whose table build is inside the timed span.  VPIN_GENS_TMP_KEEP restores the old behaviour.
  // Only THIS block leaves the pool (the stream has been synchronised above, successfully): the context's other cached blocks
  // stay where the next proofs find them, and no other lane's work is synchronised with.
  if (e == hipSuccess && c->expected_proofs == 0 && !getenv("VPIN_GENS_TMP_KEEP") && b_prefix.p) {
    void* pp = b_prefix.p;
    b_prefix.p = nullptr;
    dev_release_block(c, pp);
  }
  if (e != hipSuccess) {
    set_last_error("vpin_gens_create", e);
    (void)hipFree(g->table);
    if (g->table_hi) (void)hipFree(g->table_hi);
    if (g->table_row) (void)hipFree(g->table_row);
    delete g;
    return VPIN_EHIP;
  }
  *out = g;
  return VPIN_OK;
}

static size_t default_budget() {
  static const size_t budget = [] {
    const char* e = getenv("VPIN_GENS_BUDGET_GB");
    size_t gb = e ? (size_t)atoi(e) : 24;
    return (gb ? gb : 24) << 30;
  }();
  return budget;
}

int vpin_gens_create(vpin_ctx* c, const uint8_t* gens_xyzt, size_t nb, vpin_gens** out) {
  return gens_build(c, gens_xyzt, nb, default_budget(), false, out);
}

// The first nb generators of a label's stream from 64 x nb bytes of SHAKE256 output (the caller's: host/transcript.h), mapped
// to the group on the device; out_xyzt: nb x 128 bytes on the host, the layout of vpin_host_gens_derive
int vpin_gens_map_stream(vpin_ctx* c, const uint8_t* stream64, size_t nb, uint8_t* out_xyzt) {
  if (!c || !stream64 || !out_xyzt || nb == 0) return VPIN_EINVAL;
  (void)hipSetDevice(c->device);
  DevBuf bs(c), bo(c);
  if (bs.alloc(nb * 64) || bo.alloc(nb * 128)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(bs.p, stream64, nb * 64, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(gens_derive_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, c->stream, (const uint32_t*)bs.p, nb, (fp*)bo.p);
  VPIN_HIP_TRY(hipGetLastError());
  VPIN_HIP_TRY(hipMemcpyAsync(out_xyzt, bo.p, nb * 128, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

// Process-wide registry of window tables by (device, label): every MultiCommitGens::new(n, label) is a
// prefix of one SHAKE stream (commitments.rs:20-38), so one table of the longest prefix requested so
// far serves every context, stream and polynomial size of that label.  Tables are immutable once
// built; superseded (shorter) ones stay alive because other contexts may still hold them.
namespace {
// rows: asked for by the provers' policy (vpin::gens_shared_rows).  ONE registry serves both kinds of request -- a prover finds and
// uses whatever table of its label covers its generators, a public table included (it then walks the multi-window table as before)
// -- with one exception: a table whose multi-window part was narrowed beside a row table is never returned by the public entry
// point, whose geometry must not depend on what a prover built before.
struct RegEntry { int device; std::string label; vpin_gens* g; bool rows; };
struct Building { int device; std::string label; size_t nb; bool rows; };
std::mutex g_reg_mu;
std::condition_variable g_reg_cv;
std::vector<RegEntry> g_reg;
std::vector<Building> g_building;  // tables under construction (the registry is unlocked meanwhile)
}  // namespace

static int gens_shared_impl(vpin_ctx* c, const char* label, const uint8_t* gens_xyzt, size_t nb, size_t budget_gb, bool rows,
                            const vpin_gens** out) {
  if (!c || !label || !out || nb == 0) return VPIN_EINVAL;
  auto lookup = [&]() -> const vpin_gens* {
    const vpin_gens* best = nullptr;
    for (auto& e : g_reg)
      if (e.device == c->device && e.label == label && (rows || !e.g->narrowed) && e.g->nb >= nb && (!best || e.g->nb < best->nb)) best = e.g;
    return best;
  };
  {
    std::unique_lock<std::mutex> lock(g_reg_mu);
    for (;;) {
      if (const vpin_gens* best = lookup()) { *out = best; return VPIN_OK; }
      // another thread is building a table that will cover this request: wait for it instead of building a second one
      // (tens of GB each); a shorter or different one under way does not help
      bool covered = false;
      for (auto& b : g_building) covered = covered || (b.device == c->device && b.label == label && (rows || !b.rows) && b.nb >= nb);
      if (!covered) break;
      g_reg_cv.wait(lock);
    }
    if (!gens_xyzt) return VPIN_EINVAL;
    // A longer prefix of a stream that already has a table: the shorter table stays (views of other contexts point into it)
    // and the new one is built beside it.  Said once: a service should ask for its largest shape first (vpin_spark_prepare).
    static std::atomic<bool> said{false};
    for (auto& e : g_reg)
      if (e.device == c->device && e.label == label && !said.exchange(true))
        fprintf(stderr, "vpin_gens_shared: a table of \"%s\" for %zu generators is built beside the one for %zu (both stay allocated): "
                        "call vpin_spark_prepare / vpin_sat_prepare with the largest shape first\n", label, nb, e.g->nb);
    g_building.push_back(Building{c->device, label, nb, rows});
  }
  // Built with the registry unlocked: other contexts of the process keep finding their tables, and building tables of other
  // labels, meanwhile.
  vpin_gens* g = nullptr;
  const int rc = gens_build(c, gens_xyzt, nb, budget_gb ? (budget_gb << 30) : default_budget(), rows, &g);
  std::lock_guard<std::mutex> lock(g_reg_mu);
  for (size_t i = 0; i < g_building.size(); i++)
    if (g_building[i].device == c->device && g_building[i].label == label && g_building[i].nb == nb && g_building[i].rows == rows) { g_building.erase(g_building.begin() + (long)i); break; }
  if (!rc) {
    g_reg.push_back(RegEntry{c->device, label, g, rows});
    *out = g;
  }
  g_reg_cv.notify_all();  // also on failure: the waiters then build for themselves
  return rc;
}

int vpin_gens_shared(vpin_ctx* c, const char* label, const uint8_t* gens_xyzt, size_t nb, size_t budget_gb,
                     const vpin_gens** out) {
  return gens_shared_impl(c, label, gens_xyzt, nb, budget_gb, false, out);
}

size_t vpin_gens_shared_bytes(int device) {
  std::lock_guard<std::mutex> lock(g_reg_mu);
  size_t total = 0;
  for (auto& e : g_reg)
    if (e.device == device)
      total += (size_t)32 * (size_t)e.g->s32 * ((size_t)e.g->W * e.g->split * (size_t)e.g->E +
                                     (e.g->split < e.g->nbt ? (size_t)e.g->W_hi * (e.g->nbt - e.g->split) * (size_t)e.g->E_hi : 0) +
                                     e.g->n_row * (size_t)e.g->E_row);
  return total;
}

void vpin_gens_shared_clear(void) {
  std::lock_guard<std::mutex> lock(g_reg_mu);
  for (auto& e : g_reg) {
    (void)hipSetDevice(e.device);
    (void)hipDeviceSynchronize();
    if (e.g->table) (void)hipFree(e.g->table);
    if (e.g->table_hi) (void)hipFree(e.g->table_hi);
    if (e.g->table_row) (void)hipFree(e.g->table_row);
    delete e.g;
  }
  g_reg.clear();
}

void vpin_gens_free(vpin_ctx* c, vpin_gens* g) {
  if (!g) return;
  if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
  if (g->table) (void)hipFree(g->table);
  if (g->table_hi) (void)hipFree(g->table_hi);
  if (g->table_row) (void)hipFree(g->table_row);
  delete g;
}

size_t vpin_gens_count(const vpin_gens* g) { return g ? g->nb : 0; }
// window layout chosen by the table budget: out = {c, W, split, c_hi, W_hi, nb + prefix-sum bases}
int vpin_gens_layout(const vpin_gens* g, size_t out[6]) {
  if (!g || !out) return VPIN_EINVAL;
  out[0] = (size_t)g->c; out[1] = (size_t)g->W; out[2] = g->split;
  out[3] = g->split < g->nbt ? (size_t)g->c_hi : 0; out[4] = g->split < g->nbt ? (size_t)g->W_hi : 0; out[5] = g->nbt;
  return VPIN_OK;
}
// the row table beside it: out = {c_row, W_row, bases covered, columns per LDS segment of the row kernel}; all 0 without one
int vpin_gens_row_layout(const vpin_gens* g, size_t out[4]) {
  if (!g || !out) return VPIN_EINVAL;
  out[0] = (size_t)g->c_row; out[1] = (size_t)g->W_row; out[2] = g->n_row; out[3] = g->c_row ? (size_t)row_segment(g->W_row) : 0;
  return VPIN_OK;
}
size_t vpin_gens_entry_bytes(void) { return table_slot_bytes(); }  // of the next table built (VPIN_TABLE_SLOT)

// shared implementation: rows of scalars -> points (kept on device), then optional outputs
static inline TableView view(const vpin_gens* g) {
  return TableView{g->table, g->table_hi, g->split, g->nbt, g->c, g->W, g->E, g->c_hi, g->W_hi, g->E_hi, g->nb, g->s32};
}

// VPIN_MSM_PIPPENGER = c (9..12, or 1 = the default width): every row commitment of the provers by the bucket method of
// msm_pip.hip instead of the table walk (few-row MSMs, the bullet reduction and single-base terms stay on the table).  For
// parity runs of whole proofs (tests/test_gpu_msm_pippenger.py) and A/B timing; read per call.
static int pip_mode() {
  const char* e = getenv("VPIN_MSM_PIPPENGER");
  const int v = e ? atoi(e) : 0;
  return v <= 0 ? 0 : (v >= 9 && v <= 12 ? v : -1);  // -1: the default width
}

static int msm_rows_pip(vpin_ctx* c, const vpin_gens* g, const fq* dZ, size_t rows, size_t stride, size_t ncols, const fq* d_extra,
                        int n_extra, size_t extra_base0, int cbits, ge_ext* d_points) {
  DevBuf dgn(c);
  if (dgn.alloc((ncols + 1) * sizeof(ge_niels))) return VPIN_ENOMEM;
  hipLaunchKernelGGL(pip_gens_kernel, dim3((unsigned)((ncols + 1 + 255) / 256)), dim3(256), 0, c->stream, view(g), ncols, extra_base0,
                     n_extra, (ge_niels*)dgn.p);
  return pip_rows(c, (const ge_niels*)dgn.p, dZ, rows, stride, ncols, d_extra, n_extra, cbits, d_points,
                  c->prof_count_adds ? c->d_add_count : nullptr);
}

// dynamic LDS the row-commitment kernels do not use: it lowers the workgroups per CU from 3 to 2 on a shared device
// (vpin_ctx_set_shared_device); VPIN_MSM_LDS_PAD overrides (experiments)
static unsigned msm_lds_pad(const vpin_ctx* c) {
  static const int env_pad = [] { const char* e = getenv("VPIN_MSM_LDS_PAD"); return e ? atoi(e) : -1; }();
  return env_pad >= 0 ? (unsigned)env_pad : (c->shared_device ? kSharedPad : 0u);
}

static inline RowTable row_view(const vpin_gens* g) {
  return RowTable{g->table_row, g->n_row, g->c_row, g->W_row, g->E_row, g->s32};
}

// Scalars from which a commitment goes to the row-table kernels.  The row table saves W - W_row = 32 - 16 additions per
// full-width scalar against the 8-bit multi-window table beside it; its finishing pass costs one lane per row running
// c (W_row - 1) = 240 doublings in sequence, ~0.5 ms whatever the size (that floor stays).  One commitment alone, walk against row
// table, host clock around the call in ms (tools/sweep_row_min.py -> profiles/r20_row_min_sweep.txt; Hyrax shape with a blind
// column / derefs shape without):
//   scalars   whole chip (256 CUs): walk -> row table   8 CUs per XCD (64 CUs): walk -> row table
//   2^17      0.47 -> 0.85 / 0.37 -> 0.83               0.95 -> 1.07 / 0.66 -> 0.98
//   2^18      0.64 -> 0.94 / 0.46 -> 0.91               1.62 -> 1.39 / 1.11 -> 1.22
//   2^19      1.00 -> 1.13 / 0.73 -> 1.08               2.74 -> 1.98 / 1.94 -> 1.66
//   2^20      1.72 -> 1.46 / 1.25 -> 1.27               5.02 -> 3.16 / 3.61 -> 2.54
//   2^21      3.14 -> 2.25 / 2.31 -> 1.86               9.42 -> 5.41 / 6.91 -> 4.26
//   2^22      5.84 -> 3.85 / 4.37 -> 3.07               18.6 -> 9.97 / 13.6 -> 7.65
// The default is the first size at which neither shape loses: 2^20 scalars, and 2^19 on a context confined to a quarter of the
// chip or less (bench.py's lanes of the smaller instances), where the same saving is worth four times the time.  The four-lane
// step at thresholds 2^24 / 2^22 / 2^20 / 2^18 / 2^16: 356.8 and 345.9 / 336.6 / 328.1 / 330.4 / 329.4 ms
// (profiles/r20_ab_row_min.txt): nothing is gained below 2^20.
// VPIN_MSM_ROW_MIN = n overrides (tests: 0; read per call); VPIN_MSM_ROW_TABLE = 0 keeps every commitment on the multi-window
// walk (A/B runs and parity tests; read per call).
// part_short: the caller's scalars are a mix of full-width and short ones (the two halves of a point-mult witness: coordinates
// beside bits and small constants).  The walk skips a short scalar's empty upper windows, so the row table saves less per scalar:
// the five point-mult instances of the LeNet trace proven one at a time on the whole chip, witness commitments (two polynomials)
// walk -> row table: 2^20..2^21 scalars each (L1-, L6-, L7-mult) 1.54 -> 2.13, 1.60 -> 2.10, 1.32 -> 1.95 ms; 2^22 and more
// (L3-mult) 3.60 -> 3.13 ms.  Such a caller takes the row table from 2^22 scalars.  On the quarter-chip lanes of the four-lane step
// the same commitments gain at every size (L6-mult 5.2 -> 3.7, L3-mult 14.7 -> 9.7 ms): there the threshold is the one above.
constexpr size_t kRowMinScalars = (size_t)1 << 20, kRowMinScalarsQuarter = (size_t)1 << 19, kRowMinScalarsPartShort = (size_t)1 << 22;
static size_t row_table_min_scalars(const vpin_ctx* c, bool part_short = false) {
  const char* e = getenv("VPIN_MSM_ROW_MIN");
  if (e) return (size_t)atoll(e);
  if (c->cu_masked && c->num_cus <= 64) return kRowMinScalarsQuarter;
  return part_short ? kRowMinScalarsPartShort : kRowMinScalars;
}
size_t vpin_msm_row_min_scalars(vpin_ctx* c, int part_short) { return c ? row_table_min_scalars(c, part_short != 0) : 0; }
static bool row_table_use(const vpin_ctx* c, const vpin_gens* g, size_t rows, size_t ncols, int n_extra, size_t extra_base0,
                          bool part_short = false) {
  if (!g->table_row || c->comm != nullptr) return false;  // a rank's share of a split commitment keeps the walk
  const char* e = getenv("VPIN_MSM_ROW_TABLE");
  if (e && atoi(e) == 0) return false;
  if (ncols > g->n_row || (n_extra && extra_base0 + (size_t)n_extra > g->n_row)) return false;
  return rows * (ncols + (size_t)n_extra) >= row_table_min_scalars(c, part_short);
}

// rows x (ncols + n_extra) scalars over the row table: msm_rows_win_kernel on `chunks` column chunks per row, then the finishing
// pass into d_points[rows].  hr: the derefs commitment's hot columns (HotRows{} for plain rows).
static int msm_rows_win(vpin_ctx* c, const vpin_gens* g, const RowArgs& ra, size_t rows, const HotRows& hr, ge_ext* d_points) {
  const RowTable rt = row_view(g);
  const int segn = row_segment(rt.W);
  c->row_table_rows += rows;
  const size_t total = ra.ncols + (size_t)ra.n_extra;
  // Column chunks: a workgroup ends with two LDS trees and W stores, so a chunk is worth several segments; enough of them to
  // give a few-row commitment three workgroups per CU, at most 64.
  const size_t most = std::max<size_t>(1, total / ((size_t)segn * 2));
  size_t want = rows >= 768 ? 1 : (768 + rows - 1) / rows;
  if (rows >= 768 && total > (size_t)kSeg) want = std::min<size_t>(8, (total + kSeg - 1) / kSeg);  // as row_chunks: short tails
  const char* ec = getenv("VPIN_MSM_ROW_WIN_CHUNKS");  // tests and A/B runs; read per call
  const int chunks = ec && atoi(ec) > 0 ? std::min(atoi(ec), 64) : (int)std::max<size_t>(1, std::min<size_t>(64, std::min(want, most)));
  DevBuf parts(c);
  if (parts.alloc(rows * (size_t)chunks * (size_t)rt.W * sizeof(ge_ext))) return VPIN_ENOMEM;
  hipLaunchKernelGGL(msm_rows_win_kernel, dim3((unsigned)rows, (unsigned)chunks), dim3(kMsmBlock), msm_lds_pad(c), c->stream, ra, view(g),
                     rt, hr, segn, (ge_ext*)parts.p);
  hipLaunchKernelGGL(msm_rows_finish_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, c->stream, (ge_ext*)parts.p, rows, chunks,
                     rt.W, rt.c, d_points);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

// Column chunks per row of the multi-window row kernels (gridDim.y), `total` scalars per row.
static int row_chunks(size_t rows, size_t total, bool hot_kernel) {
  if (hot_kernel) {
    // msm_rows_hot_kernel (the derefs commitment): one workgroup per compaction segment of a row, at most 8
    static const int env_chunks = [] { const char* e = getenv("VPIN_MSM_HOT_CHUNKS"); return e ? atoi(e) : 0; }();
    return env_chunks > 0 ? env_chunks : (int)std::max<size_t>(1, std::min<size_t>(8, total / kSeg));
  }
  if (rows < 128) {  // spread a few rows over the chip: ~one scalar per thread, <= 64 chunks per row
    size_t want = (total + kMsmBlock - 1) / kMsmBlock * 4;
    return (int)(want < 1 ? 1 : want > 64 ? 64 : want);
  }
  if (rows >= 768 && total > (size_t)kSeg) {
    // long rows (more than one compaction segment): one workgroup per segment, so that a launch of a few waves of
    // workgroups (a rank's share of a split commitment) does not end in a long, mostly idle tail
    static const int env_chunks = [] { const char* e = getenv("VPIN_MSM_ROW_CHUNKS"); return e ? atoi(e) : 0; }();
    return env_chunks > 0 ? env_chunks : (int)std::min<size_t>(8, (total + kSeg - 1) / kSeg);
  }
  if (rows < 768 && total >= 2 * (size_t)kMsmBlock) {
    // Fewer than three workgroups per CU: a wave's 22-addition chains run at ~13 us per addition instead of ~9.5 us
    // with the SIMDs full, and every thread walks several of them.  Split the rows into column chunks until the chip is
    // full or a thread is down to one scalar (the 2^15..2^17-constraint instances' derefs commitment: 573 -> ~300 us).
    size_t want = (768 + rows - 1) / rows, most = total / kMsmBlock;
    return std::max(1, (int)(want < most ? want : most));
  }
  return 1;
}

// The shape of msm_strip_kernel's launch for `eligible` regular rows of R scalars on `slots` workgroup slots: `groups` x
// `strips` workgroups that take the first `rows_used` eligible rows (0: none; the rows beyond the shape go back to the row
// kernel).  Host arithmetic only.
// Every CU must run the SAME number of strip workgroups, or the workgroups of a strip drift apart (a CU with two of them
// runs each 1.5x faster than a CU with three) and a table block is long evicted from L2 when the slow ones want it: the
// PMC pass of the first version (608 workgroups on 768 slots) showed 95 B of L2 misses per addition, more than the row
// kernel's 34 B.
// Choose the strips: every eligible row (G = ceil(n / 256) groups), S the largest multiple of 8 (a strip stays on one
// XCD) with G x S workgroups all RESIDENT (3 per CU) -- they wait for each other (msm_strip_kernel's sync) -- and strips of
// at least 128 generators.  Measured on the 2^25 instance (7844 eligible rows; profiles/r04_ab_strip.txt): free-running
// workgroups 85.8 ms and 139 M FETCH_SIZE units per dispatch, one generator of slack 81.6 ms and 91 M, two 82.6 / 103, four
// 85.0 / 111.
struct StripShape { size_t groups; int strips; uint32_t rows_used; };
static StripShape strip_shape(size_t R, uint32_t eligible, size_t slots, bool cu_masked, size_t min_list) {
  const size_t G = ((size_t)eligible + kMsmBlock - 1) / kMsmBlock;
  size_t bestG = 0;
  int bestS = 0;
  for (int cand = 8; cand <= 64 && (size_t)cand * 128 <= R; cand += 8)
    if (G * (size_t)cand <= slots) { bestG = G; bestS = cand; }
  // On a context confined to some of the CUs (vpin_ctx_create_cumask) "every eligible row" can leave the CUs unevenly
  // loaded (31 groups x 16 strips on 576 slots): take fewer groups and more strips when that fills more slots.
  // VPIN_MSM_STRIP_SHAPE=G,S forces a shape (A/B runs).
  if (cu_masked)
    for (int cand = 8; cand <= 64 && (size_t)cand * 128 <= R; cand += 8) {
      const size_t g2 = std::min(G, slots / (size_t)cand);
      if (g2 * kMsmBlock >= min_list && g2 * (size_t)cand > bestG * (size_t)bestS) { bestG = g2; bestS = cand; }
    }
  if (const char* eshape = getenv("VPIN_MSM_STRIP_SHAPE")) {
    int eg = 0, esn = 0;
    if (sscanf(eshape, "%d,%d", &eg, &esn) == 2 && eg > 0 && esn > 0 && esn % 8 == 0 && (size_t)esn <= R / 8) {
      // the strip's workgroups wait for each other: a forced shape must be resident as a whole like the chosen ones
      if (std::min(G, (size_t)eg) * (size_t)esn <= slots) { bestG = std::min(G, (size_t)eg); bestS = esn; }
      else if (getenv("VPIN_MSM_STRIP_TRACE")) fprintf(stderr, "[strip] VPIN_MSM_STRIP_SHAPE=%d,%d refused: %zu workgroups on %zu slots\n", eg, esn, std::min(G, (size_t)eg) * (size_t)esn, slots);
    }
  }
  return StripShape{bestG, bestS, bestG ? (uint32_t)std::min<size_t>(eligible, bestG * kMsmBlock) : 0u};
}

// What strip_take leaves for the launches of a commitment: the rows taken (n, 0: none), their flags for the row kernel (flag),
// their list with its count behind it, and the launch shape.
struct StripTake {
  DevBuf flag, list, parts, sync;
  size_t nrows = 0;
  uint32_t n = 0;
  int S = 16;
  bool uniform_shape = false;  // every strip workgroup of the launch is resident at once: they may wait for each other
  explicit StripTake(vpin_ctx* c) : flag(c), list(c), parts(c), sync(c) {}
  const uint32_t* d_list() const { return (const uint32_t*)list.p; }
  const uint32_t* d_count() const { return (const uint32_t*)list.p + nrows; }
};

// Row per lane (msm_strip_kernel) for a commitment of enough regular rows to keep every strip's block hot in L2 and the
// chip full: the 2^25-constraint instance's 16384 x 16384 derefs polynomial (9.5 k of its rows qualify).  Smaller ones,
// and a rank's share of a split commitment, stay with one workgroup per row.  Classifies the rows, lists and trims the regular
// ones to the launch shape; st.n = the rows taken, whose table walks strip_launch does and strip_combine adds to the row
// kernel's points.
// VPIN_MSM_STRIP = 0: off, S: number of strips; VPIN_MSM_STRIP_MIN = n: take the path from n rows on (tests, A/B runs; read per
// call so that a test can switch it)
static int strip_take(vpin_ctx* c, const vpin_gens* g, const RowArgs& ra, size_t nrows, const HotRows& hr, StripTake& st) {
  const char* es = getenv("VPIN_MSM_STRIP");
  const char* em = getenv("VPIN_MSM_STRIP_MIN");
  const size_t R = ra.ncols;
  const int env_strip = es ? atoi(es) : -1;
  const size_t min_rows = em ? (size_t)atol(em) : 8192, min_list = em ? (size_t)1 : 4096, min_R = em ? (size_t)64 : 4096;
  st.S = env_strip > 0 ? env_strip : 16;
  st.nrows = nrows;
  // Not on a shared device (vpin_ctx_set_shared_device: other contexts prove at the same time and the row kernels run one
  // workgroup per CU): with a single wave per SIMD nothing hides the strip kernel's per-generator chain scalar load ->
  // Montgomery conversion -> first gather, and its workgroups no longer step together: the default LeNet step of bench.py
  // measured 469-473 ms with it against 438-442 ms without (profiles/r04_ab_strip.txt), while the 2^25 instance proven alone
  // gains (313 -> 303 ms).  VPIN_MSM_STRIP > 0 forces it (A/B runs).
  // Nor for a rank's share of a split commitment (c->comm set: at W = 2 the share of 16384 rows is exactly min_rows, and
  // rehearsal ranks share one GPU without saying so): its workgroups would not all be resident and the bounded wait of the
  // kernel would be sat out per generator.
  if (!(env_strip != 0 && (env_strip > 0 || (!c->shared_device && c->comm == nullptr)) && nrows >= min_rows && R >= min_R && R <= g->split &&
        st.S % 8 == 0 && (size_t)st.S <= R / 8))
    return VPIN_OK;
  if (st.flag.alloc(nrows) || st.list.alloc((nrows + 1) * sizeof(uint32_t))) return VPIN_ENOMEM;
  uint32_t* d_list = (uint32_t*)st.list.p;
  uint32_t* d_count = d_list + nrows;
  uint32_t n_strip = 0;
  hipLaunchKernelGGL(strip_classify_kernel, dim3((unsigned)nrows), dim3(kMsmBlock), 0, c->stream, ra, hr, (uint8_t*)st.flag.p);
  hipLaunchKernelGGL(strip_list_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint8_t*)st.flag.p, nrows, d_list, d_count);
  VPIN_HIP_TRY(hipMemcpyAsync(&n_strip, d_count, sizeof n_strip, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_strip < min_list) n_strip = 0;  // too few rows to share a block's fetch: the row kernel takes everything
  if (n_strip && env_strip < 0) {
    const size_t slots = (size_t)c->num_cus * (c->shared_device ? 1 : 3);
    const StripShape shape = strip_shape(R, n_strip, slots, c->cu_masked, min_list);
    if (shape.rows_used && shape.rows_used < n_strip)
      hipLaunchKernelGGL(strip_trim_kernel, dim3((n_strip - shape.rows_used + 255) / 256), dim3(256), 0, c->stream, (const uint32_t*)d_list,
                         d_count, shape.rows_used, n_strip, (uint8_t*)st.flag.p);
    if (getenv("VPIN_MSM_STRIP_TRACE")) fprintf(stderr, "[strip] %zu rows: %u eligible, %u taken as %zu groups x %d strips on %zu slots\n", nrows, n_strip, shape.rows_used, shape.groups, shape.strips, slots);
    n_strip = shape.rows_used;
    if (n_strip) {
      st.S = shape.strips;
      st.uniform_shape = true;
    }
  }
  if (n_strip && st.parts.alloc((size_t)n_strip * (size_t)st.S * sizeof(ge_ext))) return VPIN_ENOMEM;
  st.n = n_strip;
  return VPIN_OK;
}
// the table walks of the rows taken: st.parts[li * S + s]
static int strip_launch(vpin_ctx* c, const vpin_gens* g, const RowArgs& ra, const HotRows& hr, StripTake& st, unsigned pad) {
  c->strip_rows_taken += st.n;
  const unsigned groups = (unsigned)((st.n + kMsmBlock - 1) / kMsmBlock);
  const size_t per = (ra.ncols + (size_t)st.S - 1) / (size_t)st.S;
  const char* el = getenv("VPIN_MSM_STRIP_LAG");  // generators a workgroup may run ahead of its strip's slowest; 0: no sync
  const int lag = el ? atoi(el) : 1;
  uint32_t* d_sync = nullptr;
  if (lag > 0 && st.uniform_shape) {
    if (st.sync.alloc((size_t)st.S * (per + 1) * sizeof(uint32_t))) return VPIN_ENOMEM;
    d_sync = (uint32_t*)st.sync.p;
    VPIN_HIP_TRY(hipMemsetAsync(d_sync, 0, (size_t)st.S * (per + 1) * sizeof(uint32_t), c->stream));
  }
  hipLaunchKernelGGL(msm_strip_kernel, dim3(groups * (unsigned)st.S), dim3(kMsmBlock), pad, c->stream, ra, view(g), hr, st.d_list(),
                     st.d_count(), st.S, (ge_ext*)st.parts.p, d_sync, lag);
  return VPIN_OK;
}

// How a commitment's rows are launched.
struct RowPolicy {
  // the caller knows its scalars to be mostly short (addresses, counters): the multi-window walk, where a lane skips a short
  // scalar's empty upper windows; in the row-table kernel those windows' lanes would idle
  bool walk_only = false;
  bool part_short = false;  // see row_table_min_scalars
  // the derefs commitment: without a row table msm_rows_hot_kernel (hr's hot columns) and the strip path may be tried
  bool may_strip = false;
};

// The one launch path of the row commitments: d_points[i] = the commitment of launch row i of ra, i < rows.  Over the row table
// where row_table_use says so, else msm_rows_kernel or (may_strip) msm_rows_hot_kernel beside the strip kernel, on row_chunks
// column chunks that are summed at the end.
static int msm_rows_launch(vpin_ctx* c, const vpin_gens* g, const RowArgs& ra, size_t rows, const HotRows& hr, const RowPolicy& pol,
                           ge_ext* d_points) {
  const size_t total = ra.ncols + (size_t)ra.n_extra;
  const int chunks = row_chunks(rows, total, pol.may_strip);
  // With a row table the whole derefs commitment, regular rows included, goes to msm_rows_win_kernel.  Measured against the strip
  // kernel forced (which then walks the 8-bit window table): step 345.5-347.1 against 431.6 ms, L5-mult alone 251.8 against 329.8 ms
  // (profiles/r12_ab_row_table.txt).  An explicit VPIN_MSM_STRIP / VPIN_MSM_STRIP_MIN keeps its meaning: the
  // strip and hot kernels over the multi-window table.
  const bool strip_asked = pol.may_strip && (getenv("VPIN_MSM_STRIP") || getenv("VPIN_MSM_STRIP_MIN"));
  const bool use_row = !pol.walk_only && !strip_asked && row_table_use(c, g, rows, ra.ncols, ra.n_extra, ra.extra_base0, pol.part_short);
  const bool as_rows = pol.may_strip || rows >= 128;  // counted and profiled as a row commitment (not the few-row MSMs)
  if (c->prof_count_adds && c->d_add_count && as_rows)
    hipLaunchKernelGGL(msm_count_adds_kernel, dim3((unsigned)rows), dim3(kMsmBlock), 0, c->stream, ra, view(g), hr, use_row ? g->c_row : 0,
                       use_row ? g->W_row : 0, c->d_add_count);
  const double bytes = 32.0 * (double)rows * (double)total;
  if (use_row) {
    ProfScope ps(c, VPIN_K_MSM, bytes, as_rows ? VPIN_K_MSM_ROWS : -1);
    return msm_rows_win(c, g, ra, rows, hr, d_points);
  }
  DevBuf parts(c);
  ge_ext* dst = d_points;
  if (chunks > 1) {
    if (parts.alloc(rows * (size_t)chunks * sizeof(ge_ext))) return VPIN_ENOMEM;
    dst = (ge_ext*)parts.p;
  }
  StripTake st(c);
  if (pol.may_strip)
    if (const int rc = strip_take(c, g, ra, rows, hr, st)) return rc;
  {
    ProfScope ps(c, VPIN_K_MSM, bytes, as_rows ? VPIN_K_MSM_ROWS : -1);
    const unsigned pad = msm_lds_pad(c);
    const dim3 grid((unsigned)rows, (unsigned)chunks);
    if (st.n)
      if (const int rc = strip_launch(c, g, ra, hr, st, pad)) return rc;
    if (pol.may_strip)
      hipLaunchKernelGGL(msm_rows_hot_kernel, grid, dim3(kMsmBlock), pad, c->stream, ra, view(g), hr, dst,
                         st.n ? (const uint8_t*)st.flag.p : (const uint8_t*)nullptr);
    else
      hipLaunchKernelGGL(msm_rows_kernel, grid, dim3(kMsmBlock), pad, c->stream, ra, view(g), dst);
    if (chunks > 1)
      hipLaunchKernelGGL(ge_sum_chunks_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, c->stream, (const ge_ext*)dst, rows, chunks,
                         d_points);
    if (st.n)
      hipLaunchKernelGGL(strip_combine_kernel, dim3((st.n + 63) / 64), dim3(64), 0, c->stream, (const ge_ext*)st.parts.p, st.d_list(),
                         st.d_count(), st.S, d_points);
  }
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

// plain rows: rows x (ncols scalars from Z with row stride `stride`) + optional extra scalars on bases
// [extra_base0, extra_base0 + n_extra).  d_points[row] = sum_j s[row][j] * g_j  (extended coords)
static int msm_rows(vpin_ctx* c, const vpin_gens* g, const fq* dZ, size_t rows, size_t stride, size_t ncols,
                    const fq* d_extra, int n_extra, size_t extra_base0, ge_ext* d_points, bool walk_only = false,
                    bool part_short = false) {
  if (const int pm = pip_mode())
    if (n_extra <= 1 && ncols + (size_t)n_extra <= 32768)
      return msm_rows_pip(c, g, dZ, rows, stride, ncols, d_extra, n_extra, extra_base0, pm < 0 ? 0 : pm, d_points);
  return msm_rows_launch(c, g, RowArgs{dZ, stride, ncols, d_extra, n_extra, extra_base0, 0, 1, 0}, rows, HotRows{},
                         RowPolicy{walk_only, part_short, false}, d_points);
}

// The end of every commitment: compress the n points at d_pts and bring the encodings home, the first n / k of them to out0,
// the next to out1, .. for the k outputs given; synchronises.
static int compress_to_host(vpin_ctx* c, const ge_ext* d_pts, size_t n, uint8_t* out0, uint8_t* out1 = nullptr, uint8_t* out2 = nullptr) {
  uint8_t* const outs[3] = {out0, out1, out2};
  const size_t k = out2 ? 3 : out1 ? 2 : 1, per = n / k * 32;
  DevBuf dout(c);
  if (dout.alloc(n * 32)) return VPIN_ENOMEM;
  hipLaunchKernelGGL(ge_compress_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, d_pts, n, (fp*)dout.p, (fp*)nullptr);
  VPIN_HIP_TRY(hipGetLastError());
  for (size_t i = 0; i < k; i++) VPIN_HIP_TRY(hipMemcpyAsync(outs[i], (uint8_t*)dout.p + i * per, per, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

// out_compressed[i] = commitment of row i: R scalars at z + i * stride over generators [0, R), plus blinds[i] (host, optional)
// on generator blind_base.  buckets: by msm_pip.hip with windows of c_bits (0: its default) instead of the table walk.
// The entry points below have checked the arguments.
static int commit_rows(vpin_ctx* c, const vpin_gens* g, const fq* z, size_t rows, size_t stride, size_t R, const uint8_t* blinds,
                       size_t blind_base, bool buckets, int c_bits, uint8_t* out_compressed, bool walk_only = false) {
  (void)hipSetDevice(c->device);
  const int n_extra = blinds ? 1 : 0;
  DevBuf dbl(c), dpts(c);
  if ((blinds && dbl.alloc(rows * 32)) || dpts.alloc(rows * sizeof(ge_ext))) return VPIN_ENOMEM;
  if (blinds) VPIN_HIP_TRY(hipMemcpyAsync(dbl.p, blinds, rows * 32, hipMemcpyHostToDevice, c->stream));
  const int rc = buckets ? msm_rows_pip(c, g, z, rows, stride, R, (const fq*)dbl.p, n_extra, blind_base, c_bits, (ge_ext*)dpts.p)
                         : msm_rows(c, g, z, rows, stride, R, (const fq*)dbl.p, n_extra, blind_base, (ge_ext*)dpts.p, walk_only);
  if (rc) return rc;
  return compress_to_host(c, (const ge_ext*)dpts.p, rows, out_compressed);
}

int vpin_hyrax_commit(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, const uint8_t* blinds, size_t L,
                      size_t blind_base, uint8_t* out_compressed) {
  if (!c || !g || !Z || !Z->d || !blinds || !out_compressed || L == 0) return VPIN_EINVAL;
  if (Z->len % L != 0) return VPIN_ESHAPE;  // assert_eq!(L_size * R_size, self.Z.len())
  const size_t R = Z->len / L;
  if (R > g->nb || blind_base >= g->nb) return VPIN_ESHAPE;  // assert_eq!(gens_n.n, self.len())
  return commit_rows(c, g, Z->d, L, R, R, blinds, blind_base, false, 0, out_compressed);
}

// the same commitment by Pippenger's bucket method from the generators alone (msm_pip.hip): same bytes, no table walked
int vpin_hyrax_commit_pippenger(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, const uint8_t* blinds, size_t L,
                                size_t blind_base, int c_bits, uint8_t* out_compressed) {
  if (!c || !g || !Z || !Z->d || !out_compressed || L == 0) return VPIN_EINVAL;
  if (Z->len % L != 0) return VPIN_ESHAPE;
  const size_t R = Z->len / L;
  if (R > g->nb || (blinds && blind_base >= g->nb)) return VPIN_ESHAPE;
  return commit_rows(c, g, Z->d, L, R, R, blinds, blind_base, true, c_bits, out_compressed);
}

int vpin_hyrax_commit_rows(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, size_t L, size_t row0, size_t nrows,
                           const uint8_t* blinds, size_t blind_base, uint8_t* out_compressed) {
  if (!c || !g || !Z || !Z->d || !out_compressed || L == 0 || nrows == 0) return VPIN_EINVAL;
  if (Z->len % L != 0 || row0 + nrows > L) return VPIN_ESHAPE;
  const size_t R = Z->len / L;
  if (R > g->nb || (blinds && blind_base >= g->nb)) return VPIN_ESHAPE;
  return commit_rows(c, g, Z->d + row0 * R, nrows, R, R, blinds, blind_base, false, 0, out_compressed);
}

}  // extern "C"

namespace vpin {

// DensePolynomial::commit(gens, None) for the derefs polynomial (8N scalars as L rows of R; sparse_mlpoly.rs:525-531) with the
// hot column of each matrix's col-derefs vector taken out (msm_rows_hot_kernel).  col_idx[m]: the N column indices of matrix
// m on the device, hot[m]: its hot column or 0xffffffff, e_ry: the table the col-derefs were gathered from.
int hyrax_commit_derefs_hot(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, size_t L, size_t N, const uint32_t* const col_idx[3],
                            const uint32_t hot[3], const fq* e_ry, uint8_t* out_compressed, size_t row0, size_t nrows, size_t row_step,
                            const fq* z_rows) {
  // z_rows != nullptr: the nrows rows of this call stored densely (Z may then be a shape-only handle: d unused)
  if (!c || !g || !Z || (!Z->d && !z_rows) || !col_idx || !hot || !e_ry || !out_compressed || L == 0 || Z->len % L) return VPIN_EINVAL;
  const size_t R = Z->len / L;
  if (R > g->nb || N % R || Z->len < 6 * N) return VPIN_ESHAPE;
  const fq* zbase = z_rows ? z_rows : (const fq*)Z->d;
  const int z_compact = z_rows ? 1 : 0;
  if (nrows == (size_t)-1) { row0 = 0; nrows = L; row_step = 1; }  // all rows
  if (row_step == 0 || (nrows && row0 + (nrows - 1) * row_step >= L)) return VPIN_ESHAPE;
  if (nrows == 0) return VPIN_OK;
  if (pip_mode()) return hyrax_commit_rows_strided(c, g, Z, L, row0, nrows, row_step, out_compressed, z_rows);  // plain rows, buckets
  (void)hipSetDevice(c->device);
  DevBuf dpts(c), dT(c);
  if (dpts.alloc(nrows * sizeof(ge_ext))) return VPIN_ENOMEM;
  HotRows hr{};
  hr.row0 = 3 * (N / R);
  hr.rows_per_vec = N / R;
  // one T table per distinct hot column
  uint32_t distinct[3];
  int nd = 0;
  for (int m = 0; m < 3; m++) {
    hr.idx[m] = col_idx[m];
    hr.hot[m] = hot[m];
    if (hot[m] == 0xffffffffu) continue;
    bool seen = false;
    for (int k = 0; k < nd; k++) seen = seen || distinct[k] == hot[m];
    if (!seen) distinct[nd++] = hot[m];
  }
  if (nd && dT.alloc((size_t)nd * R * sizeof(ge_cached))) return VPIN_ENOMEM;
  for (int k = 0; k < nd; k++) {
    ge_cached* Tk = (ge_cached*)dT.p + (size_t)k * R;
    hipLaunchKernelGGL(scalar_times_bases_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, c->stream, e_ry + distinct[k], R, view(g), Tk);
    for (int m = 0; m < 3; m++)
      if (hot[m] == distinct[k]) hr.T[m] = Tk;
  }
  if (const int rc = msm_rows_launch(c, g, RowArgs{zbase, R, R, nullptr, 0, 0, row0, row_step, z_compact}, nrows, hr,
                                     RowPolicy{false, false, true}, (ge_ext*)dpts.p))
    return rc;
  return compress_to_host(c, (const ge_ext*)dpts.p, nrows, out_compressed);
}

int hyrax_commit_walk(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, const uint8_t* blinds, size_t L, size_t blind_base,
                      uint8_t* out_compressed) {
  if (!c || !g || !Z || !Z->d || !blinds || !out_compressed || L == 0) return VPIN_EINVAL;
  if (Z->len % L != 0) return VPIN_ESHAPE;
  const size_t R = Z->len / L;
  if (R > g->nb || blind_base >= g->nb) return VPIN_ESHAPE;
  return commit_rows(c, g, Z->d, L, R, R, blinds, blind_base, false, 0, out_compressed, true);
}

int gens_shared_rows(vpin_ctx* c, const char* label, const uint8_t* gens_xyzt, size_t nb, size_t budget_gb, const vpin_gens** out) {
  return gens_shared_impl(c, label, gens_xyzt, nb, budget_gb, true, out);
}

int hyrax_commit_rows_strided(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, size_t L, size_t row0, size_t nrows, size_t row_step,
                              uint8_t* out_compressed, const fq* z_rows) {
  if (!c || !g || !Z || (!Z->d && !z_rows) || !out_compressed || L == 0 || row_step == 0) return VPIN_EINVAL;
  if (nrows == 0) return VPIN_OK;
  if (Z->len % L != 0 || row0 + (nrows - 1) * row_step >= L) return VPIN_ESHAPE;
  const size_t R = Z->len / L;
  if (R > g->nb) return VPIN_ESHAPE;
  if (z_rows) return commit_rows(c, g, z_rows, nrows, R, R, nullptr, 0, false, 0, out_compressed);
  return commit_rows(c, g, Z->d + row0 * R, nrows, row_step * R, R, nullptr, 0, false, 0, out_compressed);
}

}  // namespace vpin

extern "C" {

int vpin_hyrax_commit_derefs(vpin_ctx* c, const vpin_gens* g, const vpin_table* Z, size_t L, size_t N, const uint32_t* col_idx,
                             const uint32_t hot[3], const vpin_table* e_ry, uint8_t* out_compressed) {
  if (!c || !g || !Z || !Z->d || !col_idx || !hot || !e_ry || !e_ry->d || !out_compressed || L == 0 || N == 0) return VPIN_EINVAL;
  for (size_t i = 0; i < 3 * N; i++)
    if (col_idx[i] >= e_ry->len) return VPIN_ESHAPE;
  for (int m = 0; m < 3; m++)
    if (hot[m] != 0xffffffffu && hot[m] >= e_ry->len) return VPIN_ESHAPE;
  (void)hipSetDevice(c->device);
  DevBuf didx(c);
  if (didx.alloc(3 * N * sizeof(uint32_t))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(didx.p, col_idx, 3 * N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  const uint32_t* const idx[3] = {(const uint32_t*)didx.p, (const uint32_t*)didx.p + N, (const uint32_t*)didx.p + 2 * N};
  return vpin::hyrax_commit_derefs_hot(c, g, Z, L, N, idx, hot, (const fq*)e_ry->d, out_compressed);  // synchronises
}

int vpin_hyrax_commit_pair(vpin_ctx* c, const vpin_gens* g, const vpin_table* Za, const vpin_table* Zb,
                           const uint8_t* blinds_a, const uint8_t* blinds_b, size_t L, size_t blind_base,
                           uint8_t* out_a, uint8_t* out_b, uint8_t* out_sum) {
  if (!c || !g || !Za || !Zb || !blinds_a || !blinds_b || !out_a || !out_b || !out_sum || L == 0) return VPIN_EINVAL;
  if (Za->len != Zb->len || Za->len % L != 0) return VPIN_ESHAPE;
  size_t R = Za->len / L;
  if (R > g->nb || blind_base >= g->nb) return VPIN_ESHAPE;
  (void)hipSetDevice(c->device);
  DevBuf dbl(c), dpts(c);
  if (dbl.alloc(2 * L * 32) || dpts.alloc(3 * L * sizeof(ge_ext))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(dbl.p, blinds_a, L * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync((uint8_t*)dbl.p + L * 32, blinds_b, L * 32, hipMemcpyHostToDevice, c->stream));
  ge_ext* pts = (ge_ext*)dpts.p;
  int rc = msm_rows(c, g, Za->d, L, R, R, (const fq*)dbl.p, 1, blind_base, pts);
  if (rc) return rc;
  rc = msm_rows(c, g, Zb->d, L, R, R, (const fq*)dbl.p + L, 1, blind_base, pts + L);
  if (rc) return rc;
  hipLaunchKernelGGL(ge_add_rows_kernel, dim3((unsigned)((L + 63) / 64)), dim3(64), 0, c->stream, pts, pts + L, L, pts + 2 * L);
  return compress_to_host(c, pts, 3 * L, out_a, out_b, out_sum);
}

// partial points of few-row MSMs: parts_xyzt must hold rows * vpin_gens_msm_parts_count(ncols) * 128 bytes
// at most kMaxParts per row: longer rows get a second, on-device summation stage (the host would
// otherwise add a thousand points per row for the 32k-generator evaluation proofs)
constexpr size_t kMaxParts = 128;  // the host adds up to 128 partial points per row (~20 us) rather than wait for a second kernel
static inline int wide_q(size_t ncols) { return ncols >= 8192 ? 4 : 1; }
static inline size_t raw_parts(size_t ncols) { const size_t per = (size_t)kWideScalars * wide_q(ncols); return (ncols + per - 1) / per; }
size_t vpin_gens_msm_parts_count(size_t ncols) { size_t n = raw_parts(ncols); return n < kMaxParts ? n : kMaxParts; }

int vpin_gens_msm_parts(vpin_ctx* c, const vpin_gens* g, const uint8_t* scalars_mont, size_t rows, size_t ncols,
                        uint8_t* parts_xyzt) {
  if (!c || !g || !scalars_mont || !parts_xyzt || rows == 0 || ncols == 0) return VPIN_EINVAL;
  if (ncols > g->nb) return VPIN_ESHAPE;
  (void)hipSetDevice(c->device);
  DevBuf ds(c);
  if (ds.alloc(rows * ncols * 32)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(ds.p, scalars_mont, rows * ncols * 32, hipMemcpyHostToDevice, c->stream));
  return vpin::gens_msm_parts_dev(c, g, (const fq*)ds.p, rows, ncols, parts_xyzt);
}

}  // extern "C"

// Split-phase form of vpin_hyrax_commit_pair for the host prover: `begin` enqueues the two big
// row MSMs (which do not depend on the blinds), the host draws the 2L blinds from its RandomTape
// while they run, `finish` adds blind_i * g[blind_base] per row, combines and compresses.
namespace vpin {
struct CommitPairState {
  DevBuf pts;  // [5L] : M_a | M_b | blind_a*h | blind_b*h (reused for sums) | a+b
  size_t L = 0;  // rows this state commits (a block of the polynomial's rows when the commitment is split across ranks)
  explicit CommitPairState(vpin_ctx* c) : pts(c) {}
};

int commit_pair_begin(vpin_ctx* c, const vpin_gens* g, const vpin_table* Za, const vpin_table* Zb, size_t L_all,
                      CommitPairState** out, size_t row0, size_t nrows, size_t row_step) {
  if (!c || !g || !Za || !Zb || !out || L_all == 0) return VPIN_EINVAL;
  if (Za->len != Zb->len || Za->len % L_all != 0) return VPIN_ESHAPE;
  size_t R = Za->len / L_all;
  if (R > g->nb) return VPIN_ESHAPE;
  if (nrows == (size_t)-1) { row0 = 0; nrows = L_all; row_step = 1; }
  if (nrows == 0 || row_step == 0 || row0 + (nrows - 1) * row_step >= L_all) return VPIN_ESHAPE;
  const size_t L = nrows;
  (void)hipSetDevice(c->device);
  CommitPairState* st = new (std::nothrow) CommitPairState(c);
  if (!st) return VPIN_ENOMEM;
  st->L = L;
  if (st->pts.alloc(5 * L * sizeof(ge_ext))) { delete st; return VPIN_ENOMEM; }
  ge_ext* pts = (ge_ext*)st->pts.p;
  // the provers' witness halves: part_short (see row_table_min_scalars)
  int rc = msm_rows(c, g, Za->d + row0 * R, L, row_step * R, R, nullptr, 0, 0, pts, false, true);
  if (!rc) rc = msm_rows(c, g, Zb->d + row0 * R, L, row_step * R, R, nullptr, 0, 0, pts + L, false, true);
  if (rc) { delete st; return rc; }
  *out = st;
  return VPIN_OK;
}

int commit_pair_finish(vpin_ctx* c, const vpin_gens* g, CommitPairState* st, const uint8_t* blinds_a, const uint8_t* blinds_b,
                       size_t blind_base, uint8_t* out_a, uint8_t* out_b, uint8_t* out_sum) {
  if (!st) return VPIN_EINVAL;
  std::unique_ptr<CommitPairState> guard(st);
  if (!c || !g || !blinds_a || !blinds_b || !out_a || !out_b || !out_sum) return VPIN_EINVAL;
  if (blind_base >= g->nb) return VPIN_ESHAPE;
  const size_t L = st->L;
  DevBuf dbl(c);
  if (dbl.alloc(2 * L * 32)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(dbl.p, blinds_a, L * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync((uint8_t*)dbl.p + L * 32, blinds_b, L * 32, hipMemcpyHostToDevice, c->stream));
  ge_ext* pts = (ge_ext*)st->pts.p;
  // 2L single-scalar multiples of the blind generator
  hipLaunchKernelGGL(single_base_mul_kernel, dim3((unsigned)((2 * L + 7) / 8)), dim3(64), 0, c->stream, (const fq*)dbl.p, 2 * L,
                     view(g), blind_base, pts + 2 * L);
  const unsigned gb = (unsigned)((2 * L + 63) / 64);
  hipLaunchKernelGGL(ge_add_rows_kernel, dim3(gb), dim3(64), 0, c->stream, pts, pts + 2 * L, 2 * L, pts + 2 * L);  // a, b
  hipLaunchKernelGGL(ge_add_rows_kernel, dim3((unsigned)((L + 63) / 64)), dim3(64), 0, c->stream, pts + 2 * L, pts + 3 * L, L,
                     pts + 4 * L);  // a + b
  return compress_to_host(c, pts + 2 * L, 3 * L, out_a, out_b, out_sum);
}
}  // namespace vpin

extern "C" {

// vpin_hyrax_commit_pair through the provers' split-phase path (commit_pair_begin / commit_pair_finish): the blind terms are
// single_base_mul_kernel's
int vpin_hyrax_commit_pair_split(vpin_ctx* c, const vpin_gens* g, const vpin_table* Za, const vpin_table* Zb,
                                 const uint8_t* blinds_a, const uint8_t* blinds_b, size_t L, size_t blind_base,
                                 uint8_t* out_a, uint8_t* out_b, uint8_t* out_sum) {
  if (!c || !g || !Za || !Zb || !Za->d || !Zb->d || !blinds_a || !blinds_b || !out_a || !out_b || !out_sum || L == 0) return VPIN_EINVAL;
  vpin::CommitPairState* st = nullptr;
  if (const int rc = vpin::commit_pair_begin(c, g, Za, Zb, L, &st, 0, (size_t)-1, 1)) return rc;
  return vpin::commit_pair_finish(c, g, st, blinds_a, blinds_b, blind_base, out_a, out_b, out_sum);
}

int vpin_gens_msm(vpin_ctx* c, const vpin_gens* g, const uint8_t* scalars_mont, size_t rows, size_t ncols,
                  uint8_t* out_compressed, uint8_t* out_xyzt) {
  if (!c || !g || !scalars_mont || rows == 0 || ncols == 0 || (!out_compressed && !out_xyzt)) return VPIN_EINVAL;
  if (ncols > g->nb) return VPIN_ESHAPE;  // dalek asserts equal lengths (group.rs:105)
  (void)hipSetDevice(c->device);
  DevBuf ds(c), dpts(c), dout(c), dx(c);
  if (ds.alloc(rows * ncols * 32) || dpts.alloc(rows * sizeof(ge_ext)) || dout.alloc(rows * 32) || dx.alloc(rows * 128))
    return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(ds.p, scalars_mont, rows * ncols * 32, hipMemcpyHostToDevice, c->stream));
  int rc = msm_rows(c, g, (const fq*)ds.p, rows, ncols, ncols, nullptr, 0, 0, (ge_ext*)dpts.p);
  if (rc) return rc;
  hipLaunchKernelGGL(ge_compress_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, c->stream, (const ge_ext*)dpts.p,
                     rows, out_compressed ? (fp*)dout.p : (fp*)nullptr, out_xyzt ? (fp*)dx.p : (fp*)nullptr);
  VPIN_HIP_TRY(hipGetLastError());
  if (out_compressed) VPIN_HIP_TRY(hipMemcpyAsync(out_compressed, dout.p, rows * 32, hipMemcpyDeviceToHost, c->stream));
  if (out_xyzt) VPIN_HIP_TRY(hipMemcpyAsync(out_xyzt, dx.p, rows * 128, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

}  // extern "C"

namespace vpin {

// asynchronous form: kernels and the device-to-host copy are enqueued on the context's stream; `scratch` must hold
// rows * (raw_parts(ncols) + nparts) * 128 bytes and outlive them (gens_msm_parts_scratch_bytes)
size_t gens_msm_parts_scratch_bytes(size_t rows, size_t ncols) { return rows * (raw_parts(ncols) + vpin_gens_msm_parts_count(ncols)) * 128; }
int gens_msm_parts_launch(vpin_ctx* c, const vpin_gens* g, const fq* d_scalars, size_t rows, size_t ncols, void* scratch,
                          uint8_t* parts_xyzt, bool host_mapped) {
  if (!c || !g || !d_scalars || !parts_xyzt || !scratch || rows == 0 || ncols == 0) return VPIN_EINVAL;
  if (ncols > g->nb) return VPIN_ESHAPE;
  (void)hipSetDevice(c->device);
  const size_t nraw = raw_parts(ncols), nparts = vpin_gens_msm_parts_count(ncols);
  // host_mapped: parts_xyzt is pinned host memory, which the device addresses directly -- the last stage stores its
  // partial points there and the ~10 us copy command per call goes away (the caller waits for the stream instead)
  fp* dp = (fp*)scratch;
  fp* dr = (fp*)((uint8_t*)scratch + rows * nraw * 128);
  fp* first_out = (host_mapped && nraw == nparts) ? (fp*)parts_xyzt : dp;
  {
    ProfScope ps(c, VPIN_K_MSM, 32.0 * (double)rows * (double)ncols);
    if (wide_q(ncols) == 4)
      hipLaunchKernelGGL((msm_wide_kernel<4>), dim3((unsigned)nraw, (unsigned)rows), dim3(kMsmBlock), 0, c->stream, d_scalars, ncols,
                         view(g), first_out);
    else
      hipLaunchKernelGGL((msm_wide_kernel<1>), dim3((unsigned)nraw, (unsigned)rows), dim3(kMsmBlock), 0, c->stream, d_scalars, ncols,
                         view(g), first_out);
  }
  const void* src = first_out;
  if (nraw > nparts) {
    fp* second_out = host_mapped ? (fp*)parts_xyzt : dr;
    hipLaunchKernelGGL(parts_reduce_kernel, dim3((unsigned)((rows * nparts + 63) / 64)), dim3(64), 0, c->stream, (const fp*)dp, rows,
                       nraw, (int)nparts, second_out);
    src = second_out;
  }
  VPIN_HIP_TRY(hipGetLastError());
  if (src != (const void*)parts_xyzt) VPIN_HIP_TRY(hipMemcpyAsync(parts_xyzt, src, rows * nparts * 128, hipMemcpyDeviceToHost, c->stream));
  return VPIN_OK;
}

// one launch per bullet round (bullet_step_kernel); parts_pinned / up_pinned are pinned host memory.  R must be a multiple
// of 32.  R > 4096 (more than 128 MSM workgroups): dev_parts (2 x R/32 x 128 bytes of device memory) takes the workgroups'
// points and a second launch leaves R/4096 sums per side in parts_pinned (bullet_parts_reduce_kernel).
int bullet_step_launch(vpin_ctx* c, const vpin_gens* g, const fq* a_prev, const fq* b_prev, fq* a_next, fq* b_next, fq* sj, size_t n,
                       size_t R, bool fold, bool finish, const uint8_t* u, const uint8_t* u_inv, uint8_t* parts_pinned,
                       uint32_t* up_pinned, uint32_t seq, void* dev_parts) {
  if (!c || !g || !a_prev || !b_prev || !sj || !parts_pinned || !up_pinned || R % kWideScalars || R > g->nb) return VPIN_EINVAL;
  if (!finish && (n == 0 || 2 * n > R || !a_next || !b_next)) return VPIN_EINVAL;
  if ((fold || finish) && (!u || !u_inv)) return VPIN_EINVAL;
  const int nmsm = (int)(R / kWideScalars);
  const bool reduce = nmsm > 128;
  if (reduce && (!dev_parts || (nmsm & (nmsm - 1)))) return VPIN_EINVAL;
  (void)hipSetDevice(c->device);
  BulletStep a{};
  a.a_prev = a_prev; a.b_prev = b_prev; a.a_next = a_next; a.b_next = b_next; a.sj = sj;
  a.n = finish ? 0 : n; a.R = R; a.fold = fold ? 1 : 0; a.finish = finish ? 1 : 0;
  a.nmsm = nmsm;
  if (u) { memcpy(a.u.v, u, 32); memcpy(a.u_inv.v, u_inv, 32); }
  a.parts = reduce ? (fp*)dev_parts : (fp*)parts_pinned; a.up = up_pinned; a.seq = seq;
  const int nip = finish ? 1 : (int)((n + kMsmBlock - 1) / kMsmBlock);
  {
    ProfScope ps(c, VPIN_K_MSM, 32.0 * 2.0 * (double)R);
    hipLaunchKernelGGL(bullet_step_kernel, dim3((unsigned)(a.nmsm + nip)), dim3(kMsmBlock), 0, c->stream, a, view(g));
  }
  if (reduce)
    hipLaunchKernelGGL(bullet_parts_reduce_kernel, dim3((unsigned)(nmsm / 128), finish ? 1u : 2u), dim3(kMsmBlock), 0, c->stream,
                       (const fp*)dev_parts, nmsm, a.n, a.finish, (fp*)parts_pinned);
  VPIN_HIP_TRY(hipGetLastError());
  return VPIN_OK;
}

int gens_msm_parts_dev(vpin_ctx* c, const vpin_gens* g, const fq* d_scalars, size_t rows, size_t ncols, uint8_t* parts_xyzt) {
  if (!c || !g || !d_scalars || !parts_xyzt || rows == 0 || ncols == 0) return VPIN_EINVAL;
  if (ncols > g->nb) return VPIN_ESHAPE;
  (void)hipSetDevice(c->device);
  DevBuf scratch(c);
  if (scratch.alloc(gens_msm_parts_scratch_bytes(rows, ncols))) return VPIN_ENOMEM;
  if (const int rc = gens_msm_parts_launch(c, g, d_scalars, rows, ncols, scratch.p, parts_xyzt, false)) return rc;
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

}  // namespace vpin
