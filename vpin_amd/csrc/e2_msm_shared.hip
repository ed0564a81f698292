// e2_msm_shared.hip -- many linear combinations on E2 whose sums share their scalar vectors (vpin_e2_msm_shared, and the
// random-linear-combination sums of vpin_enc_conv2d and vpin_enc_conv2d_mc[_bias] where e2_rlc_shared_wins says so):
//
//     sum[s] = sum over t < n_terms of  r[vec[s]][t] * P[base[s] + off[pat[s]][t]]
//
// All sums of one vector see the same scalars and differ in their points alone, so a bucket walk needs no sorting pass and no
// divergence: the digit of r[vec][t] is the same for the 64 lanes of a wave, which are 64 sums of that vector.
//
//   e2_sh_window_kernel   one 256-lane workgroup per (tile of 64 sums of one vector, 3-bit window): wave b holds the bucket of
//                         magnitude b + 1 of every sum of the tile as ONE named accumulator per lane.  The loop over t reads the
//                         four scalar bits of the window through wave-uniform addresses (Booth digits -4 .. 4: digit w is
//                         -4 b[3w+2] + 2 b[3w+1] + b[3w] + b[3w-1], no carry between windows), branches uniformly, and on a hit
//                         every lane gathers its own point and does one e2_add_mixed, the sign applied to y.  No doubling in the
//                         loop.  The four buckets meet in LDS and wave 0 forms sum_v v * B_v by the running-sum rule
//                         Where the grid would not fill the device, sums of 512 terms or more are split into up to eight segments
//                         of terms, a workgroup each (one 256 x 256 plane: 50 sums of 65536 terms are 43 workgroups unsplit)
//   e2_sh_horner_kernel   one lane per sum: sum_w 8^w * window_w from the top window down, three doublings and one addition per
//                         segment each
//   e2_sh_offsets_kernel  the layers' pattern table from the window rule (E2Geom): off[k][t] for the taps k, and the row off[taps][t]
//                         = t for the sums over the outputs themselves.  Built on the device: no per-term array crosses from the host
// Exactness: every addition is complete by case (e2_dev.h): a bucket that receives the same point twice doubles it, P and -P
// cancel to the identity, flagged points and negative pattern entries add nothing.  The results go through e2_emit, so the bytes
// are the unique affine representatives.  The accumulators are named registers (one e2_jac per lane): no per-lane arrays.
// Memory: the per-window results are n_slots x windows x segments x 96 bytes from the context's pool; above kShCapBytes the tiles are taken
// in chunks of a fixed size, so the temporaries do not grow with the batch.  Everything runs on c->stream.
#include "e2_dev.h"
#include "enc_conv.h"

#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

namespace vpin {

namespace {

constexpr int kShWindow = 3;                       // bits per window: digits -4 .. 4, four bucket waves
constexpr int kShTile = 64;                        // sums per tile: one lane each
constexpr size_t kShCapBytes = (size_t)128 << 20;  // per-window results held at once (vpin_ctx_set_rlc_shared_cap: tests)
constexpr uint32_t kShNone = 0xffffffffu;          // an empty lane of a tile
// few long sums: while the grid has fewer than kShFullGrid workgroups (four a CU of an MI355X; at 176 VGPRs two are resident), the
// terms are split into segments of at least 256, eight at most, a workgroup each.  A full grid is not split: every segment pays
// the bucket combination and a Horner addition again (layer 0 of LeNet-5 at B = 32 split in four: 106 ms against 85)
constexpr size_t kShSegTerms = 256, kShMaxSegs = 8, kShFullGrid = 1024;

struct ShSets {
  const fq *X0, *Y0;
  const uint8_t* F0;
  const fq *X1, *Y1;
  const uint8_t* F1;
};

// desc[s] = {vec, pat, base, set}: pat < 0: no terms.  order: 64 sums per tile (kShNone: none), tile_vec: the tile's vector.
// The terms are taken in gridDim.z segments of seg terms.  wins[(z * windows + w) * n_slots + slot].  grid: x = tile, y = window, z = segment
__global__ __launch_bounds__(kE2Block) void e2_sh_window_kernel(ShSets ps, const int4* __restrict__ desc, const int32_t* __restrict__ off,
                                                                const uint32_t* __restrict__ r, const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ tile_vec, size_t n_slots, unsigned n_terms,
                                                                unsigned seg, fq a, e2_jac* __restrict__ wins) {
  __shared__ e2_jac sh[kE2Block];
  const int lane = threadIdx.x & 63;
  const uint32_t bucket = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + 1u;
  const unsigned tile = blockIdx.x, w = blockIdx.y;
  const size_t slot = (size_t)tile * kShTile + lane;
  const uint32_t s = order[slot];
  int4 d = make_int4(0, -1, 0, 0);
  if (s != kShNone) d = desc[s];
  const bool live = d.y >= 0;
  const int32_t* offp = off + (size_t)(live ? d.y : 0) * n_terms;
  const size_t base = (uint32_t)d.z;
  const fq* X = d.w ? ps.X1 : ps.X0;
  const fq* Y = d.w ? ps.Y1 : ps.Y0;
  const uint8_t* F = d.w ? ps.F1 : ps.F0;
  // the window's four bits 3w - 1 .. 3w + 2 of the 128-bit scalar: two words at most, the same for the whole workgroup
  const int pos = kShWindow * (int)w - 1, wi = pos < 0 ? 0 : pos >> 5, sh_r = pos < 0 ? 0 : pos & 31;
  const uint32_t* rw = r + (size_t)tile_vec[tile] * n_terms * 4 + wi;
  e2_jac acc = e2_identity();
  const unsigned t0 = blockIdx.z * seg, t1 = t0 + seg < n_terms ? t0 + seg : n_terms;
  for (unsigned t = t0; t < t1; t++) {
    const uint32_t lo = rw[4 * (size_t)t], hi = wi < 3 ? rw[4 * (size_t)t + 1] : 0u;
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)((pos < 0 ? (uint32_t)(both << 1) : (uint32_t)(both >> sh_r)) & 0xfu));
    const uint32_t half = ((v & 7u) + 1u) >> 1, mag = (v & 8u) ? 4u - half : half;
    if (mag != bucket) continue;  // the same for every lane of the wave
    if (!live) continue;
    const int32_t o = offp[t];
    if (o < 0) continue;  // no term: padding
    const size_t idx = base + (size_t)o;
    if (F[idx]) continue;  // a flagged point is the identity
    const fq y = fq_load(Y + idx);
    acc = e2_add_mixed(acc, fq_load(X + idx), (v & 8u) ? fq_neg(y) : y, a);
  }
  e2_store(&sh[threadIdx.x], acc);
  __syncthreads();
  if (threadIdx.x >= 64) return;
  // sum_v v * B_v: run = B4, B4 + B3, ..; the total adds every run
  e2_jac run = e2_load(&sh[192 + lane]), tot = run;
  run = e2_add(run, e2_load(&sh[128 + lane]), a); tot = e2_add(tot, run, a);
  run = e2_add(run, e2_load(&sh[64 + lane]), a);  tot = e2_add(tot, run, a);
  run = e2_add(run, acc, a);                      tot = e2_add(tot, run, a);
  e2_store(wins + ((size_t)blockIdx.z * gridDim.y + w) * n_slots + slot, tot);
}

// one lane per slot: out[order[slot]] = sum_w 8^w * sum_z wins[z][w][slot]
__global__ __launch_bounds__(kE2Block) void e2_sh_horner_kernel(const e2_jac* __restrict__ wins, const uint32_t* __restrict__ order,
                                                                size_t n_slots, int n_win, int n_seg, fq a, e2_jac* __restrict__ out) {
  const size_t slot = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (slot >= n_slots) return;
  const uint32_t s = order[slot];
  if (s == kShNone) return;
  e2_jac acc = e2_identity();
  for (int w = n_win - 1; w >= 0; w--) {
    if (!e2_is_identity(acc)) {
      acc = e2_dbl(acc, a); acc = e2_dbl(acc, a); acc = e2_dbl(acc, a);
    }
    for (int z = 0; z < n_seg; z++) acc = e2_add(acc, e2_load(wins + ((size_t)z * n_win + w) * n_slots + slot), a);
  }
  e2_store(out + s, acc);
}

// grid: x = blocks of outputs, y = pattern (taps + 1 of them)
__global__ __launch_bounds__(kE2Block) void e2_sh_offsets_kernel(E2Geom g, int taps, unsigned n_terms, int32_t* __restrict__ off) {
  const unsigned t = blockIdx.x * kE2Block + threadIdx.x, k = blockIdx.y;
  if (t >= n_terms) return;
  off[(size_t)k * n_terms + t] = (int)k == taps ? (int32_t)t : (int32_t)e2_window_index(g, (int)t, (int)k);
}

int sh_windows(int scalar_bits) { return (scalar_bits + 1 + kShWindow - 1) / kShWindow; }

// The core.  desc: n_sums x {vec, pat, base, set} on the host, every vec < n_vec, every address inside its set (the callers'
// duty); off, r: on the device; out: n_sums Jacobian sums in the caller's order.  Orders the sums by vector into tiles of 64,
// takes the tiles in chunks under the cap.  Synchronises once, before its host staging goes away
int sh_run(vpin_ctx* c, const ShSets& ps, const int32_t* desc, size_t n_sums, size_t n_vec, const int32_t* off, size_t n_terms,
           const uint32_t* r, int scalar_bits, e2_jac* out) {
  const int n_win = sh_windows(scalar_bits);
  std::vector<size_t> first(n_vec + 1, 0);  // tiles before vector v
  std::vector<uint32_t> cnt(n_vec, 0);
  for (size_t s = 0; s < n_sums; s++) cnt[(uint32_t)desc[4 * s]]++;
  for (size_t v = 0; v < n_vec; v++) first[v + 1] = first[v] + (cnt[v] + kShTile - 1) / kShTile;
  const size_t n_tiles = first[n_vec];
  std::vector<uint32_t> order(n_tiles * kShTile, kShNone), tile_vec(n_tiles);
  std::fill(cnt.begin(), cnt.end(), 0u);
  for (size_t s = 0; s < n_sums; s++) {
    const uint32_t v = (uint32_t)desc[4 * s];
    order[first[v] * kShTile + cnt[v]++] = (uint32_t)s;
  }
  for (size_t v = 0; v < n_vec; v++)
    for (size_t t = first[v]; t < first[v + 1]; t++) tile_vec[t] = (uint32_t)v;
  const size_t wgs = n_tiles * n_win;
  const size_t n_seg = std::max<size_t>(1, std::min({kShMaxSegs, n_terms / kShSegTerms, (kShFullGrid + wgs - 1) / wgs}));
  const size_t seg = (n_terms + n_seg - 1) / n_seg;
  const size_t cap = c->rlc_shared_cap ? c->rlc_shared_cap : kShCapBytes, per_tile = (size_t)kShTile * n_win * n_seg * sizeof(e2_jac);
  const size_t chunk = std::min(n_tiles, std::max<size_t>(1, cap / per_tile));
  DevBuf ds(c), ord(c), tv(c), wins(c);
  if (ds.alloc(n_sums * 16) || ord.alloc(order.size() * 4) || tv.alloc(n_tiles * 4) || wins.alloc(chunk * per_tile)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(ds.p, desc, n_sums * 16, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(ord.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(tv.p, tile_vec.data(), n_tiles * 4, hipMemcpyHostToDevice, c->stream));
  const fq a = e2_curve_a();
  for (size_t t0 = 0; t0 < n_tiles; t0 += chunk) {
    const size_t nt = std::min(chunk, n_tiles - t0), n_slots = nt * kShTile;
    hipLaunchKernelGGL(e2_sh_window_kernel, dim3((unsigned)nt, (unsigned)n_win, (unsigned)n_seg), dim3(kE2Block), 0, c->stream, ps, (const int4*)ds.p,
                       off, r, (const uint32_t*)ord.p + t0 * kShTile, (const uint32_t*)tv.p + t0, n_slots, (unsigned)n_terms, (unsigned)seg, a,
                       (e2_jac*)wins.p);
    VPIN_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(e2_sh_horner_kernel, dim3(blocks_of(n_slots, kE2Block)), dim3(kE2Block), 0, c->stream, (const e2_jac*)wins.p,
                       (const uint32_t*)ord.p + t0 * kShTile, n_slots, n_win, (int)n_seg, a, out);
    VPIN_HIP_TRY(hipGetLastError());
  }
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  c->rlc_shared_sums += n_sums;
  return VPIN_OK;
}

}  // namespace

// THE selection rule between the one-lane-per-term kernels (e2_rlc_kernel, e2_rlc_mc_kernel) and the shared-scalar walk, a
// function of the shape alone (the thresholds are the least measured points of the sweep in
// profiles/r23_rlc_shared_sweep.txt at which the walk's median was not above the old kernels' at any larger point).  A tile
// costs the same whether 1 or 64 of its lanes hold a sum, and every sum pays the Horner pass (4 operations per window) however
// few terms it has; the old kernels pay 1.5 operations per scalar bit and term.  So the walk wins once a vector's sums fill a fair
// part of a wave and a sum has more than a few terms.  Both sides scale with scalar_bits alike: it only has to fill one window
bool e2_rlc_shared_wins(size_t sums_per_vec, size_t n_terms, int scalar_bits) {
  return sums_per_vec >= 17 && n_terms >= 9 && scalar_bits >= kShWindow;
}

int e2_rlc_shared(vpin_ctx* c, const E2Points& in, const E2Points& out, const ConvGeom& g, const int32_t* desc, size_t n_sums, size_t n_pairs,
                  const void* r_dev, int scalar_bits, e2_jac* sums) {
  const size_t n_terms = g.oh * g.ow, taps = g.taps(), per = g.H * g.W;
  std::vector<int32_t> d(4 * n_sums);
  for (size_t s = 0; s < n_sums; s++) {  // {plane, tap, pair, 0} -> {vec, pat, base, set}
    const int32_t plane = desc[4 * s], tap = desc[4 * s + 1], pair = desc[4 * s + 2];
    d[4 * s] = pair;
    d[4 * s + 1] = plane >= 0 ? tap : plane == -1 ? (int32_t)taps : -1;
    d[4 * s + 2] = (int32_t)(uint32_t)(plane >= 0 ? (size_t)plane * per : (size_t)pair * n_terms);
    d[4 * s + 3] = plane == -1;
  }
  DevBuf off(c);
  if (off.alloc((taps + 1) * n_terms * 4)) return VPIN_ENOMEM;
  hipLaunchKernelGGL(e2_sh_offsets_kernel, dim3(blocks_of(n_terms, kE2Block), (unsigned)(taps + 1)), dim3(kE2Block), 0, c->stream, e2_geom(g),
                     (int)taps, (unsigned)n_terms, (int32_t*)off.p);
  VPIN_HIP_TRY(hipGetLastError());
  const ShSets ps{in.X(), in.Y(), in.F(), out.X(), out.Y(), out.F()};
  return sh_run(c, ps, d.data(), n_sums, n_pairs, (const int32_t*)off.p, n_terms, (const uint32_t*)r_dev, scalar_bits, sums);
}

}  // namespace vpin

using namespace vpin;

extern "C" {

unsigned long long vpin_ctx_rlc_shared_sums(vpin_ctx* c) { return c ? c->rlc_shared_sums : 0ull; }

int vpin_ctx_set_rlc_shared_cap(vpin_ctx* c, size_t bytes) {
  if (!c) return enc::fail(VPIN_EINVAL, "vpin_ctx_set_rlc_shared_cap: null argument");
  c->rlc_shared_cap = bytes;
  return VPIN_OK;
}

int vpin_e2_msm_shared(vpin_ctx* c, const uint8_t* scalars_le16, size_t n_vec, size_t n_terms, int scalar_bits, const uint8_t* px,
                       const uint8_t* py, const uint8_t* pinf, size_t n_points, const int32_t* off, size_t n_pat, const uint32_t* vec,
                       const uint32_t* pat, const uint32_t* base, size_t n_sums, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  const std::string name("vpin_e2_msm_shared: ");
  auto failed = [&](const char* why) { return enc::fail(VPIN_EINVAL, (name + why).c_str()); };
  if (!c || !scalars_le16 || !px || !py || !pinf || !off || !vec || !pat || !base || !out_x || !out_y || !out_inf) return failed("null argument");
  if (!n_vec || !n_terms || !n_points || !n_pat || !n_sums) return failed("a count is zero");
  const size_t lim = ((size_t)1 << 31) - 1;
  if (n_sums > lim || n_terms > lim || n_sums * n_terms > lim) return failed("n_sums or n_sums * n_terms is above 2^31 - 1");
  if (n_vec > lim || n_pat > lim || n_points > lim || n_vec * n_terms > lim || n_pat * n_terms > lim) return failed("a count is above 2^31 - 1");
  if (scalar_bits < 1 || scalar_bits > 128) return failed("scalar_bits must be in 1 .. 128");
  for (size_t i = 0; i < n_vec * n_terms; i++)  // a set bit at or above scalar_bits: the walk skips those windows
    for (int b = 15; 8 * b + 7 >= scalar_bits; b--) {
      const uint8_t v = scalars_le16[16 * i + b];
      if (8 * b >= scalar_bits ? v != 0 : (v >> (scalar_bits - 8 * b)) != 0) return failed("a scalar has a set bit at or above scalar_bits");
    }
  // the addresses: per pattern its largest entry (a negative one is no term), -1 when it has none
  std::vector<int64_t> hi(n_pat, -1);
  for (size_t p = 0; p < n_pat; p++)
    for (size_t t = 0; t < n_terms; t++) hi[p] = std::max<int64_t>(hi[p], off[p * n_terms + t]);
  std::vector<int32_t> desc(4 * n_sums);
  for (size_t s = 0; s < n_sums; s++) {
    if (vec[s] >= n_vec) return failed("vec[s] is not below n_vec");
    if (pat[s] >= n_pat) return failed("pat[s] is not below n_pat");
    const bool none = hi[pat[s]] < 0;  // a pattern with no term reads no point
    if (!none && (uint64_t)base[s] + (uint64_t)hi[pat[s]] >= n_points) return failed("an address base + off is outside the points");
    desc[4 * s] = (int32_t)vec[s];
    desc[4 * s + 1] = none ? -1 : (int32_t)pat[s];
    desc[4 * s + 2] = (int32_t)base[s];
    desc[4 * s + 3] = 0;
  }
  (void)hipSetDevice(c->device);
  E2Points pts(c);
  int rc = pts.load(c, px, py, pinf, n_points, "vpin_e2_msm_shared", "point");
  if (rc) return rc;
  DevBuf r(c), od(c), sums(c);
  if (r.alloc(n_vec * n_terms * 16) || od.alloc(n_pat * n_terms * 4) || sums.alloc(n_sums * sizeof(e2_jac))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(r.p, scalars_le16, n_vec * n_terms * 16, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(od.p, off, n_pat * n_terms * 4, hipMemcpyHostToDevice, c->stream));
  const ShSets ps{pts.X(), pts.Y(), pts.F(), pts.X(), pts.Y(), pts.F()};
  if ((rc = sh_run(c, ps, desc.data(), n_sums, n_vec, (const int32_t*)od.p, n_terms, (const uint32_t*)r.p, scalar_bits, (e2_jac*)sums.p))) return rc;
  return e2_emit(c, (const e2_jac*)sums.p, n_sums, out_x, out_y, out_inf);
}

}  // extern "C"
