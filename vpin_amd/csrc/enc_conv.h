// enc_conv.h -- what the encrypted layers share.  Device side (enc_conv.hip, enc_fc.hip, enc_convmc.hip, enc_add.hip; also used by lenet.hip
// and e2_client.hip): E2Points, a set of affine points resident on the device; E2Affine / e2_emit, the one path from Jacobian
// results to canonical bytes on the host; EncConvDev, the stages of one layer.  Host side (enc_conv.cpp, for enc_fc.cpp and
// enc_convmc.cpp too): E2 on the host, the PRF, the frame of a layer driver and the tail that writes a chain of additions
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "host/field.h"

struct vpin_conv_trace;

namespace vpin {

struct ConvGeom {
  size_t P = 1, H = 0, W = 0, fh = 0, fw = 0, pad = 0, stride = 1, oh = 0, ow = 0;
  size_t pixels() const { return P * H * W; }
  size_t outputs() const { return P * oh * ow; }
  size_t taps() const { return fh * fw; }
};

constexpr uint32_t kE2FlagRange = 1u;     // a coordinate >= q
constexpr uint32_t kE2FlagOffCurve = 2u;  // a non-identity point that does not satisfy the curve equation

struct fq;
struct e2_jac;
struct E2Geom;

// n affine points resident on the device: Montgomery coordinates (n x 32 bytes each) and one flag byte per point, 1 = the
// identity (its coordinates are then not read).  Filled by load() from the caller's bytes or by a normalisation (E2Affine)
struct E2Points {
  DevBuf x, y, inf;
  size_t n = 0;
  explicit E2Points(vpin_ctx* c) : x(c), y(c), inf(c) {}
  // x, y: n x 32 canonical little-endian bytes; inf: n flag bytes.  Upload, e2_load_kernel (Montgomery form, range and curve
  // checks), one synchronisation.  VPIN_EINVAL with "<who>: a coordinate is not below q" or "<who>: a <what> is not on the
  // curve E2" when a point is rejected
  int load(vpin_ctx* c, const uint8_t* x, const uint8_t* y, const uint8_t* inf, size_t n, const char* who = "enc_conv",
           const char* what = "pixel");
  int resize(size_t n);  // fresh buffers for n points
  const fq* X() const { return (const fq*)x.p; }
  const fq* Y() const { return (const fq*)y.p; }
  const uint8_t* F() const { return (const uint8_t*)inf.p; }
};

// The one way from Jacobian results to the host.  normalise: ONE e2_to_affine_kernel launch over n points into buffers this
// object owns; with `keep` the Montgomery coordinates and the flags go into *keep and stay resident there.  copy_out: the
// canonical bytes and flags of the points [first, first + count) to three host pointers (inf may be NULL: no flags wanted).
// Neither synchronises; the object has to live until the caller has synchronised
struct E2Affine {
  DevBuf mx, my, cx, cy, fl;
  const uint8_t* flags = nullptr;  // fl, or keep's
  explicit E2Affine(vpin_ctx* c) : mx(c), my(c), cx(c), cy(c), fl(c) {}
  int normalise(vpin_ctx* c, const e2_jac* jac, size_t n, E2Points* keep = nullptr);
  int copy_out(vpin_ctx* c, size_t first, size_t count, uint8_t* x, uint8_t* y, uint8_t* inf) const;
};
// normalise, copy all n points out, synchronise
int e2_emit(vpin_ctx* c, const e2_jac* jac, size_t n, uint8_t* x, uint8_t* y, uint8_t* inf, E2Points* keep = nullptr);

// The device stages of one layer over `in`, the loaded inputs (in.load).  Every stage synchronises the context's stream once,
// before it returns.  conv, matvec and conv_mc read `in` and leave their normalised results resident in `out` (and set g);
// rlc and rlc_mc read both; add_bias reads `out`; msm and pool_sums read `in` alone.
//   conv       out[p][i][j] = sum_k w[k] * X[p][i s + ii][j s + jj] (e2_conv_kernel); canonical bytes to the host
//   rlc        for every plane the taps() + 1 sums  sum_t r[p][t] * window[t][k]  and  sum_t r[p][t] * out[p][t]
//              (e2_rlc_kernel + e2_reduce_kernel), returned as Jacobian Montgomery triples: (P x (taps() + 1)) x 96 bytes
//   msm        rlc with no taps over `in` itself: one sum of n terms
//   matvec     C[p][j] = sum_k W[k][j] * X[p][k] for P rows of K points (e2_matvec_kernel<is_signed>); weights: K x N words
//              row-major, u32 or int32 (a negative weight adds |w| times the negated point).  `out` is C as P planes of 1 x N
//              with no taps, so rlc gives sum_j r[p][j] * C[p][j] per row
//   pool_sums  per pooled output (geom: fh = fw = k, pad 0) its taps() - 1 accumulators e_0, e_0 + e_1, .. in the order of the
//              addition list, normalised, canonical bytes; acc_identity: one byte per output, 1 = one of them is the identity
//   conv_mc    `in` as groups x C planes: out[g][o][t] = sum over the connected c and the taps k of w[o][c][k] *
//              window_t(X[g][c])[k] (e2_convmc_kernel); the groups * n_out planes as canonical bytes to the host.  w: n_out * C *
//              taps() int32, connect: n_out * C bytes (never NULL here), top_bit: per o the top set bit of its largest |w| over
//              the connected channels, -1 when all are zero
//   add_bias   after conv_mc, bias: groups * n_out loaded points: res[plane][t] = out[plane][t] + bias[plane]
//              (e2_bias_add_kernel, the complete addition), canonical bytes to the host.  `out` stays C: the check runs over C
//   rlc_mc     n_sums sums, one descriptor of four ints each: {plane, tap, pair, 0}.  plane >= 0: sum_t r[pair][t] *
//              window_t(X[plane])[tap]; plane = -1: sum_t r[pair][t] * out[pair][t]; plane = -2: no terms (the padding of a
//              chain).  neg[i] != 0 negates sum i (e2_negate_kernel).  All sums are normalised by one launch: canonical bytes and
//              flags to the host, and they stay resident in *sums, ready for mul_chain
// rlc and rlc_mc take scalar_bits, a bound on their scalars (8 * prf_bytes), and go through the shared-scalar walk
// (e2_msm_shared.hip) where e2_rlc_shared_wins says so: the sums are the same group elements either way
struct EncConvDev {
  vpin_ctx* c;
  ConvGeom g;
  E2Points in, out;
  explicit EncConvDev(vpin_ctx* ctx) : c(ctx), in(ctx), out(ctx) {}
  int conv(const ConvGeom& geom, const uint8_t* filter_le16, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int rlc(const uint8_t* r_le16, uint8_t* sums_jac, int scalar_bits = 128);
  int msm(const uint8_t* r_le16, size_t n, uint8_t sum_jac[96]);
  int matvec(size_t P, size_t K, size_t N, const void* weights, bool is_signed, uint8_t* c_x, uint8_t* c_y, uint8_t* c_inf);
  int pool_sums(const ConvGeom& geom, uint8_t* acc_x, uint8_t* acc_y, uint8_t* acc_identity);
  int conv_mc(const ConvGeom& geom, size_t groups, size_t C, size_t n_out, const int32_t* w, const uint8_t* connect, const int32_t* top_bit,
              uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int add_bias(const E2Points& bias, size_t groups, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int rlc_mc(size_t n_pairs, const int32_t* desc, const uint8_t* neg, size_t n_sums, const uint8_t* r_le16, E2Points* sums, uint8_t* s_x,
             uint8_t* s_y, uint8_t* s_inf, int scalar_bits = 128);
};

// The tail of a layer's RLC check, also vpin_e2_mul_chain (enc_fc.hip: e2_scalar_mul_kernel, e2_chain_scan_kernel, one
// normalisation): P chains of K terms over pts, T[p][k] = s[p][k] * X[p][k] and the inclusive prefixes acc[p][k] = T[p][0] + ..
// + T[p][k], both as canonical bytes with identity flags (P * K points each).  Synchronises once
int mul_chain(vpin_ctx* c, const E2Points& pts, const uint8_t* s_le16, size_t P, size_t K, uint8_t* t_x, uint8_t* t_y, uint8_t* t_inf,
              uint8_t* acc_x, uint8_t* acc_y, uint8_t* acc_inf);

// The addition layer's stage (enc_add.hip: e2_pair_add_kernel, one normalisation): out[p][t] = x[p][t] + r[p][t] over P planes of
// per_plane loaded points each, the complete addition, canonical bytes and flags to the host; bad_plane: P bytes, 1 = an x of
// that plane is the identity (the scan of the first operands' flags, on the device).  Synchronises once
int e2_pair_add(vpin_ctx* c, const E2Points& x, const E2Points& r, size_t P, size_t per_plane, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf,
                uint8_t* bad_plane);

// What the other .hip files take from enc_conv.hip (types: fq_dev.h, e2_dev.h): a device constant from 32 canonical
// little-endian bytes, the curve coefficient a (both in Montgomery form), the geometry as the kernels take it, and the launches
// of e2_to_affine_kernel (n points) and e2_reduce_kernel (n_sums sums of n_parts partials each) on the context's stream, not
// synchronised
fq fq_of_le32(const uint8_t* le32);
fq e2_curve_a();
E2Geom e2_geom(const ConvGeom& g);
int e2_to_affine(vpin_ctx* c, const e2_jac* in, size_t n, fq* mx, fq* my, fq* cx, fq* cy, uint8_t* oinf);
int e2_reduce(vpin_ctx* c, const e2_jac* parts, size_t n_sums, size_t n_parts, e2_jac* out);

// e2_msm_shared.hip: the selection rule between the one-lane-per-term kernels and the shared-scalar walk (stated there), and the
// layers' sums through the walk: desc as rlc_mc takes it, n_pairs vectors of oh * ow scalars at r_dev, n_sums Jacobian sums to `sums`
// in the order of desc.  Synchronises
bool e2_rlc_shared_wins(size_t sums_per_vec, size_t n_terms, int scalar_bits);
int e2_rlc_shared(vpin_ctx* c, const E2Points& in, const E2Points& out, const ConvGeom& g, const int32_t* desc, size_t n_sums, size_t n_pairs,
                  const void* r_dev, int scalar_bits, e2_jac* sums);

inline unsigned blocks_of(size_t n, int b) { return (unsigned)((n + b - 1) / b); }

#define VPIN_EC_ALLOC(buf, bytes) do { (buf).release(); if ((buf).alloc((bytes) ? (bytes) : 16)) return VPIN_ENOMEM; } while (0)

void set_last_error_text(const char* text);

// ---- the host side the layer drivers share (defined in enc_conv.cpp) ------------------------------------------------
namespace enc {

using vpin_host::Fq;

// E2 on the host: affine in and out, complete by case
struct Aff {
  Fq x = Fq::zero(), y = Fq::zero();
  bool inf = true;
};
struct Jac {
  Fq X, Y, Z;
  bool inf() const { return Z.is_zero(); }
};
Aff to_affine(const Jac& p);
Aff aff_add(const Aff& p, const Aff& q);
Jac jac_from_bytes(const uint8_t* p);  // a Jacobian Montgomery triple as rlc returns it
Aff aff_from_bytes(const uint8_t* x, const uint8_t* y, uint8_t inf);  // canonical little-endian coordinates and the flag
void put_point(const Aff& p, uint8_t* x, uint8_t* y);  // canonical little-endian; the identity is written as zeros

int fail(int code, const char* why);  // records why for vpin_last_error() and returns code
constexpr size_t kMaxDim = (size_t)1 << 24;  // no dimension above it; no more than 65535 planes or rows (a grid axis)
int make_geom(size_t P, size_t H, size_t W, size_t fh, size_t fw, size_t pad, size_t stride, ConvGeom* g);
int team_size();                       // threads of the host team
double* reset_timings();               // the 8 slots of vpin_enc_conv_last_timings (per thread), zeroed: every driver's first step
// the rows * per_row scalars of a layer's check, 16 bytes each: row i under the key keys32 + 32 i, the index t restarting at 0 in
// every row (one OpenMP team).  r_t = int.from_bytes(HMAC-SHA256(key, ascii_decimal(t))[:prf_bytes], "big") as a little-endian u128
std::vector<uint8_t> prf_rows(const uint8_t* keys32, size_t rows, size_t per_row, int prf_bytes);

// points as canonical little-endian bytes with a flag byte each; the identity is zeros and flag 1
struct PointBytes {
  const uint8_t *x, *y, *inf;
  PointBytes at(size_t i) const { return PointBytes{x + 32 * i, y + 32 * i, inf + i}; }
};
// One chain of a layer's check into the trace: prod, prefix: its len products T_k and inclusive prefixes T_0 + .. + T_k.  Writes
// the len - 1 additions (prefix k - 1, T_k, rz = T_k's flag) from index *ai on and advances *ai.  VPIN_ESHAPE with
// "<who>: an addition accumulator is the identity .." when a prefix before a step is the identity; the last prefix may be: it is
// only compared.  *closes: the last prefix equals left[0] (flag and both coordinates)
int emit_chain(const char* who, vpin_conv_trace* t, size_t* ai, PointBytes prod, PointBytes prefix, size_t len, PointBytes left, bool* closes);

// The units (planes, groups, rows) that break a VPIN_ESHAPE rule, for vpin_enc_last_refusals: per thread, like the error text.
// Every layer entry point clears the list first; a scan that refuses notes every unit that breaks its rule and then returns the
// first hit's code and text, so the list holds the units of the ONE stage that refused
void clear_refusals();
void note_refusal(size_t unit);

struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double operator()() {
    const auto n = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(n - t).count();
    t = n;
    return s;
  }
};

}  // namespace enc

}  // namespace vpin

// what every encrypted layer returns (vpin_enc_conv2d, vpin_enc_conv2d_mc[_bias], vpin_enc_fc[_signed], vpin_enc_avgpool2d, vpin_enc_add)
struct vpin_conv_trace {
  size_t P = 0, oh = 0, ow = 0, n_mult = 0, n_add = 0;
  std::vector<uint8_t> out_x, out_y, out_inf;        // P * oh * ow
  std::vector<uint8_t> m_w, m_px, m_py;              // n_mult
  std::vector<uint8_t> a_px, a_py, a_rx, a_ry, a_rz; // n_add
  std::vector<uint8_t> left_x, left_y, left_inf;     // P, or none (pooling)
  void resize_lists() {
    m_w.resize(n_mult * 16); m_px.resize(n_mult * 32); m_py.resize(n_mult * 32);
    a_px.resize(n_add * 32); a_py.resize(n_add * 32); a_rx.resize(n_add * 32); a_ry.resize(n_add * 32); a_rz.resize(n_add);
  }
};
