// enc_conv.h -- device stages of the encrypted layers (enc_conv.hip, enc_fc.hip), driven by enc_conv.cpp and enc_fc.cpp, and
// the host pieces the two drivers share (E2 on the host, the PRF, the trace)
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "host/field.h"

namespace vpin {

struct ConvGeom {
  size_t P = 1, H = 0, W = 0, fh = 0, fw = 0, pad = 0, stride = 1, oh = 0, ow = 0;
  size_t pixels() const { return P * H * W; }
  size_t outputs() const { return P * oh * ow; }
  size_t taps() const { return fh * fw; }
};

constexpr uint32_t kE2FlagRange = 1u;     // a coordinate >= q
constexpr uint32_t kE2FlagOffCurve = 2u;  // a non-identity point that does not satisfy the curve equation

// The device side of one layer.  Stages run in this order, each synchronises the context's stream before it returns:
//   load   pixels (x, y: n x 32 LE bytes; inf: n flag bytes) -> Montgomery coordinates in HBM, range and curve checks
//   conv   out[p][i][j] = sum_k w[k] * X[p][i s + ii][j s + jj] (e2_conv_kernel), normalised to affine (batched inversion);
//          the outputs stay resident for rlc and are copied to the host as canonical bytes
//   rlc    for every plane the taps() + 1 sums  sum_t r[p][t] * window[t][k]  and  sum_t r[p][t] * out[p][t]
//          (e2_rlc_kernel + e2_reduce_kernel), returned as Jacobian Montgomery triples: (P x (taps() + 1)) x 96 bytes
// msm is rlc with no taps over the loaded points themselves: one sum of n terms.
// The fully connected layer and the pooling (enc_fc.hip) run over the loaded points too:
//   matvec      C[p][j] = sum_k W[k][j] * X[p][k] for P rows of K points and u32 weights (K x N row-major, little-endian),
//               normalised; C takes conv's place as the resident outputs (P planes of 1 x N, no taps), so rlc gives
//               sum_j r[p][j] * C[p][j] per row
//   matvec_signed  matvec over int32 weights (e2_matvec_signed_kernel): a negative weight adds |w| times the negated point
//   pool_sums   per pooled output (geom: fh = fw = k, pad 0) its taps() - 1 accumulators e_0, e_0 + e_1, .. in the order of
//               the addition list, normalised, canonical bytes; acc_identity: one byte per output, 1 = one of them is the identity
// The tail of the fully connected layer's RLC check, also vpin_e2_mul_chain (enc_fc.hip: e2_scalar_mul_kernel,
// e2_chain_scan_kernel, one e2_to_affine_kernel launch):
//   mul_chain   P chains of K terms over the loaded points: T[p][k] = s[p][k] * X[p][k] and the inclusive prefixes
//               acc[p][k] = T[p][0] + .. + T[p][k], both as canonical bytes with identity flags (P * K points each)
// The convolution with one signed filter per (output channel, input channel) and its sums (enc_convmc.hip), over the loaded
// points as groups x C planes (this->g after conv_mc: P = groups * C):
//   conv_mc     out[g][o][t] = sum over the connected c and the taps k of w[o][c][k] * window_t(X[g][c])[k] (e2_convmc_kernel),
//               normalised; the groups * n_out output planes stay resident for rlc_mc and go to the host as canonical bytes.
//               w: n_out * C * taps() int32, connect: n_out * C bytes (never NULL here), top_bit: per o the top set bit of its
//               largest |w| over the connected channels, -1 when all are zero
//   add_bias    after conv_mc, with `bias` holding the groups * n_out loaded bias points: out[plane][t] = C[plane][t] +
//               bias[plane] (e2_bias_add_kernel, the complete addition), normalised, canonical bytes to the host.  The resident
//               outputs stay C: the check runs over C, not out
//   rlc_mc      n_sums sums, one descriptor of four ints each: {plane, tap, pair, 0}.  plane >= 0: sum_t r[pair][t] *
//               window_t(X[plane])[tap]; plane = -1: sum_t r[pair][t] * out[pair][t]; plane = -2: no terms (the padding of a
//               chain).  neg[i] != 0 negates sum i (e2_negate_kernel).  All sums are normalised by one launch: canonical bytes and
//               flags to the host, and the Montgomery coordinates become tail's loaded points, ready for tail->mul_chain
struct EncConvDev {
  vpin_ctx* c;
  ConvGeom g;
  DevBuf px, py, pinf, ox, oy, oinf, filt;
  explicit EncConvDev(vpin_ctx* ctx) : c(ctx), px(ctx), py(ctx), pinf(ctx), ox(ctx), oy(ctx), oinf(ctx), filt(ctx) {}
  int load(const uint8_t* x, const uint8_t* y, const uint8_t* inf, size_t n, uint32_t* flags);
  int conv(const ConvGeom& geom, const uint8_t* filter_le16, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int rlc(const uint8_t* r_le16, uint8_t* sums_jac);
  int msm(const uint8_t* r_le16, size_t n, uint8_t sum_jac[96]);
  int matvec(size_t P, size_t K, size_t N, const uint8_t* weights_le4, uint8_t* c_x, uint8_t* c_y, uint8_t* c_inf);
  int matvec_signed(size_t P, size_t K, size_t N, const int32_t* weights, uint8_t* c_x, uint8_t* c_y, uint8_t* c_inf);
  int matvec_any(size_t P, size_t K, size_t N, const void* weights, bool is_signed, uint8_t* c_x, uint8_t* c_y, uint8_t* c_inf);
  int pool_sums(const ConvGeom& geom, uint8_t* acc_x, uint8_t* acc_y, uint8_t* acc_identity);
  int mul_chain(const uint8_t* s_le16, size_t P, size_t K, uint8_t* t_x, uint8_t* t_y, uint8_t* t_inf, uint8_t* acc_x, uint8_t* acc_y,
                uint8_t* acc_inf);
  int conv_mc(const ConvGeom& geom, size_t groups, size_t C, size_t n_out, const int32_t* w, const uint8_t* connect, const int32_t* top_bit,
              uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int add_bias(const EncConvDev& bias, size_t groups, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int rlc_mc(size_t n_pairs, const int32_t* desc, const uint8_t* neg, size_t n_sums, const uint8_t* r_le16, EncConvDev* tail, uint8_t* s_x,
             uint8_t* s_y, uint8_t* s_inf);
};

// What enc_fc.hip takes from enc_conv.hip (types: fq_dev.h, e2_dev.h): the curve coefficient a in Montgomery form, the
// geometry as the kernels take it, and the launches of e2_to_affine_kernel (n points) and e2_reduce_kernel (n_sums sums of
// n_parts partials each) on the context's stream, not synchronised
struct fq;
struct e2_jac;
struct E2Geom;
fq e2_curve_a();
E2Geom e2_geom(const ConvGeom& g);
int e2_to_affine(vpin_ctx* c, const e2_jac* in, size_t n, fq* mx, fq* my, fq* cx, fq* cy, uint8_t* oinf);
int e2_reduce(vpin_ctx* c, const e2_jac* parts, size_t n_sums, size_t n_parts, e2_jac* out);

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
bool aff_eq(const Aff& p, const Aff& q);
Jac jac_from_bytes(const uint8_t* p);  // a Jacobian Montgomery triple as rlc returns it
Aff aff_from_bytes(const uint8_t* x, const uint8_t* y, uint8_t inf);  // canonical little-endian coordinates and the flag
void put_point(const Aff& p, uint8_t* x, uint8_t* y);  // canonical little-endian; the identity is written as zeros

// r_t = int.from_bytes(HMAC-SHA256(key, ascii_decimal(t))[:prf_bytes], "big") as a little-endian u128
void prf_scalar(const uint8_t key[32], size_t t, int prf_bytes, uint8_t out_le16[16]);

int fail(int code, const char* why);  // records why for vpin_last_error() and returns code
// the flag word of EncConvDev::load as a rejection: VPIN_EINVAL and "<who>: a <what> is not on the curve E2" or the range rule
int check_flags(uint32_t flags, const char* who = "enc_conv", const char* what = "pixel");
constexpr size_t kMaxDim = (size_t)1 << 24;  // no dimension above it; no more than 65535 planes or rows (a grid axis)
int make_geom(size_t P, size_t H, size_t W, size_t fh, size_t fw, size_t pad, size_t stride, ConvGeom* g);
int team_size();                       // threads of the host team
double* last_timings();                // the 8 slots of vpin_enc_conv_last_timings, per thread

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

// what every encrypted layer returns (vpin_enc_conv2d, vpin_enc_conv2d_mc[_bias], vpin_enc_fc[_signed], vpin_enc_avgpool2d)
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
