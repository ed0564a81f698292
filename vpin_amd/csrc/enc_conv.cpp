// enc_conv.cpp -- the encrypted convolution layer of vPIN's inference server and its random-linear-combination check,
// host side: input validation, the PRF scalars (HMAC-SHA256, one OpenMP team), the f^2 multiplications and f^2 - 1
// additions that the check reduces one convolution to, the equality test, and the two operation lists in the order the
// point-mult / point-add gadgets prove them.  The convolution itself and the f^2 + 1 sums of the check run on the device
// (enc_conv.hip).  Restates the type-1 path of the reference's convolution service (src/convolution/Server.py,
// src/LeNet/Server.py: myConv2d, rLCL, rLCR).  The E2 host code, the PRF and the trace accessors here also serve the fully
// connected and pooling layers (enc_fc.cpp) and the trained convolution (enc_convmc.cpp) through namespace vpin::enc of
// enc_conv.h, as do the frame of a layer driver (reset_timings, prf_rows) and the tail that writes one chain (emit_chain).
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"
#include "host/field.h"
#include "host/gadget_ops.h"

using vpin::ConvGeom;
using vpin::EncConvDev;
using vpin::set_last_error_text;
using vpin_host::Fq;
typedef unsigned __int128 u128;

namespace vpin {
namespace enc {

// ---- E2 on the host: affine in and out, Jacobian inside, complete by case -----------------------------------------

static Fq fq_from_le32(const uint8_t* b) {
  Fq t;
  memcpy(t.l, b, 32);
  return t * Fq::r2();
}

static const Fq& curve_a() {
  static const Fq a = fq_from_le32(vpin_gadgets::kAPdBytes);
  return a;
}

static Jac jac_identity() { return Jac{Fq::zero(), Fq::one(), Fq::zero()}; }

static Jac jac_dbl(const Jac& p) {
  if (p.inf()) return p;
  const Fq XX = p.X * p.X, YY = p.Y * p.Y, YYYY = YY * YY, ZZ = p.Z * p.Z;
  Fq S = p.X * YY; S = S + S; S = S + S;
  const Fq M = XX + XX + XX + curve_a() * ZZ * ZZ;
  Jac r;
  r.X = M * M - S - S;
  Fq t = YYYY + YYYY; t = t + t; t = t + t;
  r.Y = M * (S - r.X) - t;
  r.Z = p.Y * p.Z; r.Z = r.Z + r.Z;
  return r;
}

static Jac jac_add_mixed(const Jac& p, const Aff& q) {
  if (q.inf) return p;
  if (p.inf()) return Jac{q.x, q.y, Fq::one()};
  const Fq ZZ = p.Z * p.Z, U2 = q.x * ZZ, S2 = q.y * ZZ * p.Z, H = U2 - p.X, R = S2 - p.Y;
  if (H.is_zero()) return R.is_zero() ? jac_dbl(p) : jac_identity();
  const Fq HH = H * H, HHH = HH * H, V = p.X * HH;
  Jac r;
  r.X = R * R - HHH - V - V;
  r.Y = R * (V - r.X) - p.Y * HHH;
  r.Z = p.Z * H;
  return r;
}

Aff to_affine(const Jac& p) {
  Aff r;
  if (p.inf()) return r;
  const Fq zi = p.Z.invert(), zi2 = zi * zi;
  r.x = p.X * zi2;
  r.y = p.Y * zi2 * zi;
  r.inf = false;
  return r;
}

Aff aff_add(const Aff& p, const Aff& q) {
  if (p.inf) return q;
  return to_affine(jac_add_mixed(Jac{p.x, p.y, Fq::one()}, q));
}

static Aff aff_mul(u128 w, const Aff& p) {
  Jac acc = jac_identity();
  if (p.inf) return Aff();
  for (int b = 127; b >= 0; b--) {
    acc = jac_dbl(acc);
    if ((w >> b) & 1) acc = jac_add_mixed(acc, p);
  }
  return to_affine(acc);
}

Aff aff_from_bytes(const uint8_t* x, const uint8_t* y, uint8_t inf) {
  Aff r;
  if (inf) return r;
  r.x = fq_from_le32(x);
  r.y = fq_from_le32(y);
  r.inf = false;
  return r;
}

// canonical little-endian coordinates; the identity is written as zeros
void put_point(const Aff& p, uint8_t* x, uint8_t* y) {
  if (p.inf) { memset(x, 0, 32); memset(y, 0, 32); return; }
  p.x.to_bytes(x);
  p.y.to_bytes(y);
}

// ---- HMAC-SHA256 (RFC 2104) over the library's SHA-256, key of 32 bytes --------------------------------------------

static void hmac_sha256_key32(const uint8_t key[32], const uint8_t* msg, size_t n, uint8_t out[32]) {
  uint8_t inner[64 + 32], outer[64 + 32];  // n <= 32: a decimal index
  memset(inner, 0x36, 64);
  memset(outer, 0x5c, 64);
  for (int i = 0; i < 32; i++) { inner[i] ^= key[i]; outer[i] ^= key[i]; }
  memcpy(inner + 64, msg, n);
  vpin_sha256(inner, 64 + n, outer + 64);
  vpin_sha256(outer, 96, out);
}

// r_t = int.from_bytes(HMAC(key, ascii_decimal(t))[:prf_bytes], "big") as a little-endian u128
static void prf_scalar(const uint8_t key[32], size_t t, int prf_bytes, uint8_t out_le16[16]) {
  char msg[32];
  const int n = snprintf(msg, sizeof(msg), "%zu", t);
  uint8_t mac[32];
  hmac_sha256_key32(key, (const uint8_t*)msg, (size_t)n, mac);
  memset(out_le16, 0, 16);
  for (int i = 0; i < prf_bytes; i++) out_le16[i] = mac[prf_bytes - 1 - i];
}

int fail(int code, const char* why) {
  set_last_error_text(why);
  return code;
}

int make_geom(size_t P, size_t H, size_t W, size_t fh, size_t fw, size_t pad, size_t stride, ConvGeom* g) {
  if (!P || !H || !W || !fh || !fw || !stride) return fail(VPIN_EINVAL, "enc_conv: a dimension is zero");
  if (P > 65535 || H > kMaxDim || W > kMaxDim || fh > kMaxDim || fw > kMaxDim || pad > kMaxDim || stride > kMaxDim || fh * fw > 65534)
    return fail(VPIN_EINVAL, "enc_conv: a dimension is out of range");
  if (H + 2 * pad < fh || W + 2 * pad < fw) return fail(VPIN_EINVAL, "enc_conv: the window does not fit the padded plane");
  g->P = P; g->H = H; g->W = W; g->fh = fh; g->fw = fw; g->pad = pad; g->stride = stride;
  g->oh = (H + 2 * pad - fh) / stride + 1;
  g->ow = (W + 2 * pad - fw) / stride + 1;
  if (g->oh * g->ow >= ((size_t)1 << 31) || H * W >= ((size_t)1 << 31))
    return fail(VPIN_EINVAL, "enc_conv: a plane has 2^31 pixels or more");
  return VPIN_OK;
}

Jac jac_from_bytes(const uint8_t* p) {
  Jac r;
  memcpy(r.X.l, p, 32); memcpy(r.Y.l, p + 32, 32); memcpy(r.Z.l, p + 64, 32);
  return r;
}

static thread_local double g_timings[8] = {0, 0, 0, 0, 0, 0, 0, 0};

double* reset_timings() {
  for (double& v : g_timings) v = 0.0;
  return g_timings;
}

std::vector<uint8_t> prf_rows(const uint8_t* keys32, size_t rows, size_t per_row, int prf_bytes) {
  std::vector<uint8_t> r(rows * per_row * 16);
#pragma omp parallel for schedule(static) num_threads(team_size())
  for (long i = 0; i < (long)(rows * per_row); i++)
    prf_scalar(keys32 + 32 * ((size_t)i / per_row), (size_t)i % per_row, prf_bytes, &r[16 * (size_t)i]);
  return r;
}

int emit_chain(const char* who, vpin_conv_trace* t, size_t* ai, PointBytes prod, PointBytes prefix, size_t len, PointBytes left, bool* closes) {
  for (size_t k = 1; k < len; k++, ++*ai) {
    if (prefix.inf[k - 1])
      return fail(VPIN_ESHAPE, (std::string(who) + ": an addition accumulator is the identity (the witness format has no flag for it)").c_str());
    memcpy(&t->a_px[32 * *ai], prefix.x + 32 * (k - 1), 32); memcpy(&t->a_py[32 * *ai], prefix.y + 32 * (k - 1), 32);
    memcpy(&t->a_rx[32 * *ai], prod.x + 32 * k, 32); memcpy(&t->a_ry[32 * *ai], prod.y + 32 * k, 32);
    t->a_rz[*ai] = prod.inf[k];
  }
  const PointBytes last = prefix.at(len - 1);  // both sides are canonical, the identity zeros
  *closes = *last.inf == *left.inf && !memcmp(last.x, left.x, 32) && !memcmp(last.y, left.y, 32);
  return VPIN_OK;
}

static thread_local std::vector<uint32_t> g_refusals;  // ascending: every scan walks its units in order

void clear_refusals() { g_refusals.clear(); }

void note_refusal(size_t unit) {
  if (g_refusals.empty() || g_refusals.back() != (uint32_t)unit) g_refusals.push_back((uint32_t)unit);
}

int team_size() { return (int)std::max(1.0, std::min(16.0, vpin::host_cpu_quota())); }

}  // namespace enc
}  // namespace vpin

using namespace vpin::enc;

extern "C" {

int vpin_e2_msm(vpin_ctx* c, const uint8_t* scalars_le16, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t n,
                uint8_t out_x[32], uint8_t out_y[32], uint8_t* out_inf) {
  if (!c || !scalars_le16 || !px || !py || !pinf || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_msm: null argument");
  if (n == 0 || n >= ((size_t)1 << 31)) return fail(VPIN_EINVAL, "vpin_e2_msm: n must be in 1 .. 2^31 - 1");
  EncConvDev d(c);
  int rc = d.in.load(c, px, py, pinf, n);
  if (rc) return rc;
  uint8_t sum[96];
  if ((rc = d.msm(scalars_le16, n, sum))) return rc;
  const Aff r = to_affine(jac_from_bytes(sum));
  put_point(r, out_x, out_y);
  *out_inf = r.inf ? 1 : 0;
  return VPIN_OK;
}

int vpin_e2_conv2d(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t H, size_t W,
                   const uint8_t* filter_le16, size_t fh, size_t fw, size_t pad, size_t stride, uint8_t* out_x, uint8_t* out_y,
                   uint8_t* out_inf) {
  if (!c || !px || !py || !pinf || !filter_le16 || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_conv2d: null argument");
  ConvGeom g;
  int rc = make_geom(1, H, W, fh, fw, pad, stride, &g);
  if (rc) return rc;
  EncConvDev d(c);
  if ((rc = d.in.load(c, px, py, pinf, g.pixels()))) return rc;
  return d.conv(g, filter_le16, out_x, out_y, out_inf);
}

int vpin_enc_conv2d(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t H, size_t W,
                    const uint8_t* filter_le16, size_t fh, size_t fw, size_t pad, size_t stride, const uint8_t* keys32, int prf_bytes,
                    vpin_conv_trace** out) {
  clear_refusals();
  if (out) *out = nullptr;
  if (!c || !px || !py || !pinf || !filter_le16 || !keys32 || !out) return fail(VPIN_EINVAL, "vpin_enc_conv2d: null argument");
  if (prf_bytes < 1 || prf_bytes > 16) return fail(VPIN_EINVAL, "vpin_enc_conv2d: prf_bytes must be in 1 .. 16");
  ConvGeom g;
  int rc = make_geom(P, H, W, fh, fw, pad, stride, &g);
  if (rc) return rc;
  double* tm = reset_timings();
  Lap total, lap;
  std::unique_ptr<vpin_conv_trace> t(new (std::nothrow) vpin_conv_trace());
  if (!t) return VPIN_ENOMEM;
  const char* no_flag = "vpin_enc_conv2d: a multiplication operand B'[k] is the identity (the witness format has no flag for it)";
  const size_t taps = g.taps(), nsum = taps + 1, per_plane = g.oh * g.ow, n_out = g.outputs();
  t->P = P; t->oh = g.oh; t->ow = g.ow;

  // validate: upload, range and curve checks on the device
  EncConvDev d(c);
  if ((rc = d.in.load(c, px, py, pinf, g.pixels()))) return rc;
  tm[0] = lap();

  // the convolution
  t->out_x.resize(n_out * 32); t->out_y.resize(n_out * 32); t->out_inf.resize(n_out);
  if ((rc = d.conv(g, filter_le16, t->out_x.data(), t->out_y.data(), t->out_inf.data()))) return rc;
  tm[1] = lap();

  // the PRF scalars: the index restarts at 0 for every plane
  const std::vector<uint8_t> r = prf_rows(keys32, P, per_plane, prf_bytes);
  tm[2] = lap();

  // the f^2 + 1 sums of every plane
  std::vector<uint8_t> sums(P * nsum * 96);
  if ((rc = d.rlc(r.data(), sums.data(), 8 * prf_bytes))) return rc;
  tm[3] = lap();

  // host tail: T_k = w[k] * B'[k] on the team, the prefixes of every plane's chain, the two lists, the equation
  std::vector<Aff> B(P * nsum), T(P * taps);
  std::vector<u128> w(taps);
  for (size_t k = 0; k < taps; k++) memcpy(&w[k], filter_le16 + 16 * k, 16);
#pragma omp parallel for schedule(dynamic, 1) num_threads(team_size())
  for (long i = 0; i < (long)(P * nsum); i++) B[(size_t)i] = to_affine(jac_from_bytes(&sums[96 * (size_t)i]));
  bool refused = false;
  for (size_t p = 0; p < P; p++)
    for (size_t k = 0; k < taps; k++)
      if (B[p * nsum + k].inf) { note_refusal(p); refused = true; break; }
  if (refused) return fail(VPIN_ESHAPE, no_flag);
#pragma omp parallel for schedule(dynamic, 1) num_threads(team_size())
  for (long i = 0; i < (long)(P * taps); i++) {
    const size_t p = (size_t)i / taps, k = (size_t)i % taps;
    T[(size_t)i] = aff_mul(w[k], B[p * nsum + k]);
  }
  t->n_mult = P * taps;
  t->n_add = P * (taps - 1);
  t->resize_lists();
  t->left_x.resize(P * 32); t->left_y.resize(P * 32); t->left_inf.resize(P);
  std::vector<uint8_t> tx(taps * 32), ty(taps * 32), tinf(taps), ax(taps * 32), ay(taps * 32), ainf(taps);  // one plane's chain
  const PointBytes prod{tx.data(), ty.data(), tinf.data()}, prefix{ax.data(), ay.data(), ainf.data()};
  const PointBytes left{t->left_x.data(), t->left_y.data(), t->left_inf.data()};
  bool equal = true;
  size_t ai = 0;
  for (size_t p = 0; p < P; p++) {
    Aff acc;
    for (size_t k = 0; k < taps; k++) {
      const size_t m = p * taps + k;
      memcpy(&t->m_w[16 * m], filter_le16 + 16 * k, 16);
      put_point(B[p * nsum + k], &t->m_px[32 * m], &t->m_py[32 * m]);
      acc = aff_add(acc, T[m]);  // complete: an identity prefix is emit_chain's to reject
      put_point(T[m], &tx[32 * k], &ty[32 * k]);
      tinf[k] = T[m].inf ? 1 : 0;
      put_point(acc, &ax[32 * k], &ay[32 * k]);
      ainf[k] = acc.inf ? 1 : 0;
    }
    const Aff& l = B[p * nsum + taps];
    put_point(l, &t->left_x[32 * p], &t->left_y[32 * p]);
    t->left_inf[p] = l.inf ? 1 : 0;
    bool closes = false;
    if (emit_chain("vpin_enc_conv2d", t.get(), &ai, prod, prefix, taps, left.at(p), &closes)) {  // VPIN_ESHAPE, the same text for every plane
      note_refusal(p);
      refused = true;
      ai = (p + 1) * (taps - 1);
    }
    if (!closes) equal = false;
  }
  if (refused) return VPIN_ESHAPE;
  tm[4] = lap();
  tm[5] = total();
  if (!equal) return fail(VPIN_EVERIFY, "vpin_enc_conv2d: the two sides of the random linear combination differ");
  *out = t.release();
  return VPIN_OK;
}

void vpin_conv_trace_free(vpin_conv_trace* t) { delete t; }

int vpin_conv_trace_dims(const vpin_conv_trace* t, size_t out[5]) {
  if (!t || !out) return VPIN_EINVAL;
  out[0] = t->P; out[1] = t->oh; out[2] = t->ow; out[3] = t->n_mult; out[4] = t->n_add;
  return VPIN_OK;
}

int vpin_conv_trace_output(const vpin_conv_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf) {
  if (!t || !x || !y || !inf) return VPIN_EINVAL;
  *x = t->out_x.data(); *y = t->out_y.data(); *inf = t->out_inf.data();
  return VPIN_OK;
}

int vpin_conv_trace_mults(const vpin_conv_trace* t, const uint8_t** weights_le16, const uint8_t** px, const uint8_t** py) {
  if (!t || !weights_le16 || !px || !py) return VPIN_EINVAL;
  *weights_le16 = t->m_w.data(); *px = t->m_px.data(); *py = t->m_py.data();
  return VPIN_OK;
}

int vpin_conv_trace_adds(const vpin_conv_trace* t, const uint8_t** px, const uint8_t** py, const uint8_t** rx, const uint8_t** ry,
                         const uint8_t** rz) {
  if (!t || !px || !py || !rx || !ry || !rz) return VPIN_EINVAL;
  *px = t->a_px.data(); *py = t->a_py.data(); *rx = t->a_rx.data(); *ry = t->a_ry.data(); *rz = t->a_rz.data();
  return VPIN_OK;
}

int vpin_conv_trace_left(const vpin_conv_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf) {
  if (!t || !x || !y || !inf) return VPIN_EINVAL;
  *x = t->left_x.data(); *y = t->left_y.data(); *inf = t->left_inf.data();
  return VPIN_OK;
}

int vpin_conv_trace_instances(vpin_ctx* c, const vpin_conv_trace* t, vpin_dev_instance** mult_out, vpin_dev_instance** add_out) {
  if (mult_out) *mult_out = nullptr;
  if (add_out) *add_out = nullptr;
  if (!c || !t || !mult_out || !add_out) return VPIN_EINVAL;
  int rc = VPIN_OK;
  if (t->n_mult && (rc = vpin_gadget_point_mult_dev(c, t->m_w.data(), t->m_px.data(), t->m_py.data(), t->n_mult, mult_out))) return rc;  // pooling multiplies nothing
  if (t->n_add == 0) return VPIN_OK;  // a 1 x 1 filter or window: nothing to add
  rc = vpin_gadget_point_add_dev(c, t->a_px.data(), t->a_py.data(), t->a_rx.data(), t->a_ry.data(), t->a_rz.data(), t->n_add, add_out);
  if (rc && *mult_out) { vpin_dev_instance_free(c, *mult_out); *mult_out = nullptr; }
  return rc;
}

int vpin_enc_last_refusals(uint32_t* units, size_t cap, size_t* n) {
  if (!n || (cap && !units)) return fail(VPIN_EINVAL, "vpin_enc_last_refusals: null argument");
  *n = g_refusals.size();
  for (size_t i = 0; i < g_refusals.size() && i < cap; i++) units[i] = g_refusals[i];
  return VPIN_OK;
}

void vpin_enc_conv_last_timings(double out[8]) {
  for (int i = 0; i < 8; i++) out[i] = g_timings[i];
}

}  // extern "C"
