// enc_fc.cpp -- the encrypted fully connected layer with its random-linear-combination check, and the encrypted average
// pooling, host side: input validation, the PRF scalars, the folded weights s_k = sum_j r_j * W[k][j] (exact, in 128 bits),
// out = C + bias, the checks over the chains of additions, the equality test and the operation lists in the order the
// point-mult / point-add gadgets prove them.  The matrix-vector product, the left sum, the K multiplications s_k * X[k] with
// the chain of their sums (mul_chain, also exposed as vpin_e2_mul_chain), the pooling's accumulators and its scaled outputs run
// on the device (enc_fc.hip, enc_conv.hip).  Restates FCLayer (flag 1) with the
// type-1 branch of rLCL / rLCR, and myAvgPool2d (type1 = 1, flag = 1), of the reference's src/LeNet/Server.py.  vpin_enc_fc_signed is
// the same layer over int32 weights: s_k is a signed integer, and a negative one multiplies the negated point.
#include <omp.h>

#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"

using namespace vpin::enc;
using vpin::ConvGeom;
using vpin::E2Points;
using vpin::EncConvDev;
typedef unsigned __int128 u128;

namespace {

// acc += r * w; false when the sum leaves 128 bits
bool mul_add_u128(u128& acc, u128 r, uint32_t w) {
  const u128 lo = (u128)(uint64_t)r * w, hi = (u128)(uint64_t)(r >> 64) * w;
  if (hi >> 64) return false;
  const u128 prod = lo + (hi << 64);
  if (prod < lo) return false;
  acc += prod;
  return acc >= prod;
}

// vpin_enc_fc (weights: u32) and vpin_enc_fc_signed (is_signed, weights: int32) are one layer: without a negative weight every
// neg_k below is zero, no point is negated, and the two instances of e2_matvec_kernel compute the same points
int fc_layer(const char* who, vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t K, const void* weights,
             bool is_signed, size_t N, const uint8_t* bx, const uint8_t* by, const uint8_t* binf, const uint8_t* keys32, int prf_bytes,
             vpin_conv_trace** out) {
  const std::string name(who);
  auto failed = [&](int code, const char* why) { return fail(code, (name + ": " + why).c_str()); };
  clear_refusals();
  if (out) *out = nullptr;
  if (!c || !px || !py || !pinf || !weights || !bx || !by || !binf || !keys32 || !out) return failed(VPIN_EINVAL, "null argument");
  if (prf_bytes < 1 || prf_bytes > 16) return failed(VPIN_EINVAL, "prf_bytes must be in 1 .. 16");
  if (!P || !K || !N) return failed(VPIN_EINVAL, "a dimension is zero");
  if (P > 65535 || N > 65535 || K > kMaxDim) return failed(VPIN_EINVAL, "a dimension is out of range");
  double* tm = reset_timings();
  Lap total, lap;
  std::unique_ptr<vpin_conv_trace> t(new (std::nothrow) vpin_conv_trace());
  if (!t) return VPIN_ENOMEM;
  const size_t n_in = P * K, n_out = P * N, adds_per_row = N + K - 1;
  t->P = P; t->oh = 1; t->ow = N; t->n_mult = n_in; t->n_add = P * adds_per_row;

  // validate: upload, range and curve checks on the device, for the inputs and the bias
  EncConvDev d(c);
  E2Points b(c), flipped(c);
  int rc = d.in.load(c, px, py, pinf, n_in, who, "input point");
  if (!rc) rc = b.load(c, bx, by, binf, n_out, who, "bias point");
  if (rc) return rc;
  tm[0] = lap();

  // C = X * W on the device, out = C + bias here; the first N additions of every row
  t->resize_lists();
  t->out_x.resize(n_out * 32); t->out_y.resize(n_out * 32); t->out_inf.resize(n_out);
  t->left_x.resize(P * 32); t->left_y.resize(P * 32); t->left_inf.resize(P);
  std::vector<uint8_t> cx(n_out * 32), cy(n_out * 32), cinf(n_out);
  if ((rc = d.matvec(P, K, N, weights, is_signed, cx.data(), cy.data(), cinf.data()))) return rc;
  bool refused = false;  // a scan notes every row that breaks its rule; the code and the text are the first hit's
  for (size_t i = 0; i < n_out; i++)
    if (cinf[i]) { note_refusal(i / N); refused = true; }
  if (refused) return failed(VPIN_ESHAPE, "an addition accumulator C[j] is the identity (the witness format has no flag for it)");
#pragma omp parallel for schedule(static) num_threads(team_size())
  for (long li = 0; li < (long)n_out; li++) {
    const size_t i = (size_t)li, ai = (i / N) * adds_per_row + i % N;
    const Aff bias = aff_from_bytes(bx + 32 * i, by + 32 * i, binf[i]);
    const Aff o = aff_add(aff_from_bytes(&cx[32 * i], &cy[32 * i], 0), bias);
    memcpy(&t->a_px[32 * ai], &cx[32 * i], 32); memcpy(&t->a_py[32 * ai], &cy[32 * i], 32);
    put_point(bias, &t->a_rx[32 * ai], &t->a_ry[32 * ai]);
    t->a_rz[ai] = bias.inf ? 1 : 0;
    put_point(o, &t->out_x[32 * i], &t->out_y[32 * i]);
    t->out_inf[i] = o.inf ? 1 : 0;
  }
  tm[1] = lap();

  // the PRF scalars: the index restarts at 0 for every row
  const std::vector<uint8_t> r = prf_rows(keys32, P, N, prf_bytes);
  tm[2] = lap();

  // left = sum_j r_j * C[j] of every row, over the resident C
  std::vector<uint8_t> sums(P * 96);
  if ((rc = d.rlc(r.data(), sums.data()))) return rc;
  tm[3] = lap();

  // the tail: the folded weights here, T_k = |s_k| * S_k and the prefixes of every row's chain on the device, then the equation.
  // s_k = pos_k - neg_k over the positive and the negative weights; the gadget's weight is a u128, so the sign goes into the
  // point: S_k = X[k] for s_k >= 0 and -X[k] = (x, q - y) for s_k < 0
  std::vector<size_t> minus_s;  // the m = p * K + k with s_k < 0
  for (size_t p = 0; p < P; p++) {
    bool fits = true;
    for (size_t k = 0; k < K && fits; k++) {
      u128 pos = 0, neg = 0;
      for (size_t j = 0; j < N && fits; j++) {
        u128 rj;
        uint32_t w;
        memcpy(&rj, &r[16 * (p * N + j)], 16);
        memcpy(&w, (const uint8_t*)weights + 4 * (k * N + j), 4);
        const bool minus = is_signed && (w >> 31);  // |INT32_MIN| = 2^31 as 0 - w in unsigned arithmetic
        fits = mul_add_u128(minus ? neg : pos, rj, minus ? 0u - w : w);
      }
      const size_t m = p * K + k;
      const u128 s = pos >= neg ? pos - neg : neg - pos;
      memcpy(&t->m_w[16 * m], &s, 16);
      if (pos < neg) minus_s.push_back(m);
    }
    if (!fits) { note_refusal(p); refused = true; }
  }
  if (refused) return failed(VPIN_ESHAPE, "a folded weight sum_j r_j * W[k][j] does not fit 128 bits");
  for (size_t i = 0; i < n_in; i++)
    if (pinf[i]) { note_refusal(i / K); refused = true; }
  if (refused) return failed(VPIN_ESHAPE, "a multiplication operand X[k] is the identity (the witness format has no flag for it)");
  memcpy(t->m_px.data(), px, n_in * 32);
  memcpy(t->m_py.data(), py, n_in * 32);
  for (const size_t m : minus_s) {
    Aff x = aff_from_bytes(px + 32 * m, py + 32 * m, 0);
    x.y = x.y.neg();
    put_point(x, &t->m_px[32 * m], &t->m_py[32 * m]);
  }
  const E2Points* tail = &d.in;
  if (!minus_s.empty()) {  // the chain runs over S: the recorded points, validated again as they are loaded
    if ((rc = flipped.load(c, t->m_px.data(), t->m_py.data(), pinf, n_in, who, "input point"))) return rc;
    tail = &flipped;
  }
  std::vector<uint8_t> tx(n_in * 32), ty(n_in * 32), tinf(n_in), ax(n_in * 32), ay(n_in * 32), ainf(n_in);
  if ((rc = vpin::mul_chain(c, *tail, t->m_w.data(), P, K, tx.data(), ty.data(), tinf.data(), ax.data(), ay.data(), ainf.data()))) return rc;
  const PointBytes prod{tx.data(), ty.data(), tinf.data()}, prefix{ax.data(), ay.data(), ainf.data()};
  const PointBytes left{t->left_x.data(), t->left_y.data(), t->left_inf.data()};
  bool equal = true;
  for (size_t p = 0; p < P; p++) {
    const Aff l = to_affine(jac_from_bytes(&sums[96 * p]));
    put_point(l, &t->left_x[32 * p], &t->left_y[32 * p]);
    t->left_inf[p] = l.inf ? 1 : 0;
    size_t ai = p * adds_per_row + N;  // after the row's bias additions
    bool closes = false;
    if (emit_chain(who, t.get(), &ai, prod.at(p * K), prefix.at(p * K), K, left.at(p), &closes)) {  // VPIN_ESHAPE, one text for every row
      note_refusal(p);
      refused = true;
    }
    if (!closes) equal = false;
  }
  if (refused) return VPIN_ESHAPE;
  tm[4] = lap();
  tm[5] = total();
  if (!equal) return failed(VPIN_EVERIFY, "the two sides of the random linear combination differ");
  *out = t.release();
  return VPIN_OK;
}

}  // namespace

extern "C" {

int vpin_e2_mul_chain(vpin_ctx* c, const uint8_t* scalars_le16, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P,
                      size_t K, uint8_t* t_x, uint8_t* t_y, uint8_t* t_inf, uint8_t* acc_x, uint8_t* acc_y, uint8_t* acc_inf) {
  if (!c || !scalars_le16 || !px || !py || !pinf || !t_x || !t_y || !t_inf || !acc_x || !acc_y || !acc_inf)
    return fail(VPIN_EINVAL, "vpin_e2_mul_chain: null argument");
  if (!P || !K || P >= ((size_t)1 << 31) || K >= ((size_t)1 << 31) || P * K >= ((size_t)1 << 31))
    return fail(VPIN_EINVAL, "vpin_e2_mul_chain: P and K must be at least 1 and P * K at most 2^31 - 1");
  E2Points pts(c);
  const int rc = pts.load(c, px, py, pinf, P * K, "vpin_e2_mul_chain", "point");
  if (rc) return rc;
  return vpin::mul_chain(c, pts, scalars_le16, P, K, t_x, t_y, t_inf, acc_x, acc_y, acc_inf);
}

int vpin_enc_fc(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t K, const uint8_t* weights_le4,
                size_t N, const uint8_t* bx, const uint8_t* by, const uint8_t* binf, const uint8_t* keys32, int prf_bytes,
                vpin_conv_trace** out) {
  return fc_layer("vpin_enc_fc", c, px, py, pinf, P, K, weights_le4, false, N, bx, by, binf, keys32, prf_bytes, out);
}

int vpin_enc_fc_signed(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t K, const int32_t* weights,
                       size_t N, const uint8_t* bx, const uint8_t* by, const uint8_t* binf, const uint8_t* keys32, int prf_bytes,
                       vpin_conv_trace** out) {
  return fc_layer("vpin_enc_fc_signed", c, px, py, pinf, P, K, weights, true, N, bx, by, binf, keys32, prf_bytes, out);
}

int vpin_enc_avgpool2d(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t P, size_t H, size_t W, size_t k,
                       size_t stride, const uint8_t scale_le16[16], vpin_conv_trace** out) {
  clear_refusals();
  if (out) *out = nullptr;
  if (!c || !px || !py || !pinf || !scale_le16 || !out) return fail(VPIN_EINVAL, "vpin_enc_avgpool2d: null argument");
  ConvGeom g;
  int rc = make_geom(P, H, W, k, k, 0, stride, &g);  // zero dimensions, k > H, k > W
  if (rc) return rc;
  double* tm = reset_timings();
  Lap total, lap;
  std::unique_ptr<vpin_conv_trace> t(new (std::nothrow) vpin_conv_trace());
  if (!t) return VPIN_ENOMEM;
  const size_t taps = g.taps(), n_out = g.outputs(), per_plane = g.oh * g.ow;
  t->P = P; t->oh = g.oh; t->ow = g.ow; t->n_add = n_out * (taps - 1);

  EncConvDev d(c);
  if ((rc = d.in.load(c, px, py, pinf, g.pixels(), "vpin_enc_avgpool2d", "pixel"))) return rc;
  tm[0] = lap();

  // the accumulators of the additions, then out = scale * (window sum) as the convolution under a constant filter
  t->resize_lists();
  if (t->n_add) {
    std::vector<uint8_t> bad(n_out);
    if ((rc = d.pool_sums(g, t->a_px.data(), t->a_py.data(), bad.data()))) return rc;
    bool refused = false;
    for (size_t i = 0; i < n_out; i++)
      if (bad[i]) { note_refusal(i / per_plane); refused = true; }
    if (refused) return fail(VPIN_ESHAPE, "vpin_enc_avgpool2d: an addition accumulator is the identity (the witness format has no flag for it)");
  }
  std::vector<uint8_t> filt(taps * 16);
  for (size_t m = 0; m < taps; m++) memcpy(&filt[16 * m], scale_le16, 16);
  t->out_x.resize(n_out * 32); t->out_y.resize(n_out * 32); t->out_inf.resize(n_out);
  if ((rc = d.conv(g, filt.data(), t->out_x.data(), t->out_y.data(), t->out_inf.data()))) return rc;
  tm[1] = lap();

  // host tail: the second operands e_1 .. e_{k*k-1} of every output, from the caller's bytes
#pragma omp parallel for schedule(static) num_threads(team_size())
  for (long lo = 0; lo < (long)n_out; lo++) {
    const size_t o = (size_t)lo, plane = o / per_plane, i = (o % per_plane) / g.ow, j = o % g.ow;
    for (size_t m = 1; m < taps; m++) {
      const size_t src = plane * H * W + (i * stride + m / k) * W + j * stride + m % k, ai = o * (taps - 1) + (m - 1);
      if (pinf[src]) {
        t->a_rz[ai] = 1;  // rx, ry stay zero
      } else {
        memcpy(&t->a_rx[32 * ai], px + 32 * src, 32); memcpy(&t->a_ry[32 * ai], py + 32 * src, 32);
      }
    }
  }
  tm[4] = lap();
  tm[5] = total();
  *out = t.release();
  return VPIN_OK;
}

}  // extern "C"
