// enc_convmc.cpp -- the trained convolution layer and its random-linear-combination check, host side: one signed filter per
// (output channel, input channel) with an optional connection table, the channel mixing inside the check.  Input validation, the
// PRF scalars per (group, output channel), the descriptors of the sums (per pair the B'[c][k] of its connected channels in chain
// order, then its left side), the VPIN_ESHAPE rules, the equality test and the two operation lists.  The convolution, the sums,
// the negation S = -B' for a negative weight and the chain T_m = |w_m| * S_m with its prefixes (mul_chain) run on the device
// (enc_convmc.hip, enc_conv.hip, enc_fc.hip).  Generalises the type-1 path of the reference's myConv2d with rLCL / rLCR
// (src/LeNet/Server.py), which has one non-negative filter and sums the channels outside the check; enc_conv.cpp restates that one.
// vpin_enc_conv2d_mc_bias adds one encrypted bias point per output plane on the device (e2_bias_add_kernel) and records the additions.
#include <omp.h>

#include <algorithm>
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

namespace {

// what both entry points validate and derive: the geometry over the groups * C input planes, the table with NULL spelt out, per
// output channel its connected channels and the top set bit of its largest |w|
struct McPlan {
  ConvGeom g;
  std::vector<uint8_t> connect;            // n_out * C, 0 / 1
  std::vector<std::vector<uint32_t>> chan;  // per o, ascending
  std::vector<int32_t> top_bit;            // per o; -1: all its weights are zero
  size_t pairs = 0, k_max = 0;             // connected (o, c) pairs; the longest chain, in terms
};

uint32_t magnitude(int32_t w) { return w < 0 ? 0u - (uint32_t)w : (uint32_t)w; }

int make_plan(const char* who, size_t groups, size_t C, size_t n_out, size_t H, size_t W, const int32_t* w, const uint8_t* connect, size_t fh,
              size_t fw, size_t pad, size_t stride, McPlan* p) {
  const std::string name(who);
  if (!groups || !C || !n_out) return fail(VPIN_EINVAL, (name + ": groups, C or n_out is zero").c_str());
  if (groups > 65535 || n_out > 65535 || C > 65535 || groups * C > 65535)
    return fail(VPIN_EINVAL, (name + ": a dimension is out of range").c_str());
  const int rc = make_geom(groups * C, H, W, fh, fw, pad, stride, &p->g);
  if (rc) return rc;
  const size_t taps = p->g.taps(), per_plane = p->g.oh * p->g.ow;
  if (groups * n_out * per_plane >= ((size_t)1 << 31) || C * taps >= ((size_t)1 << 24))
    return fail(VPIN_EINVAL, (name + ": a dimension is out of range").c_str());
  p->connect.assign(n_out * C, 1);
  p->chan.assign(n_out, {});
  p->top_bit.assign(n_out, -1);
  for (size_t o = 0; o < n_out; o++) {
    uint32_t all = 0;
    for (size_t c = 0; c < C; c++) {
      if (connect && !connect[o * C + c]) { p->connect[o * C + c] = 0; continue; }
      p->chan[o].push_back((uint32_t)c);
      for (size_t k = 0; k < taps; k++) all |= magnitude(w[(o * C + c) * taps + k]);
    }
    if (p->chan[o].empty()) return fail(VPIN_EINVAL, (name + ": a row of connect selects no channel").c_str());
    while (all) { p->top_bit[o]++; all >>= 1; }
    p->pairs += p->chan[o].size();
    p->k_max = std::max(p->k_max, p->chan[o].size() * taps);
  }
  return VPIN_OK;
}

// vpin_enc_conv2d_mc (no bias: bx = by = binf = NULL) and vpin_enc_conv2d_mc_bias.  With a bias the convolution's result is C,
// the output is C + bias, every pair's additions begin with its oh * ow pairs (C[t], bias), and the check still runs over C
int mc_layer(const char* who, bool with_bias, vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C,
             size_t n_out, size_t H, size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw, size_t pad, size_t stride,
             const uint8_t* bx, const uint8_t* by, const uint8_t* binf, const uint8_t* keys32, int prf_bytes, vpin_conv_trace** out) {
  const std::string name(who);
  auto failed = [&](int code, const char* why) { return fail(code, (name + ": " + why).c_str()); };
  clear_refusals();
  if (out) *out = nullptr;
  if (!c || !px || !py || !pinf || !weights || !keys32 || !out || (with_bias && (!bx || !by || !binf))) return failed(VPIN_EINVAL, "null argument");
  if (prf_bytes < 1 || prf_bytes > 16) return failed(VPIN_EINVAL, "prf_bytes must be in 1 .. 16");
  McPlan p;
  int rc = make_plan(who, groups, C, n_out, H, W, weights, connect, fh, fw, pad, stride, &p);
  if (rc) return rc;
  const ConvGeom& g = p.g;
  const size_t taps = g.taps(), per_plane = g.oh * g.ow, n_pairs = groups * n_out, n_o = n_pairs * per_plane, K = p.k_max;
  const size_t n_chain = n_pairs * K, n_sums = n_chain + n_pairs;  // the chains, padded to K terms each, then the left sides
  if (n_sums * ((per_plane + 255) / 256) >= ((size_t)1 << 31)) return failed(VPIN_EINVAL, "a dimension is out of range");
  double* tm = reset_timings();
  Lap total, lap;
  std::unique_ptr<vpin_conv_trace> t(new (std::nothrow) vpin_conv_trace());
  if (!t) return VPIN_ENOMEM;
  t->P = n_pairs; t->oh = g.oh; t->ow = g.ow;
  t->n_mult = groups * taps * p.pairs;
  t->n_add = t->n_mult - n_pairs + (with_bias ? n_o : 0);

  // validate: upload, range and curve checks on the device
  EncConvDev d(c);
  E2Points tail(c), b(c);
  if ((rc = d.in.load(c, px, py, pinf, g.pixels(), who, "pixel"))) return rc;
  if (with_bias && (rc = b.load(c, bx, by, binf, n_pairs, who, "bias point"))) return rc;
  tm[0] = lap();

  // the convolution
  t->out_x.resize(n_o * 32); t->out_y.resize(n_o * 32); t->out_inf.resize(n_o);
  if ((rc = d.conv_mc(g, groups, C, n_out, weights, p.connect.data(), p.top_bit.data(), t->out_x.data(), t->out_y.data(), t->out_inf.data())))
    return rc;
  std::vector<uint8_t> cx, cy;  // C, the first operands of the bias additions; the trace's output becomes C + bias
  bool refused = false;  // a scan notes every group that breaks its rule; the code and the text are the first hit's
  if (with_bias) {
    for (size_t i = 0; i < n_o; i++)
      if (t->out_inf[i]) { note_refusal(i / (n_out * per_plane)); refused = true; }
    if (refused) return failed(VPIN_ESHAPE, "an addition accumulator C[t] is the identity (the witness format has no flag for it)");
    cx = t->out_x; cy = t->out_y;
    if ((rc = d.add_bias(b, groups, n_out, t->out_x.data(), t->out_y.data(), t->out_inf.data()))) return rc;
  }
  tm[1] = lap();

  // the PRF scalars: one key per (g, o), the index restarts at 0 for every pair
  const std::vector<uint8_t> r = prf_rows(keys32, n_pairs, per_plane, prf_bytes);
  tm[2] = lap();

  // the sums: per pair q = (g, o) its terms m = (c, k) over the connected c ascending, padded to K; then the left sides.  The
  // chain's scalars |w_m| go with them, and the flags of the sums that are negated
  std::vector<int32_t> desc(4 * n_sums, 0);
  std::vector<uint8_t> neg(n_sums, 0), s(n_chain * 16, 0);
  for (size_t q = 0; q < n_pairs; q++) {
    const size_t grp = q / n_out, o = q % n_out, len = p.chan[o].size() * taps;
    for (size_t m = 0; m < K; m++) {
      int32_t* ds = &desc[4 * (q * K + m)];
      ds[0] = -2; ds[2] = (int32_t)q;
      if (m >= len) continue;
      const size_t ch = p.chan[o][m / taps], k = m % taps;
      const int32_t w = weights[(o * C + ch) * taps + k];
      const uint32_t mag = magnitude(w);
      ds[0] = (int32_t)(grp * C + ch); ds[1] = (int32_t)k;
      neg[q * K + m] = w < 0;
      memcpy(&s[16 * (q * K + m)], &mag, 4);  // little-endian u128
    }
    int32_t* dl = &desc[4 * (n_chain + q)];
    dl[0] = -1; dl[2] = (int32_t)q;
  }
  std::vector<uint8_t> sx(n_sums * 32), sy(n_sums * 32), sinf(n_sums);
  if ((rc = d.rlc_mc(n_pairs, desc.data(), neg.data(), n_sums, r.data(), &tail, sx.data(), sy.data(), sinf.data(), 8 * prf_bytes))) return rc;
  tm[3] = lap();

  // the tail: T_m = |w_m| * S_m and the prefixes of every chain on the device, then the equation and the two lists
  for (size_t q = 0; q < n_pairs; q++)
    for (size_t m = 0; m < p.chan[q % n_out].size() * taps; m++)
      if (sinf[q * K + m]) { note_refusal(q / n_out); refused = true; }
  if (refused) return failed(VPIN_ESHAPE, "a multiplication operand B'[c][k] is the identity (the witness format has no flag for it)");
  std::vector<uint8_t> tx(n_chain * 32), ty(n_chain * 32), tinf(n_chain), ax(n_chain * 32), ay(n_chain * 32), ainf(n_chain);
  if ((rc = vpin::mul_chain(c, tail, s.data(), n_pairs, K, tx.data(), ty.data(), tinf.data(), ax.data(), ay.data(), ainf.data()))) return rc;
  t->resize_lists();
  t->left_x.resize(n_pairs * 32); t->left_y.resize(n_pairs * 32); t->left_inf.resize(n_pairs);
  const PointBytes sum{sx.data(), sy.data(), sinf.data()}, prod{tx.data(), ty.data(), tinf.data()}, prefix{ax.data(), ay.data(), ainf.data()};
  bool equal = true;
  size_t mi = 0, ai = 0;
  for (size_t q = 0; q < n_pairs; q++) {
    const size_t len = p.chan[q % n_out].size() * taps;  // the chain without its padding
    for (size_t tt = 0; with_bias && tt < per_plane; tt++, ai++) {
      const size_t i = q * per_plane + tt;
      memcpy(&t->a_px[32 * ai], &cx[32 * i], 32); memcpy(&t->a_py[32 * ai], &cy[32 * i], 32);
      if (binf[q]) { t->a_rz[ai] = 1; continue; }  // rx, ry stay zero
      memcpy(&t->a_rx[32 * ai], bx + 32 * q, 32); memcpy(&t->a_ry[32 * ai], by + 32 * q, 32);
    }
    memcpy(&t->m_w[16 * mi], &s[16 * q * K], 16 * len);
    memcpy(&t->m_px[32 * mi], &sx[32 * q * K], 32 * len); memcpy(&t->m_py[32 * mi], &sy[32 * q * K], 32 * len);
    mi += len;
    const PointBytes left = sum.at(n_chain + q);
    memcpy(&t->left_x[32 * q], left.x, 32); memcpy(&t->left_y[32 * q], left.y, 32);
    t->left_inf[q] = *left.inf;
    bool closes = false;
    const size_t chain_end = ai + len - 1;
    if (emit_chain(who, t.get(), &ai, prod.at(q * K), prefix.at(q * K), len, left, &closes)) {  // VPIN_ESHAPE, one text for every pair
      note_refusal(q / n_out);
      refused = true;
      ai = chain_end;
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

int vpin_e2_conv2d_mc(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C, size_t n_out, size_t H,
                      size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw, size_t pad, size_t stride, uint8_t* out_x,
                      uint8_t* out_y, uint8_t* out_inf) {
  if (!c || !px || !py || !pinf || !weights || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_conv2d_mc: null argument");
  McPlan p;
  int rc = make_plan("vpin_e2_conv2d_mc", groups, C, n_out, H, W, weights, connect, fh, fw, pad, stride, &p);
  if (rc) return rc;
  EncConvDev d(c);
  if ((rc = d.in.load(c, px, py, pinf, p.g.pixels(), "vpin_e2_conv2d_mc", "pixel"))) return rc;
  return d.conv_mc(p.g, groups, C, n_out, weights, p.connect.data(), p.top_bit.data(), out_x, out_y, out_inf);
}

int vpin_enc_conv2d_mc(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C, size_t n_out, size_t H,
                       size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw, size_t pad, size_t stride,
                       const uint8_t* keys32, int prf_bytes, vpin_conv_trace** out) {
  return mc_layer("vpin_enc_conv2d_mc", false, c, px, py, pinf, groups, C, n_out, H, W, weights, connect, fh, fw, pad, stride, nullptr, nullptr,
                  nullptr, keys32, prf_bytes, out);
}

int vpin_enc_conv2d_mc_bias(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t C, size_t n_out,
                            size_t H, size_t W, const int32_t* weights, const uint8_t* connect, size_t fh, size_t fw, size_t pad, size_t stride,
                            const uint8_t* bx, const uint8_t* by, const uint8_t* binf, const uint8_t* keys32, int prf_bytes,
                            vpin_conv_trace** out) {
  return mc_layer("vpin_enc_conv2d_mc_bias", true, c, px, py, pinf, groups, C, n_out, H, W, weights, connect, fh, fw, pad, stride, bx, by, binf,
                  keys32, prf_bytes, out);
}

}  // extern "C"
