// net.cpp -- an encrypted inference as a list of layers behind the C ABI: the server loop of the reference's
// src/cnn_networks/Server.py inferenceCNN (conv2_ciphertext, avgPool_ciphertext, flattening, FC1, FC2) over the layer entry
// points (vpin_enc_conv2d, vpin_enc_avgpool2d, vpin_enc_fc), the interaction with the client as a callback per round, and a
// ready-made client of any number of rounds over vpin_e2_client_round (main of src/cnn_networks/Client.py between two layers).
// The planes go through a layer as all c1 planes and then all c2 planes, the order of callConv2_ciphertext on c1 and then on c2;
// that service appends every layer's operations to the same four global lists, so the trace offers, beside each layer's own
// trace, the lists of all layers concatenated in layer order: the network's ONE label.  Ciphertexts cross every layer boundary
// as host bytes; each layer validates what it is given, the client's answers included.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"

using vpin::enc::fail;

namespace {

struct Pts {
  std::vector<uint8_t> x, y, inf;
  size_t n() const { return inf.size(); }
  void resize(size_t k) { x.resize(32 * k); y.resize(32 * k); inf.resize(k); }
  void assign(const uint8_t* px, const uint8_t* py, const uint8_t* pf, size_t k) {
    x.assign(px, px + 32 * k); y.assign(py, py + 32 * k); inf.assign(pf, pf + k);
  }
  void append(const Pts& o) {
    x.insert(x.end(), o.x.begin(), o.x.end()); y.insert(y.end(), o.y.begin(), o.y.end()); inf.insert(inf.end(), o.inf.begin(), o.inf.end());
  }
};

const char* kind_name(int kind) { return kind == VPIN_NET_CONV ? "conv" : kind == VPIN_NET_POOL ? "pool" : "fc"; }

// per layer what it consumes and leaves; the walk that vpin_net_cfg_counts and vpin_net_infer share
struct LayerPlan {
  size_t C, H, W;        // what comes in
  size_t oC, oH, oW;     // what goes out
  size_t mult, add, keys, bias_r;
  int round;             // index of the round after the layer, or -1
};

constexpr size_t kMaxLayers = 4096, kMaxSide = 4096, kMaxPlanes = 16384;

int plan(const vpin_net_cfg* g, bool weights, std::vector<LayerPlan>* out) {
  if (!g->layers || !g->n_layers) return fail(VPIN_EINVAL, "vpin_net: the configuration has no layers");
  if (!g->C || !g->H || !g->W) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
  if (g->n_layers > kMaxLayers || g->C > kMaxPlanes || g->H > kMaxSide || g->W > kMaxSide) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
  if (g->prf_bytes < 1 || g->prf_bytes > 16) return fail(VPIN_EINVAL, "vpin_net: prf_bytes must be in 1 .. 16");
  size_t C = g->C, H = g->H, W = g->W;
  int rounds = 0;
  out->clear();
  for (size_t i = 0; i < g->n_layers; i++) {
    const vpin_net_layer& l = g->layers[i];
    LayerPlan p{C, H, W, C, H, W, 0, 0, 0, 0, -1};
    const char* fit = "vpin_net: a window does not fit its plane";
    if (l.kind == VPIN_NET_CONV) {
      if (!l.fh || !l.fw || !l.stride) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.fh > kMaxSide || l.fw > kMaxSide || l.pad > kMaxSide || l.stride > kMaxSide) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (H + 2 * l.pad < l.fh || W + 2 * l.pad < l.fw) return fail(VPIN_EINVAL, fit);
      if (weights && !l.filter_le16) return fail(VPIN_EINVAL, "vpin_net: a convolution has no filter");
      p.oH = (H + 2 * l.pad - l.fh) / l.stride + 1;
      p.oW = (W + 2 * l.pad - l.fw) / l.stride + 1;
      p.mult = 2 * C * l.fh * l.fw;
      p.add = 2 * C * (l.fh * l.fw - 1);
      p.keys = 2 * C;
    } else if (l.kind == VPIN_NET_POOL) {
      if (!l.k || !l.stride) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.stride > kMaxSide) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (l.k > H || l.k > W) return fail(VPIN_EINVAL, fit);
      p.oH = (H - l.k) / l.stride + 1;
      p.oW = (W - l.k) / l.stride + 1;
      p.add = 2 * C * p.oH * p.oW * (l.k * l.k - 1);
    } else if (l.kind == VPIN_NET_FC) {
      if (!l.N || !l.K) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.N > 65535) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (l.K != C * H * W) return fail(VPIN_EINVAL, "vpin_net: a fully connected layer's K is not the C * H * W that reaches it");
      if (weights) {
        if (!l.w || !l.bias) return fail(VPIN_EINVAL, "vpin_net: a fully connected layer has no weights or no bias");
        for (size_t j = 0; j < l.K * l.N; j++)
          if (l.w[j] < 0) return fail(VPIN_EINVAL, "vpin_net: a weight of a fully connected layer is negative");
      }
      p.oC = 1; p.oH = 1; p.oW = l.N;
      p.mult = 2 * l.K;
      p.add = 2 * (l.N + l.K - 1);
      p.keys = 2;
      p.bias_r = l.N;
    } else {
      return fail(VPIN_EINVAL, "vpin_net: a layer's kind is none of conv, pool, fc");
    }
    if (l.has_round) {
      if (l.shift_bits < 0 || l.shift_bits > 62) return fail(VPIN_EINVAL, "vpin_net: a round's shift_bits is outside 0 .. 62");
      if (!l.reencrypt && i + 1 != g->n_layers) return fail(VPIN_EINVAL, "vpin_net: only the last layer's round may leave out the re-encryption");
      p.round = rounds++;
    }
    C = p.oC; H = p.oH; W = p.oW;
    out->push_back(p);
  }
  return VPIN_OK;
}

thread_local std::vector<double> g_ms;  // [0] the whole, then per layer: the layer, the round after it

struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double operator()() {
    const auto n = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
    return ms;
  }
};

// the failing call's own text behind the layer or round it happened in
int named(int rc, const std::string& where) {
  if (rc == VPIN_OK) return rc;
  const std::string why = "vpin_net_infer: " + where + ": " + vpin_last_error();
  return fail(rc, why.c_str());
}

void append(std::vector<uint8_t>* to, const std::vector<uint8_t>& from) { to->insert(to->end(), from.begin(), from.end()); }

}  // namespace

struct vpin_net_trace {
  std::vector<vpin_conv_trace*> layer;
  vpin_conv_trace label;  // the lists of all layers in layer order; the output and dims of the last layer
  ~vpin_net_trace() {
    for (vpin_conv_trace* t : layer) vpin_conv_trace_free(t);
  }
};

struct vpin_net_client {
  vpin_ctx* ctx = nullptr;
  vpin_e2_dlog* dlog = nullptr;
  vpin_e2_base *g = nullptr, *h = nullptr;
  uint8_t sk[32];
  std::vector<uint64_t> max_giant;  // per round
  std::vector<uint8_t> r;           // the queue of encryption randomness, 32 bytes each
  size_t r_pos = 0;
  std::vector<std::vector<int64_t>> v, act;
};

extern "C" {

int vpin_net_cfg_counts(const vpin_net_cfg* g, size_t* out, size_t cap) {
  if (!g || !out) return fail(VPIN_EINVAL, "vpin_net_cfg_counts: null argument");
  std::vector<LayerPlan> pl;
  const int rc = plan(g, false, &pl);
  if (rc) return rc;
  if (cap < 8 + 3 * pl.size()) return fail(VPIN_EINVAL, "vpin_net_cfg_counts: out holds fewer than 8 + 3 * n_layers values");
  size_t mult = 0, add = 0, dec = 0, enc = g->C * g->H * g->W, keys = 0, bias_r = 0, rounds = 0;
  for (size_t i = 0; i < pl.size(); i++) {
    const size_t n_out = pl[i].oC * pl[i].oH * pl[i].oW, d = pl[i].round >= 0 ? n_out : 0;
    out[8 + 3 * i] = pl[i].mult; out[9 + 3 * i] = pl[i].add; out[10 + 3 * i] = d;
    mult += pl[i].mult; add += pl[i].add; dec += d; keys += pl[i].keys; bias_r += pl[i].bias_r;
    if (pl[i].round >= 0) { rounds++; if (g->layers[i].reencrypt) enc += n_out; }
  }
  out[0] = pl.size(); out[1] = rounds; out[2] = mult; out[3] = add; out[4] = dec; out[5] = enc; out[6] = keys; out[7] = bias_r;
  return VPIN_OK;
}

void vpin_net_trace_free(vpin_net_trace* t) { delete t; }

int vpin_net_infer(vpin_ctx* c, const vpin_net_cfg* g, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                   const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const uint8_t* keys32,
                   size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user, vpin_net_trace** out) {
  if (out) *out = nullptr;
  if (!c || !g || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || !out) return fail(VPIN_EINVAL, "vpin_net_infer: null argument");
  std::vector<LayerPlan> pl;
  int rc = plan(g, true, &pl);
  if (rc) return rc;
  size_t keys = 0, bias_r = 0;
  bool any_round = false;
  for (const LayerPlan& p : pl) { keys += p.keys; bias_r += p.bias_r; any_round = any_round || p.round >= 0; }
  if (n_keys != keys) return fail(VPIN_EINVAL, "vpin_net_infer: the number of PRF keys is not one per convolution plane and fully connected row");
  if (n_bias_r != bias_r) return fail(VPIN_EINVAL, "vpin_net_infer: the number of bias randomness values is not the sum of the fully connected layers' N");
  if ((keys && !keys32) || (bias_r && (!bias_r_le32 || !baseG || !baseH)) || (any_round && !round_fn))
    return fail(VPIN_EINVAL, "vpin_net_infer: null argument");
  g_ms.assign(1 + 2 * pl.size(), 0.0);
  vpin_net_trace* t = new (std::nothrow) vpin_net_trace();
  if (!t) return VPIN_ENOMEM;
  struct Guard { vpin_net_trace* t; ~Guard() { delete t; } } guard{t};
  Lap total, lap;
  const uint8_t* key = keys32;
  const uint8_t* br = bias_r_le32;
  Pts c1, c2, a1, a2;  // what the server holds; the client's answer
  c1.assign(c1x, c1y, c1inf, g->C * g->H * g->W);
  c2.assign(c2x, c2y, c2inf, g->C * g->H * g->W);

  for (size_t i = 0; i < pl.size(); i++) {
    const vpin_net_layer& l = g->layers[i];
    const LayerPlan& p = pl[i];
    const std::string where = "layer " + std::to_string(i) + " (" + kind_name(l.kind) + ")";
    Pts in = std::move(c1);  // c1, c2 are rebuilt from this layer's output
    in.append(c2);
    vpin_conv_trace* tr = nullptr;
    if (l.kind == VPIN_NET_CONV) {
      rc = vpin_enc_conv2d(c, in.x.data(), in.y.data(), in.inf.data(), 2 * p.C, p.H, p.W, l.filter_le16, l.fh, l.fw, l.pad, l.stride, key,
                           g->prf_bytes, &tr);
    } else if (l.kind == VPIN_NET_POOL) {
      rc = vpin_enc_avgpool2d(c, in.x.data(), in.y.data(), in.inf.data(), 2 * p.C, p.H, p.W, l.k, l.stride, l.scale_le16, &tr);
    } else {
      Pts b, b2;  // the bias under the client's key: N values encrypted before the layer, as encryptBias does
      b.resize(l.N); b2.resize(l.N);
      rc = vpin_e2_encrypt(c, baseG, baseH, l.bias, br, l.N, b.x.data(), b.y.data(), b.inf.data(), b2.x.data(), b2.y.data(), b2.inf.data());
      if (!rc) {
        b.append(b2);
        std::vector<uint32_t> wu(l.K * l.N);
        for (size_t j = 0; j < l.K * l.N; j++) wu[j] = (uint32_t)l.w[j];
        rc = vpin_enc_fc(c, in.x.data(), in.y.data(), in.inf.data(), 2, l.K, (const uint8_t*)wu.data(), l.N, b.x.data(), b.y.data(),
                         b.inf.data(), key, g->prf_bytes, &tr);
      }
      br += 32 * l.N;
    }
    key += 32 * p.keys;
    g_ms[1 + 2 * i] = lap();
    if (rc) return named(rc, where);
    t->layer.push_back(tr);
    const size_t n = p.oC * p.oH * p.oW;  // the first half of the output planes is c1, the second c2
    c1.assign(tr->out_x.data(), tr->out_y.data(), tr->out_inf.data(), n);
    c2.assign(tr->out_x.data() + 32 * n, tr->out_y.data() + 32 * n, tr->out_inf.data() + n, n);
    if (p.round < 0) continue;
    const bool re = l.reencrypt != 0;
    a1.resize(re ? n : 0); a2.resize(re ? n : 0);
    const int flags = (l.relu ? VPIN_LENET_RELU : 0) | (re ? VPIN_LENET_REENCRYPT : 0);
    vpin::set_last_error_text("");  // a foreign callback may fail without a text of its own: no stale one is quoted then
    rc = round_fn(user, p.round, flags, l.shift_bits, c1.x.data(), c1.y.data(), c1.inf.data(), c2.x.data(), c2.y.data(), c2.inf.data(), n,
                  re ? a1.x.data() : nullptr, re ? a1.y.data() : nullptr, re ? a1.inf.data() : nullptr, re ? a2.x.data() : nullptr,
                  re ? a2.y.data() : nullptr, re ? a2.inf.data() : nullptr);
    g_ms[2 + 2 * i] = lap();
    if (rc) {
      if (!*vpin_last_error()) vpin::set_last_error_text("the round callback failed");
      return named(rc, "round " + std::to_string(p.round));
    }
    if (re) { std::swap(c1, a1); std::swap(c2, a2); }
  }

  // the one label: what the reference leaves in points_mult, weights_array, point_one_Add and point_two_Add
  vpin_conv_trace& L = t->label;
  const vpin_conv_trace* last = t->layer.back();
  L.P = last->P; L.oh = last->oh; L.ow = last->ow;
  L.out_x = last->out_x; L.out_y = last->out_y; L.out_inf = last->out_inf;
  for (const vpin_conv_trace* tr : t->layer) {
    L.n_mult += tr->n_mult; L.n_add += tr->n_add;
    append(&L.m_w, tr->m_w); append(&L.m_px, tr->m_px); append(&L.m_py, tr->m_py);
    append(&L.a_px, tr->a_px); append(&L.a_py, tr->a_py); append(&L.a_rx, tr->a_rx); append(&L.a_ry, tr->a_ry); append(&L.a_rz, tr->a_rz);
  }
  g_ms[0] = total();
  guard.t = nullptr;
  *out = t;
  return VPIN_OK;
}

int vpin_net_trace_layers(const vpin_net_trace* t, size_t* n) {
  if (!t || !n) return fail(VPIN_EINVAL, "vpin_net_trace_layers: null argument");
  *n = t->layer.size();
  return VPIN_OK;
}

int vpin_net_trace_layer(const vpin_net_trace* t, size_t layer, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out || layer >= t->layer.size()) return fail(VPIN_EINVAL, "vpin_net_trace_layer: null argument or no such layer");
  *out = t->layer[layer];
  return VPIN_OK;
}

int vpin_net_trace_label(const vpin_net_trace* t, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out) return fail(VPIN_EINVAL, "vpin_net_trace_label: null argument");
  *out = &t->label;
  return VPIN_OK;
}

int vpin_net_trace_instances(vpin_ctx* c, const vpin_net_trace* t, vpin_dev_instance** mult_out, vpin_dev_instance** add_out) {
  if (mult_out) *mult_out = nullptr;
  if (add_out) *add_out = nullptr;
  if (!c || !t || !mult_out || !add_out) return fail(VPIN_EINVAL, "vpin_net_trace_instances: null argument");
  return vpin_conv_trace_instances(c, &t->label, mult_out, add_out);
}

int vpin_net_trace_result(const vpin_net_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf, size_t* n) {
  if (!t || !x || !y || !inf || !n) return fail(VPIN_EINVAL, "vpin_net_trace_result: null argument");
  *n = t->label.out_inf.size() / 2;
  return vpin_conv_trace_output(&t->label, x, y, inf);
}

int vpin_net_last_timings(double* out, size_t cap) {
  if (!out) return fail(VPIN_EINVAL, "vpin_net_last_timings: null argument");
  for (size_t i = 0; i < cap; i++) out[i] = i < g_ms.size() ? g_ms[i] : 0.0;
  return VPIN_OK;
}

void vpin_net_client_free(vpin_net_client* cl) {
  if (!cl) return;
  vpin_e2_dlog_free(cl->dlog);
  vpin_e2_base_free(cl->h);
  vpin_e2_base_free(cl->g);
  delete cl;
}

int vpin_net_client_create(vpin_ctx* c, const uint8_t sk_le32[32], uint64_t nb, size_t n_rounds, const uint64_t* max_giant, const uint8_t* r_le32,
                           size_t n_r, vpin_net_client** out) {
  if (out) *out = nullptr;
  if (!c || !sk_le32 || !max_giant || (!r_le32 && n_r) || !out) return fail(VPIN_EINVAL, "vpin_net_client_create: null argument");
  if (!n_rounds || n_rounds > kMaxLayers) return fail(VPIN_EINVAL, "vpin_net_client_create: n_rounds must be in 1 .. 4096");
  vpin_net_client* cl = new (std::nothrow) vpin_net_client();
  if (!cl) return VPIN_ENOMEM;
  cl->ctx = c;
  memcpy(cl->sk, sk_le32, 32);
  cl->max_giant.assign(max_giant, max_giant + n_rounds);
  cl->v.resize(n_rounds); cl->act.resize(n_rounds);
  if (n_r) cl->r.assign(r_le32, r_le32 + 32 * n_r);
  uint8_t hx[32], hy[32], hinf = 0;
  int rc = vpin_e2_base_create(c, nullptr, nullptr, &cl->g);
  if (!rc) rc = vpin_e2_base_mul(c, cl->g, sk_le32, 1, hx, hy, &hinf);  // rejects a key that is not below the group order
  if (!rc && hinf) rc = fail(VPIN_EINVAL, "vpin_net_client_create: the key sk is zero");
  if (!rc) rc = vpin_e2_base_create(c, hx, hy, &cl->h);
  if (!rc) rc = vpin_e2_dlog_create(c, nb, &cl->dlog);
  if (rc) {
    vpin_net_client_free(cl);
    return rc;
  }
  *out = cl;
  return VPIN_OK;
}

int vpin_net_client_bases(const vpin_net_client* cl, const vpin_e2_base** baseG, const vpin_e2_base** baseH) {
  if (!cl || !baseG || !baseH) return fail(VPIN_EINVAL, "vpin_net_client_bases: null argument");
  *baseG = cl->g;
  *baseH = cl->h;
  return VPIN_OK;
}

int vpin_net_client_values(const vpin_net_client* cl, size_t round, const int64_t** v, const int64_t** act, size_t* cnt) {
  if (!cl || !v || !act || !cnt || round >= cl->v.size()) return fail(VPIN_EINVAL, "vpin_net_client_values: null argument or no such round");
  *v = cl->v[round].data();
  *act = cl->act[round].data();
  *cnt = cl->v[round].size();
  return VPIN_OK;
}

int vpin_net_client_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                          const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf,
                          uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  vpin_net_client* cl = (vpin_net_client*)user;
  if (!cl || round < 0 || (size_t)round >= cl->v.size()) return fail(VPIN_EINVAL, "vpin_net_client_round: null client or a round it was not made for");
  const bool re = (flags & VPIN_LENET_REENCRYPT) != 0;
  if (re && cl->r.size() / 32 - cl->r_pos < cnt) return fail(VPIN_EINVAL, "vpin_net_client_round: the queue of randomness r is used up");
  cl->v[round].assign(cnt, 0);
  cl->act[round].assign(cnt, 0);
  const int rc = vpin_e2_client_round(cl->ctx, cl->dlog, cl->g, cl->h, cl->sk, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, cl->max_giant[round],
                                      (flags & VPIN_LENET_RELU) != 0, shift_bits, re, re ? &cl->r[32 * cl->r_pos] : nullptr,
                                      cl->v[round].data(), cl->act[round].data(), o1x, o1y, o1inf, o2x, o2y, o2inf);
  if (re && rc == VPIN_OK) cl->r_pos += cnt;  // a failed round consumes nothing: the client can be used again
  return rc;
}

}  // extern "C"
