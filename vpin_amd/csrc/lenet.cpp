// lenet.cpp -- the whole encrypted LeNet inference behind the C ABI: the server loop of the reference's src/LeNet/Server.py
// inferenceCNN over the layer entry points (vpin_enc_conv2d, vpin_enc_avgpool2d, vpin_enc_fc, vpin_e2_plane_sums), the
// interaction with the client as a callback per round, and a ready-made client over vpin_e2_client_round (what main of
// src/LeNet/Client.py does between two layers).  Per label L1 .. L7 the trace keeps the layer's own trace, so the witness lists
// are the layers' lists in call order; the plane additions of the channel sums enter no list (the reference does not prove them).
// Ciphertexts cross every layer boundary as host bytes; each layer validates what it is given, the client's answers included.
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
  void append(const uint8_t* px, const uint8_t* py, const uint8_t* pf, size_t k) {
    x.insert(x.end(), px, px + 32 * k); y.insert(y.end(), py, py + 32 * k); inf.insert(inf.end(), pf, pf + k);
  }
};

struct Dims {
  size_t o1, p1, o2, p2;
};

size_t pooled(size_t in, size_t k, size_t stride) { return (in - k) / stride + 1; }

int check_cfg(const vpin_lenet_cfg* g, Dims* d, bool weights) {
  if (!g->connect || !g->filter_le16) return fail(VPIN_EINVAL, "vpin_lenet: the configuration has no connection table or no filter");
  if (!g->H || !g->W || !g->n1 || !g->n2 || !g->n3 || !g->f || !g->pool_k || !g->pool_stride || !g->N1 || !g->N2)
    return fail(VPIN_EINVAL, "vpin_lenet: a dimension is zero");
  if (g->H != g->W) return fail(VPIN_EINVAL, "vpin_lenet: the image must be square");
  if (g->H > 4096 || g->n1 > 4096 || g->n2 > 4096 || g->n3 > 16384 || g->N1 > 65535 || g->N2 > 65535 || g->f > 64)
    return fail(VPIN_EINVAL, "vpin_lenet: a dimension is out of range");
  if (g->prf_bytes < 1 || g->prf_bytes > 16) return fail(VPIN_EINVAL, "vpin_lenet: prf_bytes must be in 1 .. 16");
  const char* fit = "vpin_lenet: a window does not fit its plane";
  if (g->f > g->H) return fail(VPIN_EINVAL, fit);
  d->o1 = g->H - g->f + 1;
  if (g->pool_k > d->o1) return fail(VPIN_EINVAL, fit);
  d->p1 = pooled(d->o1, g->pool_k, g->pool_stride);
  if (g->f > d->p1) return fail(VPIN_EINVAL, fit);
  d->o2 = d->p1 - g->f + 1;
  if (g->pool_k > d->o2) return fail(VPIN_EINVAL, fit);
  d->p2 = pooled(d->o2, g->pool_k, g->pool_stride);
  if (g->f > d->p2) return fail(VPIN_EINVAL, fit);
  if (d->p2 != g->f) return fail(VPIN_EINVAL, "vpin_lenet: the third convolution's output is not 1 x 1");
  for (size_t o = 0; o < g->n2; o++) {
    bool any = false;
    for (size_t j = 0; j < g->n1; j++) any = any || g->connect[o * g->n1 + j] != 0;
    if (!any) return fail(VPIN_EINVAL, "vpin_lenet: a row of the connection table selects no plane");
  }
  for (int r = 0; r < 7; r++)
    if (g->shift_bits[r] < 0 || g->shift_bits[r] > 62) return fail(VPIN_EINVAL, "vpin_lenet: a round's shift_bits is outside 0 .. 62");
  if (weights) {
    if (!g->w1 || !g->w2 || !g->b1 || !g->b2) return fail(VPIN_EINVAL, "vpin_lenet: the configuration has no weights");
    for (size_t i = 0; i < g->n3 * g->N1; i++)
      if (g->w1[i] < 0) return fail(VPIN_EINVAL, "vpin_lenet: a weight of the first fully connected layer is negative");
    for (size_t i = 0; i < g->N1 * g->N2; i++)
      if (g->w2[i] < 0) return fail(VPIN_EINVAL, "vpin_lenet: a weight of the second fully connected layer is negative");
  }
  return VPIN_OK;
}

thread_local double g_ms[16] = {0};

struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double operator()() {
    const auto n = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
    return ms;
  }
};

// the failing call's own text behind the label or round it happened in
int named(int rc, const char* where) {
  if (rc == VPIN_OK) return rc;
  const std::string why = std::string("vpin_lenet_infer: ") + where + ": " + vpin_last_error();
  return fail(rc, why.c_str());
}

// a layer's output planes (k, c1), (k, c2), .. -> the c1 planes and the c2 planes, each kernel-major
void split(const vpin_conv_trace* t, Pts* c1, Pts* c2) {
  const size_t per = t->oh * t->ow;
  c1->resize(0); c2->resize(0);
  for (size_t p = 0; p < t->P; p++)
    (p % 2 ? c2 : c1)->append(&t->out_x[32 * p * per], &t->out_y[32 * p * per], &t->out_inf[p * per], per);
}

// n planes of c1 and of c2 -> (0, c1), (0, c2), (1, c1), ..
Pts interleave(const Pts& c1, const Pts& c2, size_t n) {
  const size_t per = c1.n() / n;
  Pts out;
  for (size_t p = 0; p < n; p++) {
    out.append(&c1.x[32 * p * per], &c1.y[32 * p * per], &c1.inf[p * per], per);
    out.append(&c2.x[32 * p * per], &c2.y[32 * p * per], &c2.inf[p * per], per);
  }
  return out;
}

Pts repeat(const Pts& a, size_t times) {
  Pts out;
  for (size_t i = 0; i < times; i++) out.append(a.x.data(), a.y.data(), a.inf.data(), a.n());
  return out;
}

}  // namespace

struct vpin_lenet_trace {
  vpin_conv_trace* label[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~vpin_lenet_trace() {
    for (vpin_conv_trace* t : label) vpin_conv_trace_free(t);
  }
};

struct vpin_lenet_client {
  vpin_ctx* ctx = nullptr;
  vpin_e2_dlog* dlog = nullptr;
  vpin_e2_base *g = nullptr, *h = nullptr;
  uint8_t sk[32];
  uint64_t max_giant[7];
  std::vector<uint8_t> r;  // the queue of encryption randomness, 32 bytes each
  size_t r_pos = 0;
  std::vector<int64_t> v[7], act[7];
};

extern "C" {

int vpin_lenet_cfg_default(vpin_lenet_cfg* g) {
  if (!g) return fail(VPIN_EINVAL, "vpin_lenet_cfg_default: null argument");
  memset(g, 0, sizeof *g);
  g->H = g->W = 32;
  g->n1 = 6; g->n2 = 16; g->n3 = 120;
  g->f = 5;
  g->pool_k = 2; g->pool_stride = 2;
  g->pool_scale_le16[1] = 1;  // 2^10 / k^2 = 256
  const int relu[7] = {1, 0, 1, 0, 1, 1, 1}, shift[7] = {0, 26, 0, 26, 26, 33, 0};
  for (int r = 0; r < 7; r++) {
    g->relu[r] = relu[r];
    g->shift_bits[r] = shift[r];
    g->max_giant[r] = r < 5 ? (uint64_t)1 << 11 : (uint64_t)1 << 15;  // with 2^24 baby steps: +-2^35, and +-2^39 for R6 and R7
  }
  g->prf_bytes = 13;
  g->N1 = 84; g->N2 = 10;
  return VPIN_OK;
}

int vpin_lenet_cfg_counts(const vpin_lenet_cfg* g, size_t out[32]) {
  if (!g || !out) return fail(VPIN_EINVAL, "vpin_lenet_cfg_counts: null argument");
  Dims d;
  const int rc = check_cfg(g, &d, false);
  if (rc) return rc;
  const size_t f2 = g->f * g->f, kk = g->pool_k * g->pool_k - 1;
  const size_t mult[7] = {2 * g->n1 * f2, 0, 2 * g->n2 * f2, 0, 2 * g->n3 * f2, 2 * g->n3, 2 * g->N1};
  const size_t add[7] = {2 * g->n1 * (f2 - 1), 2 * g->n1 * d.p1 * d.p1 * kk, 2 * g->n2 * (f2 - 1), 2 * g->n2 * d.p2 * d.p2 * kk,
                         2 * g->n3 * (f2 - 1), 2 * (g->N1 + g->n3 - 1), 2 * (g->N2 + g->N1 - 1)};
  const size_t dec[7] = {g->n1 * d.o1 * d.o1, g->n1 * d.p1 * d.p1, g->n2 * d.o2 * d.o2, g->n2 * d.p2 * d.p2, g->n3, g->N1, g->N2};
  size_t enc = g->H * g->W, all = 0;
  for (int r = 0; r < 7; r++) {
    out[r] = mult[r]; out[7 + r] = add[r]; out[14 + r] = dec[r];
    all += dec[r];
    if (r < 6) enc += dec[r];
  }
  out[21] = all;                                // decryptions
  out[22] = enc;                                // client encryptions, the image included
  out[23] = 2 * (g->n1 + g->n2 + g->n3) + 4;    // PRF keys
  out[24] = g->N1 + g->N2;                      // bias randomness
  for (int i = 25; i < 32; i++) out[i] = 0;
  return VPIN_OK;
}

void vpin_lenet_trace_free(vpin_lenet_trace* t) { delete t; }

int vpin_lenet_infer(vpin_ctx* c, const vpin_lenet_cfg* g, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                     const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const uint8_t* keys32,
                     size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user,
                     vpin_lenet_trace** out) {
  if (out) *out = nullptr;
  if (!c || !g || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || !baseG || !baseH || !keys32 || !bias_r_le32 || !round_fn || !out)
    return fail(VPIN_EINVAL, "vpin_lenet_infer: null argument");
  Dims d;
  int rc = check_cfg(g, &d, true);
  if (rc) return rc;
  size_t cnt[32];
  if ((rc = vpin_lenet_cfg_counts(g, cnt))) return rc;
  if (n_keys != cnt[23]) return fail(VPIN_EINVAL, "vpin_lenet_infer: the number of PRF keys is not one per convolution and fully connected call");
  if (n_bias_r != cnt[24]) return fail(VPIN_EINVAL, "vpin_lenet_infer: the number of bias randomness values is not N1 + N2");
  for (double& v : g_ms) v = 0.0;
  vpin_lenet_trace* t = new (std::nothrow) vpin_lenet_trace();
  if (!t) return VPIN_ENOMEM;
  struct Guard { vpin_lenet_trace* t; ~Guard() { delete t; } } guard{t};
  Lap total, lap;
  const uint8_t* key = keys32;
  Pts c1, c2, a1, a2;  // what the server holds; the client's answer
  c1.append(c1x, c1y, c1inf, g->H * g->W);
  c2.append(c2x, c2y, c2inf, g->H * g->W);

  // one interaction with the client: the label's output goes out, the activated and re-encrypted values come back into c1, c2
  auto interact = [&](int r) -> int {
    static const char* names[7] = {"R1", "R2", "R3", "R4", "R5", "R6", "R7"};
    split(t->label[r], &c1, &c2);
    const size_t n = c1.n();
    const int last = r == 6;
    a1.resize(last ? 0 : n); a2.resize(last ? 0 : n);
    const int flags = (g->relu[r] ? VPIN_LENET_RELU : 0) | (last ? 0 : VPIN_LENET_REENCRYPT);
    vpin::set_last_error_text("");  // a foreign callback may fail without a text of its own: no stale one is quoted then
    const int rc = round_fn(user, r, flags, g->shift_bits[r], c1.x.data(), c1.y.data(), c1.inf.data(), c2.x.data(), c2.y.data(),
                            c2.inf.data(), n, last ? nullptr : a1.x.data(), last ? nullptr : a1.y.data(), last ? nullptr : a1.inf.data(),
                            last ? nullptr : a2.x.data(), last ? nullptr : a2.y.data(), last ? nullptr : a2.inf.data());
    g_ms[7 + r] = lap();
    if (rc) {
      if (!*vpin_last_error()) vpin::set_last_error_text("the round callback failed");
      return named(rc, names[r]);
    }
    if (!last) { std::swap(c1, a1); std::swap(c2, a2); }
    return VPIN_OK;
  };
  // a convolution over per-kernel planes: (k, c1), (k, c2), .. with a key per plane
  auto conv = [&](int l, const char* name, const Pts& p1, const Pts& p2, size_t kernels, size_t side) -> int {
    const Pts in = interleave(p1, p2, kernels);
    const int rc = vpin_enc_conv2d(c, in.x.data(), in.y.data(), in.inf.data(), 2 * kernels, side, side, g->filter_le16, g->f, g->f, 0, 1, key,
                                   g->prf_bytes, &t->label[l]);
    key += 32 * 2 * kernels;
    g_ms[l] = lap();
    return named(rc, name);
  };
  auto pool = [&](int l, const char* name, size_t kernels, size_t side) -> int {
    const Pts in = interleave(c1, c2, kernels);
    const int rc = vpin_enc_avgpool2d(c, in.x.data(), in.y.data(), in.inf.data(), 2 * kernels, side, side, g->pool_k, g->pool_stride,
                                      g->pool_scale_le16, &t->label[l]);
    g_ms[l] = lap();
    return named(rc, name);
  };
  auto sums = [&](const char* name, const Pts& in, size_t n_in, size_t side, const uint8_t* table, size_t n_out, Pts* o) -> int {
    o->resize(n_out * side * side);
    return named(vpin_e2_plane_sums(c, in.x.data(), in.y.data(), in.inf.data(), n_in, side, side, table, n_out, o->x.data(), o->y.data(),
                                    o->inf.data()), name);
  };
  auto fc = [&](int l, const char* name, size_t K, const int32_t* w, size_t N, const int64_t* bias, const uint8_t* r_le32) -> int {
    Pts b1, b2;
    b1.resize(N); b2.resize(N);
    int rc = vpin_e2_encrypt(c, baseG, baseH, bias, r_le32, N, b1.x.data(), b1.y.data(), b1.inf.data(), b2.x.data(), b2.y.data(), b2.inf.data());
    if (rc) return named(rc, name);
    Pts in = std::move(c1), b = std::move(b1);  // c1, c2 are rebuilt from this layer's output by the round that follows
    in.append(c2.x.data(), c2.y.data(), c2.inf.data(), c2.n());
    b.append(b2.x.data(), b2.y.data(), b2.inf.data(), N);
    std::vector<uint32_t> wu(K * N);
    for (size_t i = 0; i < K * N; i++) wu[i] = (uint32_t)w[i];
    rc = vpin_enc_fc(c, in.x.data(), in.y.data(), in.inf.data(), 2, K, (const uint8_t*)wu.data(), N, b.x.data(), b.y.data(), b.inf.data(), key,
                     g->prf_bytes, &t->label[l]);
    key += 64;
    g_ms[l] = lap();
    return named(rc, name);
  };

  // L1: every kernel runs the one filter over the one image
  if ((rc = conv(0, "L1", repeat(c1, g->n1), repeat(c2, g->n1), g->n1, g->H)) || (rc = interact(0))) return rc;
  if ((rc = pool(1, "L2", g->n1, d.o1)) || (rc = interact(1))) return rc;
  // L3: the connected planes summed, then the filter
  Pts s1, s2;
  if ((rc = sums("L3", c1, g->n1, d.p1, g->connect, g->n2, &s1)) || (rc = sums("L3", c2, g->n1, d.p1, g->connect, g->n2, &s2))) return rc;
  if ((rc = conv(2, "L3", s1, s2, g->n2, d.p1)) || (rc = interact(2))) return rc;
  if ((rc = pool(3, "L4", g->n2, d.o2)) || (rc = interact(3))) return rc;
  // L5: every kernel takes the sum of all planes, each with keys of its own
  const std::vector<uint8_t> ones(g->n2, 1);
  if ((rc = sums("L5", c1, g->n2, d.p2, ones.data(), 1, &s1)) || (rc = sums("L5", c2, g->n2, d.p2, ones.data(), 1, &s2))) return rc;
  if ((rc = conv(4, "L5", repeat(s1, g->n3), repeat(s2, g->n3), g->n3, d.p2)) || (rc = interact(4))) return rc;
  if ((rc = fc(5, "L6", g->n3, g->w1, g->N1, g->b1, bias_r_le32)) || (rc = interact(5))) return rc;
  if ((rc = fc(6, "L7", g->N1, g->w2, g->N2, g->b2, bias_r_le32 + 32 * g->N1)) || (rc = interact(6))) return rc;
  g_ms[14] = total();
  guard.t = nullptr;
  *out = t;
  return VPIN_OK;
}

int vpin_lenet_trace_label(const vpin_lenet_trace* t, int label, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out || label < 1 || label > 7) return fail(VPIN_EINVAL, "vpin_lenet_trace_label: null argument or a label outside 1 .. 7");
  *out = t->label[label - 1];
  return VPIN_OK;
}

int vpin_lenet_trace_instances(vpin_ctx* c, const vpin_lenet_trace* t, int label, vpin_dev_instance** mult_out, vpin_dev_instance** add_out) {
  if (mult_out) *mult_out = nullptr;
  if (add_out) *add_out = nullptr;
  if (!c || !t || !mult_out || !add_out || label < 1 || label > 7)
    return fail(VPIN_EINVAL, "vpin_lenet_trace_instances: null argument or a label outside 1 .. 7");
  return vpin_conv_trace_instances(c, t->label[label - 1], mult_out, add_out);
}

int vpin_lenet_trace_result(const vpin_lenet_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf, size_t* n) {
  if (!t || !x || !y || !inf || !n) return fail(VPIN_EINVAL, "vpin_lenet_trace_result: null argument");
  *n = t->label[6]->ow;
  return vpin_conv_trace_output(t->label[6], x, y, inf);
}

void vpin_lenet_last_timings(double out[16]) {
  for (int i = 0; i < 16; i++) out[i] = g_ms[i];
}

void vpin_lenet_client_free(vpin_lenet_client* cl) {
  if (!cl) return;
  vpin_e2_dlog_free(cl->dlog);
  vpin_e2_base_free(cl->h);
  vpin_e2_base_free(cl->g);
  delete cl;
}

int vpin_lenet_client_create(vpin_ctx* c, const uint8_t sk_le32[32], uint64_t nb, const uint64_t max_giant[7], const uint8_t* r_le32,
                             size_t n_r, vpin_lenet_client** out) {
  if (out) *out = nullptr;
  if (!c || !sk_le32 || !max_giant || (!r_le32 && n_r) || !out) return fail(VPIN_EINVAL, "vpin_lenet_client_create: null argument");
  vpin_lenet_client* cl = new (std::nothrow) vpin_lenet_client();
  if (!cl) return VPIN_ENOMEM;
  cl->ctx = c;
  memcpy(cl->sk, sk_le32, 32);
  memcpy(cl->max_giant, max_giant, sizeof cl->max_giant);
  cl->r.assign(r_le32, r_le32 + 32 * n_r);
  uint8_t hx[32], hy[32], hinf = 0;
  int rc = vpin_e2_base_create(c, nullptr, nullptr, &cl->g);
  if (!rc) rc = vpin_e2_base_mul(c, cl->g, sk_le32, 1, hx, hy, &hinf);  // rejects a key that is not below the group order
  if (!rc && hinf) rc = fail(VPIN_EINVAL, "vpin_lenet_client_create: the key sk is zero");
  if (!rc) rc = vpin_e2_base_create(c, hx, hy, &cl->h);
  if (!rc) rc = vpin_e2_dlog_create(c, nb, &cl->dlog);
  if (rc) {
    vpin_lenet_client_free(cl);
    return rc;
  }
  *out = cl;
  return VPIN_OK;
}

int vpin_lenet_client_bases(const vpin_lenet_client* cl, const vpin_e2_base** baseG, const vpin_e2_base** baseH) {
  if (!cl || !baseG || !baseH) return fail(VPIN_EINVAL, "vpin_lenet_client_bases: null argument");
  *baseG = cl->g;
  *baseH = cl->h;
  return VPIN_OK;
}

int vpin_lenet_client_values(const vpin_lenet_client* cl, int round, const int64_t** v, const int64_t** act, size_t* cnt) {
  if (!cl || !v || !act || !cnt || round < 1 || round > 7) return fail(VPIN_EINVAL, "vpin_lenet_client_values: null argument or a round outside 1 .. 7");
  *v = cl->v[round - 1].data();
  *act = cl->act[round - 1].data();
  *cnt = cl->v[round - 1].size();
  return VPIN_OK;
}

int vpin_lenet_client_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                            const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* o1x, uint8_t* o1y,
                            uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  vpin_lenet_client* cl = (vpin_lenet_client*)user;
  if (!cl || round < 0 || round > 6) return fail(VPIN_EINVAL, "vpin_lenet_client_round: null client or a round outside 0 .. 6");
  const bool re = (flags & VPIN_LENET_REENCRYPT) != 0;
  if (re && cl->r.size() / 32 - cl->r_pos < cnt) return fail(VPIN_EINVAL, "vpin_lenet_client_round: the queue of randomness r is used up");
  cl->v[round].assign(cnt, 0);
  cl->act[round].assign(cnt, 0);
  const int rc = vpin_e2_client_round(cl->ctx, cl->dlog, cl->g, cl->h, cl->sk, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, cl->max_giant[round],
                                      (flags & VPIN_LENET_RELU) != 0, shift_bits, re, re ? &cl->r[32 * cl->r_pos] : nullptr,
                                      cl->v[round].data(), cl->act[round].data(), o1x, o1y, o1inf, o2x, o2y, o2inf);
  if (re && rc == VPIN_OK) cl->r_pos += cnt;  // a failed round consumes nothing: the client can be used again
  return rc;
}

}  // extern "C"
