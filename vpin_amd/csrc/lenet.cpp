// lenet.cpp -- the whole encrypted LeNet inference behind the C ABI: the server loop of the reference's src/LeNet/Server.py
// inferenceCNN as seven steps of the one driver (infer_core.cpp), planes in the order (kernel 0, c1), (kernel 0, c2), ..  Per
// label L1 .. L7 the trace keeps the layer's own trace, so the witness lists are the layers' lists in call order; the plane
// additions of the channel sums enter no list (the reference does not prove them).  vpin_lenet_as_net says the same seven steps
// as a vpin_net_cfg, for the batched, wired and multi-client paths of net.cpp.
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "infer_core.h"

using vpin::enc::fail;
using vpin::infer::Step;

namespace {

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
    using vpin::infer::any_negative;
    if (any_negative(g->w1, g->n3 * g->N1)) return fail(VPIN_EINVAL, "vpin_lenet: a weight of the first fully connected layer is negative");
    if (any_negative(g->w2, g->N1 * g->N2)) return fail(VPIN_EINVAL, "vpin_lenet: a weight of the second fully connected layer is negative");
  }
  return VPIN_OK;
}

thread_local double g_ms[16] = {0};  // [0..6] L1 .. L7, [7..13] R1 .. R7, [14] the whole

}  // namespace

struct vpin_lenet_trace {
  vpin::infer::Result run;  // step l is label L(l + 1)
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

int vpin_lenet_as_net(const vpin_lenet_cfg* g, vpin_net_layer layers[7], uint8_t* ones, vpin_net_cfg* out) {
  if (!g || !layers || !ones || !out) return fail(VPIN_EINVAL, "vpin_lenet_as_net: null argument");
  Dims d;
  const int bad = check_cfg(g, &d, true);
  if (bad) return bad;
  memset(ones, 1, g->n2);
  memset(layers, 0, 7 * sizeof *layers);
  const int kinds[7] = {VPIN_NET_CONV, VPIN_NET_POOL, VPIN_NET_CONV, VPIN_NET_POOL, VPIN_NET_CONV, VPIN_NET_FC, VPIN_NET_FC};
  for (int l = 0; l < 7; l++) {  // the steps of vpin_lenet_infer below, said as layers
    vpin_net_layer& y = layers[l];
    y.kind = kinds[l];
    y.has_round = 1; y.relu = g->relu[l]; y.shift_bits = g->shift_bits[l]; y.reencrypt = l < 6; y.max_giant = g->max_giant[l];
    if (y.kind == VPIN_NET_CONV) { y.filter_le16 = g->filter_le16; y.fh = y.fw = g->f; y.stride = 1; }
    if (y.kind == VPIN_NET_POOL) { y.k = g->pool_k; y.stride = g->pool_stride; memcpy(y.scale_le16, g->pool_scale_le16, 16); }
    if (y.kind != VPIN_NET_FC) y.plane_order = VPIN_NET_ORDER_INTERLEAVED;
  }
  layers[0].repeat = g->n1;
  layers[2].sum_table = g->connect; layers[2].sum_out = g->n2;
  layers[4].sum_table = ones; layers[4].sum_out = 1; layers[4].repeat = g->n3;
  layers[5].K = g->n3; layers[5].N = g->N1; layers[5].w = g->w1; layers[5].bias = g->b1;
  layers[6].K = g->N1; layers[6].N = g->N2; layers[6].w = g->w2; layers[6].bias = g->b2;
  out->C = 1; out->H = g->H; out->W = g->W;
  out->prf_bytes = g->prf_bytes;
  out->n_layers = 7;
  out->layers = layers;
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
  const int bad = check_cfg(g, &d, true);
  if (bad) return bad;
  const std::vector<uint8_t> ones(g->n2, 1);
  const Step::Kind kinds[7] = {Step::kConv, Step::kPool, Step::kConv, Step::kPool, Step::kConv, Step::kFc, Step::kFc};
  std::vector<Step> steps(7);
  for (int l = 0; l < 7; l++) {
    Step& s = steps[l];
    s.order = Step::kInterleaved;
    s.name = "L" + std::to_string(l + 1);
    s.has_round = true;
    s.round = l; s.relu = g->relu[l]; s.shift_bits = g->shift_bits[l]; s.reencrypt = l < 6;  // R7 is the result: nothing is encrypted
    s.round_name = "R" + std::to_string(l + 1);
    s.kind = kinds[l];
    if (s.kind == Step::kConv) { s.filter_le16 = g->filter_le16; s.fh = s.fw = g->f; }
    if (s.kind == Step::kPool) { s.k = g->pool_k; s.stride = g->pool_stride; s.scale_le16 = g->pool_scale_le16; }
    if (s.kind == Step::kFc) s.keys = 2;
  }
  // L1: every kernel runs the one filter over the one image
  steps[0].repeat = g->n1; steps[0].keys = 2 * g->n1;
  // L3: the connected planes summed, then the filter
  steps[2].sum_table = g->connect; steps[2].sum_out = g->n2; steps[2].keys = 2 * g->n2;
  // L5: every kernel takes the sum of all planes, computed once, each with keys of its own
  steps[4].sum_table = ones.data(); steps[4].sum_out = 1; steps[4].repeat = g->n3; steps[4].keys = 2 * g->n3;
  steps[5].K = g->n3; steps[5].N = g->N1; steps[5].w = g->w1; steps[5].bias = g->b1;
  steps[6].K = g->N1; steps[6].N = g->N2; steps[6].w = g->w2; steps[6].bias = g->b2;
  std::unique_ptr<vpin_lenet_trace> t(new (std::nothrow) vpin_lenet_trace());
  if (!t) return VPIN_ENOMEM;
  const vpin::infer::Call call{c, "vpin_lenet_infer", g->prf_bytes, 1, g->H, g->W, c1x, c1y, c1inf, c2x, c2y, c2inf, baseG, baseH,
                               keys32, n_keys, bias_r_le32, n_bias_r, round_fn, user};
  const int rc = vpin::infer::run(call, steps, &t->run);
  for (double& v : g_ms) v = 0.0;
  for (size_t l = 0; l < t->run.step_ms.size(); l++) { g_ms[l] = t->run.step_ms[l]; g_ms[7 + l] = t->run.round_ms[l]; }
  g_ms[14] = t->run.total_ms;
  if (rc) return rc;
  *out = t.release();
  return VPIN_OK;
}

int vpin_lenet_trace_label(const vpin_lenet_trace* t, int label, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out || label < 1 || label > 7) return fail(VPIN_EINVAL, "vpin_lenet_trace_label: null argument or a label outside 1 .. 7");
  *out = t->run.step[label - 1];
  return VPIN_OK;
}

int vpin_lenet_trace_instances(vpin_ctx* c, const vpin_lenet_trace* t, int label, vpin_dev_instance** mult_out, vpin_dev_instance** add_out) {
  if (mult_out) *mult_out = nullptr;
  if (add_out) *add_out = nullptr;
  if (!c || !t || !mult_out || !add_out || label < 1 || label > 7)
    return fail(VPIN_EINVAL, "vpin_lenet_trace_instances: null argument or a label outside 1 .. 7");
  return vpin_conv_trace_instances(c, t->run.step[label - 1], mult_out, add_out);
}

int vpin_lenet_trace_result(const vpin_lenet_trace* t, const uint8_t** x, const uint8_t** y, const uint8_t** inf, size_t* n) {
  if (!t || !x || !y || !inf || !n) return fail(VPIN_EINVAL, "vpin_lenet_trace_result: null argument");
  *n = t->run.step[6]->ow;
  return vpin_conv_trace_output(t->run.step[6], x, y, inf);
}

void vpin_lenet_last_timings(double out[16]) {
  for (int i = 0; i < 16; i++) out[i] = g_ms[i];
}

}  // extern "C"
