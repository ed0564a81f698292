// net.cpp -- an encrypted inference as a list of layers behind the C ABI: the server loop of the reference's
// src/cnn_networks/Server.py inferenceCNN (conv2_ciphertext, avgPool_ciphertext, flattening, FC1, FC2) as steps of the one
// driver (infer_core.cpp).  The planes go through a layer as all c1 planes and then all c2 planes, the order of
// callConv2_ciphertext on c1 and then on c2; that service appends every layer's operations to the same four global lists, so
// the trace offers, beside each layer's own trace, the lists of all layers concatenated in layer order: the network's ONE label.
// vpin_net_infer_batch is the same function over B images (vpin_net_infer: B = 1): every layer one call and every round one
// callback over the planes of all images, image after image; the label is then the images' labels one after the other, and
// vpin_net_trace_image_label cuts image b's own out of the layer calls' traces.
// vpin_net_infer_multi is the batch with the images of several clients: a public key per image instead of one table of H.
// vpin_net_infer_isolated is that with images that leave: the trace keeps per layer the slots of the images in its call, and an
// image is asked for by its slot wherever it stands.
// A CONV layer may say what the reference's LeNet needs (channel sums in front of it, its planes handed over several times, the
// interleaved plane order: the driver's own Step fields), and vpin_lenet_as_net (lenet.cpp) writes that network as such a list;
// its labels are single layers: vpin_net_trace_image_layer.
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "infer_core.h"

using vpin::enc::fail;
using vpin::infer::Step;

namespace {

const char* kind_name(int kind) {
  return kind == VPIN_NET_CONV ? "conv" : kind == VPIN_NET_POOL ? "pool" : kind == VPIN_NET_CONVMC ? "convmc" : kind == VPIN_NET_FCS ? "fcs"
         : kind == VPIN_NET_ADD ? "add" : "fc";
}

// per layer what it consumes and leaves; the walk that vpin_net_cfg_counts and vpin_net_infer share
struct LayerPlan {
  size_t oC, oH, oW;     // the tensor after the layer and its round: what the next layer and every reference see
  size_t sumC, inC;      // the planes per half that reach the channel sums, and the layer call behind sums and repeat
  size_t mult, add, keys, bias_r;
  int round;             // index of the round after the layer, or -1
  size_t iH, iW;         // the plane that reaches the layer (input_from followed)
  size_t dH, dW;         // the plane the layer call leaves and its round decrypts: oH x oW unless the round pools
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
  // a reference of layer i as a tensor: 0 the encrypted input, t the output of layer t - 1; false: the layer itself or a later one
  auto tensor_of = [](size_t ref, size_t i, size_t* t) {
    if (ref == VPIN_NET_FROM_INPUT) { *t = 0; return true; }
    *t = ref ? ref : i;
    return ref <= i;
  };
  auto shape_of = [&](size_t t, size_t* c, size_t* h, size_t* w) {
    if (t) { *c = (*out)[t - 1].oC; *h = (*out)[t - 1].oH; *w = (*out)[t - 1].oW; } else { *c = g->C; *h = g->H; *w = g->W; }
  };
  for (size_t i = 0; i < g->n_layers; i++) {
    const vpin_net_layer& l = g->layers[i];
    const std::string at = "vpin_net: layer " + std::to_string(i) + ": ";
    size_t in_t = i, skip_t = 0;
    if (!tensor_of(l.input_from, i, &in_t))
      return fail(VPIN_EINVAL, (at + "input_from = " + std::to_string(l.input_from) + " names the layer itself or a later one").c_str());
    if (l.skip_from && l.kind != VPIN_NET_ADD) return fail(VPIN_EINVAL, (at + "only an addition layer takes a skip_from").c_str());
    if (l.skip_from && !tensor_of(l.skip_from, i, &skip_t))
      return fail(VPIN_EINVAL, (at + "skip_from = " + std::to_string(l.skip_from) + " names the layer itself or a later one").c_str());
    if (l.input_from) shape_of(in_t, &C, &H, &W);
    LayerPlan p{C, H, W, C, C, 0, 0, 0, 0, -1, H, W, 0, 0};
    const char* fit = "vpin_net: a window does not fit its plane";
    if (l.kind == VPIN_NET_ADD) {  // before the rules of the other kinds: an addition layer's own texts
      if (!l.skip_from) return fail(VPIN_EINVAL, (at + "an addition layer has no skip_from").c_str());
      if (l.plane_order || l.sum_table || l.repeat > 1)
        return fail(VPIN_EINVAL, (at + "an addition layer takes no plane_order, sum_table or repeat").c_str());
      if (skip_t == in_t)
        return fail(VPIN_EINVAL, (at + "an addition layer's two operands are the same tensor (every addition would be a doubling)").c_str());
      size_t sC, sH, sW;
      shape_of(skip_t, &sC, &sH, &sW);
      auto dims = [](size_t c, size_t h, size_t w) { return std::to_string(c) + " x " + std::to_string(h) + " x " + std::to_string(w); };
      if (sC != C || sH != H || sW != W)
        return fail(VPIN_EINVAL, (at + "an addition layer's operands differ in shape: C x H x W = " + dims(C, H, W) + " and " + dims(sC, sH, sW)).c_str());
    }
    if (l.kind != VPIN_NET_CONV && (l.sum_table || l.repeat > 1)) return fail(VPIN_EINVAL, "vpin_net: only a convolution takes a sum_table or a repeat");
    if (l.plane_order != 0 && l.plane_order != VPIN_NET_ORDER_INTERLEAVED)
      return fail(VPIN_EINVAL, "vpin_net: a layer's plane_order is neither 0 nor VPIN_NET_ORDER_INTERLEAVED");
    if (l.kind == VPIN_NET_ADD) {  // the shape goes through; no keys, no bias r
      p.add = 2 * C * H * W;
    } else if (l.kind == VPIN_NET_CONV) {
      if (l.sum_table) {  // like a trained convolution's table, architecture: read here
        if (!l.sum_out) return fail(VPIN_EINVAL, "vpin_net: a convolution has a sum_table and sum_out = 0");
        if (l.sum_out > kMaxPlanes) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
        for (size_t o = 0; o < l.sum_out; o++) {
          bool any = false;
          for (size_t ch = 0; ch < C; ch++) any = any || l.sum_table[o * C + ch] != 0;
          if (!any) return fail(VPIN_EINVAL, "vpin_net: a row of a convolution's sum_table selects no plane");
        }
        C = l.sum_out;
      }
      if (l.repeat > kMaxPlanes || C * (l.repeat ? l.repeat : 1) > kMaxPlanes) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      C *= l.repeat ? l.repeat : 1;
      p.oC = p.inC = C;
      if (!l.fh || !l.fw || !l.stride) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.fh > kMaxSide || l.fw > kMaxSide || l.pad > kMaxSide || l.stride > kMaxSide) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (H + 2 * l.pad < l.fh || W + 2 * l.pad < l.fw) return fail(VPIN_EINVAL, fit);
      if (weights && !l.filter_le16) return fail(VPIN_EINVAL, "vpin_net: a convolution has no filter");
      p.oH = (H + 2 * l.pad - l.fh) / l.stride + 1;
      p.oW = (W + 2 * l.pad - l.fw) / l.stride + 1;
      p.mult = 2 * C * l.fh * l.fw;
      p.add = 2 * C * (l.fh * l.fw - 1);
      p.keys = 2 * C;
    } else if (l.kind == VPIN_NET_CONVMC) {
      if (!l.fh || !l.fw || !l.stride || !l.n_out) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.fh > kMaxSide || l.fw > kMaxSide || l.pad > kMaxSide || l.stride > kMaxSide || l.n_out > kMaxPlanes)
        return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (H + 2 * l.pad < l.fh || W + 2 * l.pad < l.fw) return fail(VPIN_EINVAL, fit);
      if (weights && !l.w_mc) return fail(VPIN_EINVAL, "vpin_net: a trained convolution has no weights");
      size_t pairs = 0;  // the table is architecture: the counts need it, the weights they do not
      for (size_t o = 0; o < l.n_out; o++) {
        size_t row = 0;
        for (size_t ch = 0; ch < C; ch++) row += !l.connect || l.connect[o * C + ch];
        if (!row) return fail(VPIN_EINVAL, "vpin_net: a row of a trained convolution's connect selects no channel");
        pairs += row;
      }
      p.oC = l.n_out;
      p.oH = (H + 2 * l.pad - l.fh) / l.stride + 1;
      p.oW = (W + 2 * l.pad - l.fw) / l.stride + 1;
      p.mult = 2 * l.fh * l.fw * pairs;
      p.add = p.mult - 2 * l.n_out;
      p.keys = 2 * l.n_out;
      if (l.bias) {  // like the table, whether there is a bias is architecture: n_out values, an addition per output
        p.bias_r = l.n_out;
        p.add += 2 * l.n_out * p.oH * p.oW;
      }
    } else if (l.kind == VPIN_NET_POOL) {
      if (!l.k || !l.stride) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.stride > kMaxSide) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (l.k > H || l.k > W) return fail(VPIN_EINVAL, fit);
      p.oH = (H - l.k) / l.stride + 1;
      p.oW = (W - l.k) / l.stride + 1;
      p.add = 2 * C * p.oH * p.oW * (l.k * l.k - 1);
    } else if (l.kind == VPIN_NET_FC || l.kind == VPIN_NET_FCS) {
      if (!l.N || !l.K) return fail(VPIN_EINVAL, "vpin_net: a dimension is zero");
      if (l.N > 65535) return fail(VPIN_EINVAL, "vpin_net: a dimension is out of range");
      if (l.K != C * H * W) return fail(VPIN_EINVAL, "vpin_net: a fully connected layer's K is not the C * H * W that reaches it");
      if (weights) {
        if (!l.w || !l.bias) return fail(VPIN_EINVAL, "vpin_net: a fully connected layer has no weights or no bias");
        if (l.kind == VPIN_NET_FC && vpin::infer::any_negative(l.w, l.K * l.N)) return fail(VPIN_EINVAL, "vpin_net: a weight of a fully connected layer is negative");
      }
      p.oC = 1; p.oH = 1; p.oW = l.N;
      p.mult = 2 * l.K;
      p.add = 2 * (l.N + l.K - 1);
      p.keys = 2;
      p.bias_r = l.N;
    } else {
      return fail(VPIN_EINVAL, "vpin_net: a layer's kind is none of conv, pool, fc, convmc, fcs, add");
    }
    if (l.has_round) {
      if (l.shift_bits < 0 || l.shift_bits > 62) return fail(VPIN_EINVAL, "vpin_net: a round's shift_bits is outside 0 .. 62");
      if (!l.reencrypt && i + 1 != g->n_layers) return fail(VPIN_EINVAL, "vpin_net: only the last layer's round may leave out the re-encryption");
      p.round = rounds++;
    }
    p.dH = p.oH; p.dW = p.oW;
    if (l.round_pool_k || l.round_pool_stride) {  // the client pools inside the round: the tensor that goes on is C x Ho x Wo
      if (!l.has_round) return fail(VPIN_EINVAL, (at + "round_pool_k or round_pool_stride on a layer without a round").c_str());
      if (!l.round_pool_k || !l.round_pool_stride)
        return fail(VPIN_EINVAL, (at + "round_pool_k = " + std::to_string(l.round_pool_k) + " beside round_pool_stride = " +
                                  std::to_string(l.round_pool_stride) + ": one of the two is zero").c_str());
      if (l.round_pool_k > p.dH || l.round_pool_k > p.dW)
        return fail(VPIN_EINVAL, (at + "the round's pooling window " + std::to_string(l.round_pool_k) + " does not fit the layer's " +
                                  std::to_string(p.dH) + " x " + std::to_string(p.dW) + " output").c_str());
      p.oH = (p.dH - l.round_pool_k) / l.round_pool_stride + 1;
      p.oW = (p.dW - l.round_pool_k) / l.round_pool_stride + 1;
    }
    C = p.oC; H = p.oH; W = p.oW;
    out->push_back(p);
  }
  return VPIN_OK;
}

thread_local std::vector<double> g_ms;  // [0] the whole, then per layer: the layer, the round after it
thread_local uint64_t g_isolation[3] = {0, 0, 0};  // vpin_net_last_isolation

// the share of the image at position b among the B of a layer call, of that call's lists, behind L's.  Every layer kind emits its
// lists plane by plane (row by row, pair by pair) and an image's planes stand together, so the share is the b-th of B equal parts
void append_image(vpin_conv_trace* L, const vpin_conv_trace& tr, size_t b, size_t B) {
  auto part = [&](std::vector<uint8_t>* to, const std::vector<uint8_t>& from) {
    const size_t n = from.size() / B;
    to->insert(to->end(), from.begin() + b * n, from.begin() + (b + 1) * n);
  };
  L->n_mult += tr.n_mult / B; L->n_add += tr.n_add / B;
  part(&L->m_w, tr.m_w); part(&L->m_px, tr.m_px); part(&L->m_py, tr.m_py);
  part(&L->a_px, tr.a_px); part(&L->a_py, tr.a_py); part(&L->a_rx, tr.a_rx); part(&L->a_ry, tr.a_ry); part(&L->a_rz, tr.a_rz);
}

// what a layer call at B images must not exceed: its planes (behind the channel sums and the repeat), groups or rows are a grid
// axis of its kernels (65535), its chains' terms, its outputs and the points around its channel sums an int.  At B = 1 the layer
// itself says so, with its own text
int fits(const char* who, const vpin_net_cfg* g, const std::vector<LayerPlan>& pl, size_t B) {
  for (size_t i = 0; i < pl.size(); i++) {
    const vpin_net_layer& l = g->layers[i];
    const std::string name = std::string(who) + ": layer " + std::to_string(i) + " (" + kind_name(l.kind) + "): ";
    const bool fc = l.kind == VPIN_NET_FC || l.kind == VPIN_NET_FCS;
    const size_t planes = fc ? 2 * B : 2 * B * pl[i].inC;
    if (l.sum_table) {  // H, W of what reaches the layer
      const size_t hw = pl[i].iH * pl[i].iW, most = pl[i].sumC > l.sum_out ? pl[i].sumC : l.sum_out;
      if (2 * B * most * hw >= ((size_t)1 << 31))
        return fail(VPIN_EINVAL, (name + "the planes of all images around the channel sums are 2^31 points or more").c_str());
    }
    if (planes > 65535)
      return fail(VPIN_EINVAL, (name + "2 B * C = " + std::to_string(planes) + " planes are more than the 65535 a layer call takes").c_str());
    if (fc && 2 * B * l.K >= ((size_t)1 << 31))
      return fail(VPIN_EINVAL, (name + "2 B * K = " + std::to_string(2 * B * l.K) + " chain terms are 2^31 or more").c_str());
    if (2 * B * pl[i].oC * pl[i].dH * pl[i].dW >= ((size_t)1 << 31))
      return fail(VPIN_EINVAL, (name + "the outputs of all images are 2^31 or more").c_str());
  }
  return VPIN_OK;
}

}  // namespace

struct vpin_net_trace {
  vpin::infer::Result run;  // per layer the trace of its layer call over all images
  vpin_conv_trace label;    // per image, in image order, the lists of all layers in layer order; the output and dims of the last layer
  size_t B = 1;
  // where slot b stands in layer's call (run.slots: the images that were in it), or npos when it had left
  static constexpr size_t npos = (size_t)-1;
  size_t position(size_t layer, size_t b) const {
    const std::vector<uint32_t>& in = run.slots[layer];
    const auto it = std::lower_bound(in.begin(), in.end(), (uint32_t)b);
    return it != in.end() && *it == b ? (size_t)(it - in.begin()) : npos;
  }
  bool survived(size_t b) const { return std::binary_search(run.survivors.begin(), run.survivors.end(), (uint32_t)b); }
  // VPIN_ESHAPE naming the first layer whose call image b was not in (n_layers: it left in the last round)
  int left(const char* who, size_t b) const {
    size_t layer = 0;
    while (layer < run.slots.size() && position(layer, b) != npos) layer++;
    return fail(VPIN_ESHAPE, (std::string(who) + ": image " + std::to_string(b) + " left the batch at " +
                              (layer < run.slots.size() ? "layer " + std::to_string(layer) : std::string("the last round"))).c_str());
  }
  mutable std::vector<std::unique_ptr<vpin_conv_trace>> image;  // B > 1: image b's label once it has been asked for
  mutable std::vector<std::unique_ptr<vpin_conv_trace>> image_layer;  // B > 1: [layer][b], image b's share of a layer call likewise
};

namespace {

// the public keys of vpin_net_infer_multi; none (n_pub = 0) for the other two
struct PubKeys {
  const uint8_t *hx = nullptr, *hy = nullptr;
  size_t n_pub = 0;
  const uint32_t* key_of_image = nullptr;
};

// vpin_net_infer (B = 1), vpin_net_infer_batch and vpin_net_infer_multi: the steps of the one driver and the label
int infer(const char* who, vpin_ctx* c, const vpin_net_cfg* g, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
          const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const uint8_t* keys32,
          size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user, vpin_net_trace** out,
          const PubKeys& pub = PubKeys(), vpin_net_image_status* status = nullptr) {
  if (out) *out = nullptr;
  if (!c || !g || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || !out) return fail(VPIN_EINVAL, (std::string(who) + ": null argument").c_str());
  if (!B || B > VPIN_NET_MAX_BATCH)
    return fail(VPIN_EINVAL, (std::string(who) + ": B = " + std::to_string(B) + " is outside 1 .. VPIN_NET_MAX_BATCH (" +
                              std::to_string(VPIN_NET_MAX_BATCH) + ")").c_str());
  std::vector<LayerPlan> pl;
  int bad = plan(g, true, &pl);
  if (!bad && B > 1) bad = fits(who, g, pl, B);
  if (bad) return bad;
  std::vector<Step> steps(pl.size());
  for (size_t i = 0; i < pl.size(); i++) {
    const vpin_net_layer& l = g->layers[i];
    Step& s = steps[i];
    s.kind = l.kind == VPIN_NET_CONV ? Step::kConv : l.kind == VPIN_NET_POOL ? Step::kPool : l.kind == VPIN_NET_CONVMC ? Step::kConvMc
             : l.kind == VPIN_NET_FCS ? Step::kFcs : l.kind == VPIN_NET_ADD ? Step::kAdd : Step::kFc;
    s.input_from = l.input_from; s.skip_from = l.skip_from;
    s.filter_le16 = l.filter_le16; s.fh = l.fh; s.fw = l.fw; s.pad = l.pad; s.stride = l.stride;
    if (l.kind == VPIN_NET_CONV) { s.sum_table = l.sum_table; s.sum_out = l.sum_out; s.repeat = l.repeat ? l.repeat : 1; }
    if ((l.kind == VPIN_NET_CONV || l.kind == VPIN_NET_POOL) && l.plane_order == VPIN_NET_ORDER_INTERLEAVED) s.order = Step::kInterleaved;
    if (l.kind == VPIN_NET_CONVMC) { s.n_out = l.n_out; s.w_mc = l.w_mc; s.connect = l.connect; }  // no other kind reads them
    s.k = l.k; s.scale_le16 = l.scale_le16;
    s.K = l.K; s.N = l.N; s.w = l.w; s.bias = l.bias;
    s.keys = pl[i].keys;
    s.name = "layer " + std::to_string(i) + " (" + kind_name(l.kind) + ")";
    s.has_round = pl[i].round >= 0;
    s.round = pl[i].round; s.relu = l.relu; s.shift_bits = l.shift_bits; s.reencrypt = l.reencrypt;
    s.round_pool_k = l.round_pool_k; s.round_pool_stride = l.round_pool_stride;
    s.round_name = "round " + std::to_string(pl[i].round);
  }
  std::unique_ptr<vpin_net_trace> t(new (std::nothrow) vpin_net_trace());
  if (!t) return VPIN_ENOMEM;
  t->B = B;
  vpin::infer::Isolation iso;  // vpin_net_infer_isolated: with a status array
  iso.status = status;
  const vpin::infer::Call call{c, who, g->prf_bytes, g->C, g->H, g->W, c1x, c1y, c1inf, c2x, c2y, c2inf, baseG, baseH,
                               keys32, n_keys, bias_r_le32, n_bias_r, round_fn, user, B, pub.hx, pub.hy, pub.n_pub, pub.key_of_image,
                               status ? &iso : nullptr};
  const vpin::infer::Result& res = t->run;
  const int rc = vpin::infer::run(call, steps, &t->run);
  if (status) { g_isolation[0] = iso.refused; g_isolation[1] = iso.dropped; g_isolation[2] = iso.repeats; }
  g_ms.assign(1 + 2 * pl.size(), 0.0);
  for (size_t i = 0; i < res.step_ms.size(); i++) { g_ms[1 + 2 * i] = res.step_ms[i]; g_ms[2 + 2 * i] = res.round_ms[i]; }
  if (rc == VPIN_EINVAL && !status && B > 1 && res.step.empty() && !res.step_ms.empty() && res.step_ms[0] > 0.0) {  // layer 0 ran and failed
    // the first layer refuses the caller's input without saying which point: of a batch the caller wants to know whose.  The
    // packing names the first point that is not a point of E2, counted over the whole batch (image = index / (C H W))
    const std::string text = vpin_last_error();
    const size_t n = B * g->C * g->H * g->W;
    std::vector<uint8_t> packed(32 * n);
    for (int half = 0; half < 2; half++)
      if (vpin_e2_pack(c, half ? c2x : c1x, half ? c2y : c1y, half ? c2inf : c1inf, n, packed.data()) == VPIN_EINVAL)
        return fail(rc, (text + "; the input's " + (half ? "c2" : "c1") + ": " + vpin_last_error()).c_str());
    return fail(rc, text.c_str());
  }
  if (rc) return rc;

  // the one label: what the reference leaves in points_mult, weights_array, point_one_Add and point_two_Add, image after image
  vpin::enc::Lap lap;
  vpin_conv_trace& L = t->label;
  const vpin_conv_trace* last = res.step.back();
  const size_t n_last = res.slots.back().size(), n_left = res.survivors.size();
  L.P = last->P / n_last * n_left; L.oh = last->oh; L.ow = last->ow;
  if (n_left == n_last) {
    L.out_x = last->out_x; L.out_y = last->out_y; L.out_inf = last->out_inf;
  } else {  // images left in the last round: the output of those that stayed, in slot order
    const size_t n = last->out_inf.size() / n_last;
    for (const uint32_t b : res.survivors) {
      const size_t at = t->position(res.step.size() - 1, b);
      L.out_x.insert(L.out_x.end(), last->out_x.begin() + 32 * at * n, last->out_x.begin() + 32 * (at + 1) * n);
      L.out_y.insert(L.out_y.end(), last->out_y.begin() + 32 * at * n, last->out_y.begin() + 32 * (at + 1) * n);
      L.out_inf.insert(L.out_inf.end(), last->out_inf.begin() + at * n, last->out_inf.begin() + (at + 1) * n);
    }
  }
  for (const uint32_t b : res.survivors)
    for (size_t i = 0; i < res.step.size(); i++) append_image(&L, *res.step[i], t->position(i, b), res.slots[i].size());
  t->image.resize(B);
  t->image_layer.resize(B * res.step.size());
  g_ms[0] = res.total_ms + 1e3 * lap();  // the whole, the label included
  *out = t.release();
  return VPIN_OK;
}

}  // namespace

extern "C" {

int vpin_net_cfg_counts(const vpin_net_cfg* g, size_t* out, size_t cap) {
  if (!g || !out) return fail(VPIN_EINVAL, "vpin_net_cfg_counts: null argument");
  std::vector<LayerPlan> pl;
  const int rc = plan(g, false, &pl);
  if (rc) return rc;
  if (cap < 8 + 3 * pl.size()) return fail(VPIN_EINVAL, "vpin_net_cfg_counts: out holds fewer than 8 + 3 * n_layers values");
  size_t mult = 0, add = 0, dec = 0, enc = g->C * g->H * g->W, keys = 0, bias_r = 0, rounds = 0;
  for (size_t i = 0; i < pl.size(); i++) {
    const size_t n_out = pl[i].oC * pl[i].oH * pl[i].oW, d = pl[i].round >= 0 ? pl[i].oC * pl[i].dH * pl[i].dW : 0;
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
  return infer("vpin_net_infer", c, g, 1, c1x, c1y, c1inf, c2x, c2y, c2inf, baseG, baseH, keys32, n_keys, bias_r_le32, n_bias_r, round_fn, user, out);
}

int vpin_net_infer_batch(vpin_ctx* c, const vpin_net_cfg* g, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                         const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const vpin_e2_base* baseH,
                         const uint8_t* keys32, size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn,
                         void* user, vpin_net_trace** out) {
  return infer("vpin_net_infer_batch", c, g, B, c1x, c1y, c1inf, c2x, c2y, c2inf, baseG, baseH, keys32, n_keys, bias_r_le32, n_bias_r, round_fn, user,
               out);
}

int vpin_net_infer_multi(vpin_ctx* c, const vpin_net_cfg* g, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                         const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const uint8_t* hx, const uint8_t* hy,
                         size_t n_pub, const uint32_t* key_of_image, const uint8_t* keys32, size_t n_keys, const uint8_t* bias_r_le32,
                         size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user, vpin_net_trace** out) {
  if (out) *out = nullptr;
  if (!hx || !hy || !key_of_image) return fail(VPIN_EINVAL, "vpin_net_infer_multi: null argument");
  if (!n_pub) return fail(VPIN_EINVAL, "vpin_net_infer_multi: n_pub = 0: no public key");
  for (size_t b = 0; b < B && b < VPIN_NET_MAX_BATCH; b++)
    if (key_of_image[b] >= n_pub)
      return fail(VPIN_EINVAL, ("vpin_net_infer_multi: key_of_image[" + std::to_string(b) + "] = " + std::to_string(key_of_image[b]) +
                                " is not below n_pub = " + std::to_string(n_pub)).c_str());
  return infer("vpin_net_infer_multi", c, g, B, c1x, c1y, c1inf, c2x, c2y, c2inf, baseG, nullptr, keys32, n_keys, bias_r_le32, n_bias_r, round_fn, user,
               out, PubKeys{hx, hy, n_pub, key_of_image});
}

int vpin_net_infer_isolated(vpin_ctx* c, const vpin_net_cfg* g, size_t B, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                            const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const vpin_e2_base* baseG, const uint8_t* hx,
                            const uint8_t* hy, size_t n_pub, const uint32_t* key_of_image, const uint8_t* keys32, size_t n_keys,
                            const uint8_t* bias_r_le32, size_t n_bias_r, vpin_lenet_round_fn round_fn, void* user,
                            vpin_net_image_status* status, vpin_net_trace** out) {
  if (out) *out = nullptr;
  for (uint64_t& v : g_isolation) v = 0;
  if (!hx || !hy || !key_of_image || !status) return fail(VPIN_EINVAL, "vpin_net_infer_isolated: null argument");
  if (!n_pub) return fail(VPIN_EINVAL, "vpin_net_infer_isolated: n_pub = 0: no public key");
  for (size_t b = 0; b < B && b < VPIN_NET_MAX_BATCH; b++)
    if (key_of_image[b] >= n_pub)
      return fail(VPIN_EINVAL, ("vpin_net_infer_isolated: key_of_image[" + std::to_string(b) + "] = " + std::to_string(key_of_image[b]) +
                                " is not below n_pub = " + std::to_string(n_pub)).c_str());
  return infer("vpin_net_infer_isolated", c, g, B, c1x, c1y, c1inf, c2x, c2y, c2inf, baseG, nullptr, keys32, n_keys, bias_r_le32, n_bias_r, round_fn,
               user, out, PubKeys{hx, hy, n_pub, key_of_image}, status);
}

void vpin_net_last_isolation(uint64_t out[3]) {
  for (int i = 0; i < 3; i++) out[i] = g_isolation[i];
}

int vpin_net_trace_layer_images(const vpin_net_trace* t, size_t layer, const uint32_t** slots, size_t* n) {
  if (!t || !slots || !n || layer >= t->run.slots.size()) return fail(VPIN_EINVAL, "vpin_net_trace_layer_images: null argument or no such layer");
  *slots = t->run.slots[layer].data();
  *n = t->run.slots[layer].size();
  return VPIN_OK;
}

int vpin_net_trace_images(const vpin_net_trace* t, size_t* B) {
  if (!t || !B) return fail(VPIN_EINVAL, "vpin_net_trace_images: null argument");
  *B = t->B;
  return VPIN_OK;
}

int vpin_net_trace_image_label(const vpin_net_trace* t, size_t b, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out || b >= t->B) return fail(VPIN_EINVAL, "vpin_net_trace_image_label: null argument or no such image");
  if (t->B == 1) { *out = &t->label; return VPIN_OK; }
  if (!t->survived(b)) return t->left("vpin_net_trace_image_label", b);
  if (!t->image[b]) {
    std::unique_ptr<vpin_conv_trace> L(new (std::nothrow) vpin_conv_trace());
    if (!L) return VPIN_ENOMEM;
    const vpin_conv_trace& all = t->label;  // its output is the survivors': image b's planes are the part at its place among them
    const size_t left = t->run.survivors.size(), n = all.out_inf.size() / left;
    const size_t at = (size_t)(std::lower_bound(t->run.survivors.begin(), t->run.survivors.end(), (uint32_t)b) - t->run.survivors.begin());
    L->P = all.P / left; L->oh = all.oh; L->ow = all.ow;
    L->out_x.assign(all.out_x.begin() + 32 * at * n, all.out_x.begin() + 32 * (at + 1) * n);
    L->out_y.assign(all.out_y.begin() + 32 * at * n, all.out_y.begin() + 32 * (at + 1) * n);
    L->out_inf.assign(all.out_inf.begin() + at * n, all.out_inf.begin() + (at + 1) * n);
    for (size_t i = 0; i < t->run.step.size(); i++) append_image(L.get(), *t->run.step[i], t->position(i, b), t->run.slots[i].size());
    t->image[b] = std::move(L);
  }
  *out = t->image[b].get();
  return VPIN_OK;
}

int vpin_net_trace_image_layer(const vpin_net_trace* t, size_t b, size_t layer, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out || b >= t->B || layer >= t->run.step.size())
    return fail(VPIN_EINVAL, "vpin_net_trace_image_layer: null argument, no such image or no such layer");
  if (t->B == 1) { *out = t->run.step[layer]; return VPIN_OK; }
  const size_t at = t->position(layer, b), in_call = t->run.slots[layer].size();
  if (at == vpin_net_trace::npos) return t->left("vpin_net_trace_image_layer", b);
  std::unique_ptr<vpin_conv_trace>& slot = t->image_layer[layer * t->B + b];
  if (!slot) {
    std::unique_ptr<vpin_conv_trace> L(new (std::nothrow) vpin_conv_trace());
    if (!L) return VPIN_ENOMEM;
    const vpin_conv_trace& all = *t->run.step[layer];  // an image's planes stand together: every array's part at its position
    auto part = [&](std::vector<uint8_t>* to, const std::vector<uint8_t>& from) {
      const size_t n = from.size() / in_call;
      to->assign(from.begin() + at * n, from.begin() + (at + 1) * n);
    };
    L->P = all.P / in_call; L->oh = all.oh; L->ow = all.ow;
    part(&L->out_x, all.out_x); part(&L->out_y, all.out_y); part(&L->out_inf, all.out_inf);
    part(&L->left_x, all.left_x); part(&L->left_y, all.left_y); part(&L->left_inf, all.left_inf);
    append_image(L.get(), all, at, in_call);
    slot = std::move(L);
  }
  *out = slot.get();
  return VPIN_OK;
}

int vpin_net_trace_image_instances(vpin_ctx* c, const vpin_net_trace* t, size_t b, vpin_dev_instance** mult_out, vpin_dev_instance** add_out) {
  if (mult_out) *mult_out = nullptr;
  if (add_out) *add_out = nullptr;
  if (!c || !t || !mult_out || !add_out) return fail(VPIN_EINVAL, "vpin_net_trace_image_instances: null argument");
  const vpin_conv_trace* L = nullptr;
  const int rc = vpin_net_trace_image_label(t, b, &L);
  return rc ? rc : vpin_conv_trace_instances(c, L, mult_out, add_out);
}

int vpin_net_trace_layers(const vpin_net_trace* t, size_t* n) {
  if (!t || !n) return fail(VPIN_EINVAL, "vpin_net_trace_layers: null argument");
  *n = t->run.step.size();
  return VPIN_OK;
}

int vpin_net_trace_layer(const vpin_net_trace* t, size_t layer, const vpin_conv_trace** out) {
  if (out) *out = nullptr;
  if (!t || !out || layer >= t->run.step.size()) return fail(VPIN_EINVAL, "vpin_net_trace_layer: null argument or no such layer");
  *out = t->run.step[layer];
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
  *n = t->label.out_inf.size() / (2 * t->run.survivors.size());
  return vpin_conv_trace_output(&t->label, x, y, inf);
}

int vpin_net_last_timings(double* out, size_t cap) {
  if (!out) return fail(VPIN_EINVAL, "vpin_net_last_timings: null argument");
  for (size_t i = 0; i < cap; i++) out[i] = i < g_ms.size() ? g_ms[i] : 0.0;
  return VPIN_OK;
}

}  // extern "C"
