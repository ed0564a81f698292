// infer_core.cpp -- the server loop of an encrypted inference over the layer entry points (vpin_enc_conv2d, vpin_enc_conv2d_mc[_bias],
// vpin_enc_avgpool2d, vpin_enc_fc[_signed], vpin_enc_add, vpin_e2_plane_sums_batch) and the interaction with the client as a callback per round: what vpin_lenet_infer
// (lenet.cpp) and vpin_net_infer[_batch] (net.cpp) both run.  Ciphertexts cross every layer boundary as host bytes; each layer
// validates what it is given, the client's answers included.  A batch of B images is the same loop: every layer call and every
// round takes the planes of all images at once, image after image (infer_core.h, Call).  The loop runs over the list of LIVE
// slots (infer_slots.h): all B unless the run is vpin_net_infer_isolated's, where an image that makes a layer refuse, that owns
// a point a layer's load refuses, or that the round callback drops leaves the batch and the step runs again over the others.
#include "infer_core.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <utility>

namespace vpin::infer {

namespace {

using enc::fail;

// the planes of the layer call: image after image, the image's C planes of c1 and of c2, `times` over, in the step's order
Pts gather(Pts& c1, const Pts& c2, size_t B, size_t C, size_t times, Step::Order order, bool may_move) {
  Pts in;
  if (may_move && B == 1 && times == 1 && order == Step::kBlocked) {  // c1, c2 are rebuilt from the layer's output
    in = std::move(c1);
    in.append(c2, 0, c2.n());
    return in;
  }
  const size_t img = c1.n() / B, per = img / C, n = 2 * times * c1.n();
  in.x.reserve(32 * n); in.y.reserve(32 * n); in.inf.reserve(n);
  for (size_t b = 0; b < B; b++) {
    if (order == Step::kInterleaved) {
      for (size_t p = 0; p < C * times; p++) {
        in.append(c1, b * img + (p % C) * per, per);
        in.append(c2, b * img + (p % C) * per, per);
      }
      continue;
    }
    for (size_t t = 0; t < times; t++) in.append(c1, b * img, img);
    for (size_t t = 0; t < times; t++) in.append(c2, b * img, img);
  }
  return in;
}

// the output's planes back into c1 and c2, both image-major: an image's planes are the first and the second half of its P / B
// (blocked) or the even and the odd ones
void split(const vpin_conv_trace& t, size_t B, Step::Order order, Pts* c1, Pts* c2) {
  const size_t per = t.oh * t.ow, planes = t.P / B;
  c1->resize(0); c2->resize(0);
  if (order == Step::kBlocked) {  // one run of planes / 2 planes per image and half
    const size_t run = planes / 2 * per;
    for (size_t h = 0; h < 2 * B; h++) (h % 2 ? c2 : c1)->append(&t.out_x[32 * h * run], &t.out_y[32 * h * run], &t.out_inf[h * run], run);
    return;
  }
  for (size_t p = 0; p < t.P; p++)
    (p % planes % 2 ? c2 : c1)->append(&t.out_x[32 * p * per], &t.out_y[32 * p * per], &t.out_inf[p * per], per);
}

// bias values the step encrypts per image, one r each
size_t bias_values(const Step& s) {
  return s.kind == Step::kFc || s.kind == Step::kFcs ? s.N : s.kind == Step::kConvMc && s.bias ? s.n_out : 0;
}

// every live image's n bias values under the client's key (with public keys in the call: under the key of the image's own
// client, by its slot), encrypted with the caller's r before the layer (encryptBias) by ONE call, then per image its n c1 halves
// and its n c2 halves: the layer's rows 2 b and 2 b + 1, or its groups.  r_le32: the live images' r, position after position
int encrypt_bias(const Call& a, const Slots& live, const int64_t* bias, const uint8_t* r_le32, size_t n, Pts* out) {
  const size_t B = live.n();
  Pts b1, b2;
  b1.resize(B * n); b2.resize(B * n);
  std::vector<int64_t> msgs(B * n);
  for (size_t i = 0; i < B * n; i++) msgs[i] = bias[i % n];
  int rc;
  if (a.n_pub) {
    std::vector<uint32_t> key_of(B * n);
    for (size_t i = 0; i < B * n; i++) key_of[i] = a.key_of_image[live.live[i / n]];
    rc = vpin_e2_encrypt_keyed(a.c, a.baseG, a.hx, a.hy, a.n_pub, key_of.data(), msgs.data(), r_le32, B * n, b1.x.data(), b1.y.data(),
                               b1.inf.data(), b2.x.data(), b2.y.data(), b2.inf.data());
  } else {
    rc = vpin_e2_encrypt(a.c, a.baseG, a.baseH, msgs.data(), r_le32, B * n, b1.x.data(), b1.y.data(), b1.inf.data(), b2.x.data(),
                         b2.y.data(), b2.inf.data());
  }
  if (rc) return rc;
  out->resize(0);
  for (size_t b = 0; b < B; b++) { out->append(b1, b * n, n); out->append(b2, b * n, n); }
  return VPIN_OK;
}

// the encrypted bias, then the layer on every image's c1 row and c2 row
int fc(const Call& a, const Slots& live, const Step& s, const Pts& in, const uint8_t* key, const uint8_t* r_le32, vpin_conv_trace** out) {
  Pts b;
  const int rc = encrypt_bias(a, live, s.bias, r_le32, s.N, &b);
  if (rc) return rc;
  if (s.kind == Step::kFcs)
    return vpin_enc_fc_signed(a.c, in.x.data(), in.y.data(), in.inf.data(), 2 * live.n(), s.K, s.w, s.N, b.x.data(), b.y.data(), b.inf.data(), key,
                              a.prf_bytes, out);
  std::vector<uint32_t> wu(s.K * s.N);
  for (size_t i = 0; i < s.K * s.N; i++) wu[i] = (uint32_t)s.w[i];
  return vpin_enc_fc(a.c, in.x.data(), in.y.data(), in.inf.data(), 2 * live.n(), s.K, (const uint8_t*)wu.data(), s.N, b.x.data(), b.y.data(),
                     b.inf.data(), key, a.prf_bytes, out);
}

// the trained convolution over the groups g = 2 b + half; with a bias, n_out values per image encrypted as for fc: an image's c1
// halves go to its first group, its c2 halves to its second
int conv_mc(const Call& a, const Slots& live, const Step& s, const Pts& in, size_t C, size_t H, size_t W, const uint8_t* key,
            const uint8_t* r_le32, vpin_conv_trace** out) {
  if (!s.bias)
    return vpin_enc_conv2d_mc(a.c, in.x.data(), in.y.data(), in.inf.data(), 2 * live.n(), C, s.n_out, H, W, s.w_mc, s.connect, s.fh, s.fw, s.pad,
                              s.stride, key, a.prf_bytes, out);
  Pts b;
  const int rc = encrypt_bias(a, live, s.bias, r_le32, s.n_out, &b);
  if (rc) return rc;
  return vpin_enc_conv2d_mc_bias(a.c, in.x.data(), in.y.data(), in.inf.data(), 2 * live.n(), C, s.n_out, H, W, s.w_mc, s.connect, s.fh, s.fw, s.pad,
                                 s.stride, b.x.data(), b.y.data(), b.inf.data(), key, a.prf_bytes, out);
}

// what the round callback at hand may ask and say (vpin_net_round_images, vpin_net_round_drop_images): per thread, set around
// the one call of the callback
struct Dropped {
  uint32_t slot;
  int code;
  std::string text;
};
struct RoundState {
  const Slots* live;
  bool isolated;
  size_t pool[5];  // vpin_net_round_pool
  std::vector<Dropped> dropped;
};
thread_local RoundState* g_round = nullptr;

// one interaction with the client: the step's output goes out, the activated and re-encrypted values come back into c1, c2.
// *dropped: the images the callback dropped (an isolated run), in the order it named them; they are still in c1 and c2.
// C, H, W: the shape of what goes out per image; of a round that pools they are the pooled shape afterwards, and so are c1, c2
int interact(const Call& a, const Slots& live, const Step& s, Pts* c1, Pts* c2, size_t C, size_t* H, size_t* W,
             std::vector<Dropped>* dropped) {
  const size_t n = c1->n(), k = s.round_pool_k, stride = s.round_pool_stride;
  const size_t Ho = k ? (*H - k) / stride + 1 : *H, Wo = k ? (*W - k) / stride + 1 : *W;
  Pts a1, a2;
  uint8_t* o[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // no outputs when nothing is encrypted again
  if (s.reencrypt) {
    a1.resize(live.n() * C * Ho * Wo); a2.resize(live.n() * C * Ho * Wo);
    o[0] = a1.x.data(); o[1] = a1.y.data(); o[2] = a1.inf.data(); o[3] = a2.x.data(); o[4] = a2.y.data(); o[5] = a2.inf.data();
  }
  const int flags = (s.relu ? VPIN_LENET_RELU : 0) | (s.reencrypt ? VPIN_LENET_REENCRYPT : 0) | (k ? VPIN_LENET_MAXPOOL : 0);
  set_last_error_text("");  // a foreign callback may fail without a text of its own: no stale one is quoted then
  RoundState state{&live, a.iso != nullptr, {live.n() * C, *H, *W, k, stride}, {}};
  RoundState* const outer = g_round;  // a callback that runs an inference of its own gets its own
  g_round = &state;
  const int rc = a.round_fn(a.user, s.round, flags, s.shift_bits, c1->x.data(), c1->y.data(), c1->inf.data(), c2->x.data(), c2->y.data(),
                            c2->inf.data(), n, o[0], o[1], o[2], o[3], o[4], o[5]);
  g_round = outer;
  if (rc && !*vpin_last_error()) set_last_error_text("the round callback failed");
  if (!rc && s.reencrypt) { std::swap(*c1, a1); std::swap(*c2, a2); }
  if (!rc) { *H = Ho; *W = Wo; }
  if (!rc) *dropped = std::move(state.dropped);
  return rc;
}

// the positions of the live images that own a point a layer's load refuses: the c1 and the c2 of every image through
// vpin_e2_pack, which applies the load's rules.  On the failure path only
std::vector<size_t> bad_images(const Call& a, const Pts& c1, const Pts& c2, size_t n) {
  std::vector<size_t> at;
  const size_t img = c1.n() / n;
  std::vector<uint8_t> packed(32 * img);
  for (size_t b = 0; b < n; b++)
    for (const Pts* h : {&c1, &c2})
      if (vpin_e2_pack(a.c, &h->x[32 * b * img], &h->y[32 * b * img], &h->inf[b * img], img, packed.data()) == VPIN_EINVAL) {
        at.push_back(b);
        break;
      }
  return at;
}

void write_status(vpin_net_image_status* st, int code, size_t layer, int round, const std::string& text) {
  st->code = code; st->layer = (int)layer; st->round = round;
  snprintf(st->text, sizeof st->text, "%s", text.c_str());
}

}  // namespace

bool any_negative(const int32_t* w, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (w[i] < 0) return true;
  return false;
}

int run(const Call& a, const std::vector<Step>& steps, Result* out) {
  const std::string who = std::string(a.who) + ": ";
  // the failing call's own text behind the step or round it happened in
  auto named = [&](int rc, const std::string& where) { return fail(rc, (who + where + ": " + vpin_last_error()).c_str()); };
  size_t keys = 0, bias_r = 0;
  bool any_round = false;
  for (const Step& s : steps) { keys += s.keys; bias_r += bias_values(s); any_round = any_round || s.has_round; }
  if (!a.B) return fail(VPIN_EINVAL, (who + "no image").c_str());
  if (a.n_keys != a.B * keys)
    return fail(VPIN_EINVAL, (who + "the number of PRF keys is not one per convolution plane and fully connected row").c_str());
  if (a.n_bias_r != a.B * bias_r)
    return fail(VPIN_EINVAL, (who + "the number of bias randomness values is not one per fully connected output and biased output channel").c_str());
  if ((keys && !a.keys32) || (bias_r && (!a.bias_r_le32 || !a.baseG || (!a.n_pub && !a.baseH))) ||
      (a.n_pub && (!a.hx || !a.hy || !a.key_of_image)) || (any_round && !a.round_fn))
    return fail(VPIN_EINVAL, (who + "null argument").c_str());
  out->step_ms.assign(steps.size(), 0.0);
  out->round_ms.assign(steps.size(), 0.0);
  enc::Lap total, lap;
  const size_t B = a.B;
  const uint8_t* key = a.keys32;  // slot 0's, of the step at hand; slot b's stand b * keys (b * bias_r) items on
  const uint8_t* br = a.bias_r_le32;
  size_t C = a.C, H = a.H, W = a.W;
  Slots live(B);  // the images still in the batch; all of them unless the run is isolated
  Pts c1, c2;     // what the server holds: [position][C][H][W] each
  c1.append(a.c1x, a.c1y, a.c1inf, B * C * H * W);
  c2.append(a.c2x, a.c2y, a.c2inf, B * C * H * W);
  // Tensor t is the encrypted input (t = 0) or the output of step t - 1 after its round: step i begins with tensor i in c1, c2.
  // A tensor that a step names other than as the c1, c2 at hand is kept, a copy of the pair with its shape, from the moment it is
  // at hand until the last step that names it; the kept pairs follow the live slots like c1 and c2 themselves
  struct Kept {
    Pts c1, c2;
    size_t C = 0, H = 0, W = 0;
  };
  constexpr size_t none = (size_t)-1;
  auto tensor_of = [](size_t ref, size_t i) { return ref == Step::kFromInput ? (size_t)0 : ref ? ref : i; };
  std::vector<size_t> last_use(steps.size(), none);  // per tensor the last step that takes it from `kept`
  bool any_kept = false;
  for (size_t i = 0; i < steps.size(); i++) {
    const size_t in = tensor_of(steps[i].input_from, i);
    if (in != i) last_use[in] = i;
    if (steps[i].skip_from) last_use[tensor_of(steps[i].skip_from, i)] = i;
    any_kept = any_kept || in != i || steps[i].skip_from;
  }
  std::vector<Kept> kept(any_kept ? steps.size() : 0);
  auto remove_from_all = [&](const std::vector<size_t>& at) {  // before live.remove
    remove_images(&c1, live.n(), at);
    remove_images(&c2, live.n(), at);
    for (Kept& k : kept)
      if (k.c1.n()) { remove_images(&k.c1, live.n(), at); remove_images(&k.c2, live.n(), at); }
  };
  if (a.iso)
    for (size_t b = 0; b < B; b++) write_status(&a.iso->status[b], VPIN_OK, 0, -1, "");
  // an isolated run: the images at these positions leave with their status written; false when nobody is left
  auto leave = [&](const std::vector<size_t>& at, int code, size_t layer, int round, const std::string& text) {
    for (const size_t p : at) write_status(&a.iso->status[live.live[p]], code, layer, round, text);
    remove_from_all(at);
    live.remove(at);
    return live.n() != 0;
  };
  auto nobody = [&]() { return fail(VPIN_ESHAPE, (who + "no image is left").c_str()); };
  for (size_t i = 0; i < steps.size(); i++) {
    const Step& s = steps[i];
    int rc = VPIN_OK;
    const size_t in_t = tensor_of(s.input_from, i), skip_t = s.skip_from ? tensor_of(s.skip_from, i) : none;
    if (any_kept) {
      if (last_use[i] != none) kept[i] = Kept{c1, c2, C, H, W};  // a later step, or this one by another name, reads what is at hand
      if (in_t != i) {  // the step reads a kept tensor: a copy, or the pair itself at its last use
        Kept& k = kept[in_t];
        const bool last = last_use[in_t] == i && skip_t != in_t;
        if (last) { c1 = std::move(k.c1); c2 = std::move(k.c2); } else { c1 = k.c1; c2 = k.c2; }
        C = k.C; H = k.H; W = k.W;
        if (last) k = Kept();
      }
    }
    while (s.sum_table) {  // ONE call over the groups g = 2 b + half, then the sums back into c1 and c2
      const size_t n = live.n(), img = C * H * W, out_img = s.sum_out * H * W;
      Pts in, sum;
      for (size_t b = 0; b < n; b++) { in.append(c1, b * img, img); in.append(c2, b * img, img); }
      sum.resize(2 * n * out_img);
      rc = vpin_e2_plane_sums_batch(a.c, in.x.data(), in.y.data(), in.inf.data(), 2 * n, C, H, W, s.sum_table, s.sum_out, sum.x.data(),
                                    sum.y.data(), sum.inf.data());
      if (rc == VPIN_EINVAL && a.iso) {  // a point the sums' load refuses: its image leaves, the sums run again
        const std::string text = who + s.name + ": " + vpin_last_error();
        const std::vector<size_t> at = bad_images(a, c1, c2, n);
        if (at.empty()) return fail(rc, text.c_str());
        a.iso->refused += at.size();
        a.iso->repeats++;
        if (!leave(at, rc, i, -1, text)) return nobody();
        continue;
      }
      if (rc) return named(rc, s.name);
      c1.resize(0); c2.resize(0);
      for (size_t h = 0; h < 2 * n; h++) (h % 2 ? c2 : c1).append(sum, h * out_img, out_img);
      C = s.sum_out;
      break;
    }
    if (s.kind == Step::kFc || s.kind == Step::kFcs) { W *= C * H; C = H = 1; }  // flattened: the c1 row, then the c2 row
    const size_t Cc = C * s.repeat;  // the planes per half that the call takes
    const size_t per_image = s.kind == Step::kConv || s.kind == Step::kPool || s.kind == Step::kAdd ? 2 * Cc : 2;  // planes, or groups, or rows
    vpin_conv_trace* tr = nullptr;
    for (;;) {  // the layer call; an isolated run repeats it without the images it refuses, at most B times
      const size_t n = live.n();
      const Pts in = gather(c1, c2, n, C, s.repeat, s.order, !a.iso);
      std::vector<uint8_t> own_keys, own_r;
      const uint8_t* k = of_live_images(key, keys, s.keys, live, &own_keys);
      const uint8_t* r = of_live_images(br, bias_r, bias_values(s), live, &own_r);
      enc::clear_refusals();  // a failure before the layer itself (the bias encryption) leaves no stale list
      if (s.kind == Step::kConv) {
        rc = vpin_enc_conv2d(a.c, in.x.data(), in.y.data(), in.inf.data(), n * 2 * Cc, H, W, s.filter_le16, s.fh, s.fw, s.pad, s.stride, k,
                             a.prf_bytes, &tr);
      } else if (s.kind == Step::kConvMc) {
        rc = conv_mc(a, live, s, in, Cc, H, W, k, r, &tr);
      } else if (s.kind == Step::kPool) {
        rc = vpin_enc_avgpool2d(a.c, in.x.data(), in.y.data(), in.inf.data(), n * 2 * Cc, H, W, s.k, s.stride, s.scale_le16, &tr);
      } else if (s.kind == Step::kAdd) {  // the kept pair is only read: it may have a later use
        const Pts skip = gather(kept[skip_t].c1, kept[skip_t].c2, n, C, 1, Step::kBlocked, false);
        rc = vpin_enc_add(a.c, in.x.data(), in.y.data(), in.inf.data(), skip.x.data(), skip.y.data(), skip.inf.data(), n * 2 * Cc, H, W, &tr);
      } else {
        rc = fc(a, live, s, in, k, r, &tr);
      }
      out->step_ms[i] += 1e3 * lap();
      if (!rc) break;
      if (!a.iso || (rc != VPIN_ESHAPE && rc != VPIN_EINVAL)) return named(rc, s.name);
      const std::string text = who + s.name + ": " + vpin_last_error();
      std::vector<size_t> at;
      if (rc == VPIN_ESHAPE) {  // the units the layer names, as images
        size_t n_units = 0;
        vpin_enc_last_refusals(nullptr, 0, &n_units);
        std::vector<uint32_t> units(n_units);
        vpin_enc_last_refusals(units.data(), units.size(), &n_units);
        at = positions_of_units(units.data(), units.size(), per_image, n);
      } else {  // a point the layer's load refuses: the input's, or a reply's
        at = bad_images(a, c1, c2, n);
        if (s.kind == Step::kAdd) {  // or the second operand's
          const std::vector<size_t> more = bad_images(a, kept[skip_t].c1, kept[skip_t].c2, n);
          std::vector<size_t> both;
          std::set_union(at.begin(), at.end(), more.begin(), more.end(), std::back_inserter(both));
          at = both;
        }
      }
      if (at.empty()) return fail(rc, text.c_str());  // nobody's doing, or nobody's that can be named
      a.iso->refused += at.size();
      a.iso->repeats++;
      if (!leave(at, rc, i, -1, text)) return nobody();
    }
    for (size_t t = 0; t < kept.size(); t++)
      if (last_use[t] == i) kept[t] = Kept();  // its last use
    br += 32 * bias_values(s);
    key += 32 * s.keys;
    out->step.push_back(tr);
    out->slots.push_back(live.live);
    split(*tr, live.n(), s.order, &c1, &c2);
    C = tr->P / (2 * live.n()); H = tr->oh; W = tr->ow;
    if (!s.has_round) continue;
    std::vector<Dropped> dropped;
    rc = interact(a, live, s, &c1, &c2, C, &H, &W, &dropped);
    out->round_ms[i] = 1e3 * lap();
    if (rc) return named(rc, s.round_name);
    if (dropped.empty()) continue;
    std::vector<size_t> at;  // what the callback dropped leaves after the round, each image with its own code and text
    for (const Dropped& d : dropped) {
      write_status(&a.iso->status[d.slot], d.code, i, s.round, d.text);
      at.push_back(live.position(d.slot));
    }
    std::sort(at.begin(), at.end());
    a.iso->dropped += at.size();
    remove_from_all(at);
    live.remove(at);
    if (!live.n()) return nobody();
  }
  out->survivors = live.live;
  out->total_ms = 1e3 * total();
  return VPIN_OK;
}

}  // namespace vpin::infer

extern "C" {

int vpin_net_round_images(const uint32_t** slots, size_t* n) {
  using namespace vpin::infer;
  if (!slots || !n) return fail(VPIN_EINVAL, "vpin_net_round_images: null argument");
  if (!g_round) return fail(VPIN_EINVAL, "vpin_net_round_images: no round callback is running on this thread");
  *slots = g_round->live->live.data();
  *n = g_round->live->n();
  return VPIN_OK;
}

int vpin_net_round_pool(size_t out[5]) {
  using namespace vpin::infer;
  if (!out) return fail(VPIN_EINVAL, "vpin_net_round_pool: null argument");
  if (!g_round) return fail(VPIN_EINVAL, "vpin_net_round_pool: no round callback is running on this thread");
  for (int i = 0; i < 5; i++) out[i] = g_round->pool[i];
  return VPIN_OK;
}

int vpin_net_round_drop_images(const uint32_t* slots, size_t n, int code, const char* text) {
  using namespace vpin::infer;
  if (!g_round) return fail(VPIN_EINVAL, "vpin_net_round_drop_images: no round callback is running on this thread");
  if (!g_round->isolated) return fail(VPIN_EINVAL, "vpin_net_round_drop_images: the run is not vpin_net_infer_isolated's");
  if ((n && !slots) || !code) return fail(VPIN_EINVAL, "vpin_net_round_drop_images: null argument, or the code is VPIN_OK");
  for (size_t i = 0; i < n; i++) {  // all or none
    bool twice = false;
    for (size_t j = 0; j < i; j++) twice = twice || slots[j] == slots[i];
    for (const Dropped& d : g_round->dropped) twice = twice || d.slot == slots[i];
    if (twice || g_round->live->position(slots[i]) == g_round->live->n())
      return fail(VPIN_EINVAL, ("vpin_net_round_drop_images: slot " + std::to_string(slots[i]) + " is not in the batch, or is dropped twice").c_str());
  }
  for (size_t i = 0; i < n; i++) g_round->dropped.push_back(Dropped{slots[i], code, text ? text : ""});
  return VPIN_OK;
}

}  // extern "C"
