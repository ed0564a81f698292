// wire_multi.cpp -- the server's endpoint over several wires: vpin_net_server, which keeps the checked configuration and the table
// of G across calls, and vpin_net_serve_multi, ONE inference (vpin_net_infer_multi) over the images of all admitted clients, each
// under its own public key, with every round one exchange with all of them.  Who gets which bytes is the roster's business
// (wire_roster.cpp, plain C++); here are the device's parts: ONE unpack launch over the keys and inputs of all wires at admission,
// and per round one pack launch over the batch and one unpack launch over all replies, whose rule byte per point says which
// client owns a bad one.  A client dropped in a round keeps its images in the batch: they go on as what the server sent.
// With vpin_net_server_set_isolation on the inference is vpin_net_infer_isolated: before a round the roster is re-based on the
// slots still in the batch and a client that lost an image to a layer is dropped (VPIN_NET_STAGE_LAYER); after it the images of
// the clients that are gone leave the batch (vpin_net_round_drop_images), so the later layer calls run without them.
// No table of any client's H is built: the biases are encrypted by vpin_e2_encrypt_keyed.
// vpin_net_server_send_proofs then sends every client served to DONE the proofs of its own slots (vpin_net_send_proofs per wire).
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include <sys/random.h>

#include "enc_conv.h"
#include "wire.h"

using namespace vpin::wire;

struct vpin_net_server {
  vpin_ctx* c = nullptr;
  const vpin_net_cfg* cfg = nullptr;
  size_t max_batch = 0, k = 0, r = 0, per = 0;  // per image: PRF keys, bias r, input ciphertexts
  vpin_e2_base* g = nullptr;
  uint64_t stats[5] = {0, 0, 0, 0, 0};  // calls, clients admitted, clients served to DONE, images run, base tables built
  bool isolation = false;
  uint64_t isolated[3] = {0, 0, 0};  // images of clients a layer refused, images compacted away after a wire drop, layer calls repeated
};

namespace {

const char* const kWho = "vpin_net_serve_multi";

struct Run {
  vpin_net_server* s;
  Roster* r;
  const vpin_net_image_status* image_status;  // the isolated driver's, per slot; NULL: isolation is off
};

// "point j: <rule>" for the first bad point among a client's frame of 2 * n points: its c1 part at c1, its c2 part at c2
bool first_bad(const uint8_t* bad, size_t c1, size_t c2, size_t n, std::string* text) {
  for (size_t j = 0; j < 2 * n; j++) {
    const uint8_t f = bad[j < n ? c1 + j : c2 + j - n];
    if (!f) continue;
    *text = "vpin_e2_unpack: point " + std::to_string(j) + ": " + unpack_rule_text(f);
    return true;
  }
  return false;
}

// the round callback of the driver over all live clients
int multi_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y,
                uint8_t* o2inf) {
  Run* run = (Run*)user;
  Roster& r = *run->r;
  vpin_ctx* c = run->s->c;
  const uint32_t* slots = nullptr;
  if (run->image_status) {  // the batch may have lost images since the last round: where everybody stands now, and who lost one
    size_t n = 0;
    const int rc = vpin_net_round_images(&slots, &n);
    if (rc) return rc;
    r.rebase(slots, n);
    run->s->isolated[0] += r.drop_refused(run->image_status);
    if (!r.live()) return fail(VPIN_ECOMM, (std::string(kWho) + ": round " + std::to_string(round) + ": no client is left").c_str());
  }
  const size_t per = r.batch ? cnt / r.batch : 0;
  if (round < 0 || !cnt || !r.batch || cnt % r.batch || per * r.batch > VPIN_WIRE_MAX_CNT || shift_bits < 0 || shift_bits > 255 || (flags & ~0xff))
    return fail(VPIN_EINVAL, "vpin_net_serve_multi: a round, cnt, shift_bits or flags that no header holds");
  std::vector<uint8_t> packed, reply;
  int rc = pack_pair(c, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, &packed);
  if (rc) return rc;
  if ((rc = exchange(&r, round, flags, shift_bits, packed.data(), per, &reply))) return rc;
  // isolation: the images of a client that is gone leave the batch after this round, with the client's code and text
  auto compact = [&]() {
    for (const auto& g : r.gone(slots)) {
      const vpin_net_peer_status& st = r.status[r.peers[g.first].wire];
      const int bad = vpin_net_round_drop_images(g.second.data(), g.second.size(), st.code, st.text);
      if (bad) return bad;
      if (st.stage != VPIN_NET_STAGE_LAYER) run->s->isolated[1] += g.second.size();
    }
    return VPIN_OK;
  };
  if (!(flags & VPIN_LENET_REENCRYPT)) return run->image_status ? compact() : VPIN_OK;
  std::vector<uint8_t> x(64 * cnt), y(64 * cnt), f(2 * cnt), bad(2 * cnt);
  if ((rc = unpack_rules(c, reply.data(), 2 * cnt, x.data(), y.data(), f.data(), bad.data()))) return rc;
  memcpy(o1x, x.data(), 32 * cnt); memcpy(o2x, x.data() + 32 * cnt, 32 * cnt);
  memcpy(o1y, y.data(), 32 * cnt); memcpy(o2y, y.data() + 32 * cnt, 32 * cnt);
  memcpy(o1inf, f.data(), cnt); memcpy(o2inf, f.data() + cnt, cnt);
  std::string text;
  for (size_t i = 0; i < r.peers.size(); i++) {
    const Peer& p = r.peers[i];
    if (p.live && first_bad(bad.data(), p.at * per, cnt + p.at * per, p.n * per, &text))
      r.drop(i, VPIN_EINVAL, round, "round " + std::to_string(round) + ": the reply (c1, then c2): " + text);
    if (p.live || run->image_status) continue;  // isolation: what is written for an image that leaves is ignored
    // the images of a client that is gone answer with what the server sent
    copy_images(p, per, 32, c1x, o1x); copy_images(p, per, 32, c1y, o1y); copy_images(p, per, 1, c1inf, o1inf);
    copy_images(p, per, 32, c2x, o2x); copy_images(p, per, 32, c2y, o2y); copy_images(p, per, 1, c2inf, o2inf);
  }
  if (!r.live()) return fail(VPIN_ECOMM, (std::string(kWho) + ": round " + std::to_string(round) + ": no client is left").c_str());
  return run->image_status ? compact() : VPIN_OK;
}

// what one wire sent at admission
struct Candidate {
  size_t wire = 0, n = 0, at = 0;  // its images; where its input starts among the points of the one unpack launch
  std::vector<uint8_t> hello, input;
};

int serve(vpin_net_server* s, vpin_wire* const* wires, size_t n_wires, const uint8_t* keys32, const uint8_t* bias_r_le32, Roster* r,
          vpin_net_trace** out) {
  const size_t per = s->per;
  // admission: the frames of every wire in turn, then ONE unpack launch over all keys and all inputs
  std::vector<Candidate> cand;
  size_t room = s->max_batch, points = 0;
  for (size_t i = 0; i < n_wires; i++) {
    Candidate k;
    k.wire = i;
    bool told = false;
    const int rc = read_client(wires[i], per, room, &k.hello, &k.input, &k.n, &told);
    if (rc) {
      r->report(i, rc, VPIN_NET_STAGE_ADMISSION, vpin_last_error());
      if (!told) send_error(wires[i], rc, r->status[i].text);
      continue;
    }
    room -= k.n;
    points += 2 * k.n * per;
    cand.push_back(std::move(k));
  }
  const size_t K = cand.size();
  std::vector<uint8_t> in32(32 * (K + points)), x(32 * (K + points)), y(32 * (K + points)), f(K + points), bad(K + points);
  size_t at = K;
  for (size_t j = 0; j < K; j++) {
    memcpy(&in32[32 * j], cand[j].hello.data(), 32);
    memcpy(&in32[32 * at], cand[j].input.data(), cand[j].input.size());
    cand[j].at = at;
    at += 2 * cand[j].n * per;
  }
  int rc = VPIN_OK;
  if (K) {
    Lap lap;
    rc = unpack_rules(s->c, in32.data(), K + points, x.data(), y.data(), f.data(), bad.data());
    const double ms = lap();
    for (const Candidate& k : cand) add_ms(wires[k.wire], 0, kUnpack, ms);  // the one launch, seen by every wire it served
  }
  if (rc) {
    for (const Candidate& k : cand) {
      r->report(k.wire, rc, VPIN_NET_STAGE_SERVER, vpin_last_error());
      send_error(wires[k.wire], rc, r->status[k.wire].text);
    }
    return rc;
  }
  std::vector<uint8_t> hx, hy, c1x, c1y, c1f, c2x, c2y, c2f;
  std::vector<uint32_t> key_of_image;
  for (size_t j = 0; j < K; j++) {
    const Candidate& k = cand[j];
    const size_t n = k.n * per;
    std::string text;
    if (bad[j]) text = std::string("HELLO: vpin_e2_unpack: point 0: ") + unpack_rule_text(bad[j]);
    else if (f[j]) text = "HELLO: the public key is the identity";
    else if (first_bad(bad.data(), k.at, k.at + n, n, &text)) text = "INPUT: " + text;
    if (!text.empty()) {
      r->report(k.wire, VPIN_EINVAL, VPIN_NET_STAGE_ADMISSION, text);
      send_error(wires[k.wire], VPIN_EINVAL, r->status[k.wire].text);
      continue;
    }
    key_of_image.insert(key_of_image.end(), k.n, (uint32_t)r->peers.size());
    r->admit(wires[k.wire], k.wire, k.n);
    hx.insert(hx.end(), &x[32 * j], &x[32 * j] + 32);
    hy.insert(hy.end(), &y[32 * j], &y[32 * j] + 32);
    c1x.insert(c1x.end(), &x[32 * k.at], &x[32 * k.at] + 32 * n); c2x.insert(c2x.end(), &x[32 * (k.at + n)], &x[32 * (k.at + n)] + 32 * n);
    c1y.insert(c1y.end(), &y[32 * k.at], &y[32 * k.at] + 32 * n); c2y.insert(c2y.end(), &y[32 * (k.at + n)], &y[32 * (k.at + n)] + 32 * n);
    c1f.insert(c1f.end(), &f[k.at], &f[k.at] + n); c2f.insert(c2f.end(), &f[k.at + n], &f[k.at + n] + n);
  }
  cand.clear();
  s->stats[1] += r->peers.size();
  if (r->peers.empty()) return fail(VPIN_ESHAPE, "vpin_net_serve_multi: no client was admitted");
  const size_t B = r->images;
  s->stats[3] += B;
  std::vector<vpin_net_image_status> image_status(s->isolation ? B : 0);
  Run run{s, r, s->isolation ? image_status.data() : nullptr};
  if (s->isolation) {
    rc = vpin_net_infer_isolated(s->c, s->cfg, B, c1x.data(), c1y.data(), c1f.data(), c2x.data(), c2y.data(), c2f.data(), s->g, hx.data(),
                                 hy.data(), r->peers.size(), key_of_image.data(), keys32, B * s->k, bias_r_le32, B * s->r, multi_round, &run,
                                 image_status.data(), out);
    uint64_t did[3];
    vpin_net_last_isolation(did);
    s->isolated[2] += did[2];
  } else {
    rc = vpin_net_infer_multi(s->c, s->cfg, B, c1x.data(), c1y.data(), c1f.data(), c2x.data(), c2y.data(), c2f.data(), s->g, hx.data(), hy.data(),
                              r->peers.size(), key_of_image.data(), keys32, B * s->k, bias_r_le32, B * s->r, multi_round, &run, out);
  }
  if (rc) {  // the last client gone (every status is written), or the server's own failure: the live clients are told
    std::string text = vpin_last_error();
    if (s->isolation) {  // whose image a layer refused is told the layer's text; nobody left is VPIN_ECOMM however they went
      s->isolated[0] += r->drop_refused(image_status.data());
      if (rc == VPIN_ESHAPE && !r->live()) { rc = VPIN_ECOMM; text = std::string(kWho) + ": no client is left: " + text; }
    }
    for (size_t i = 0; i < r->peers.size(); i++)
      if (r->peers[i].live) r->drop(i, rc, VPIN_NET_STAGE_SERVER, text);
    return fail(rc, text.c_str());
  }
  const size_t told = finish(r);
  s->stats[2] += told;
  if (!told) {
    vpin_net_trace_free(*out);
    *out = nullptr;
    return fail(VPIN_ECOMM, "vpin_net_serve_multi: no client was left to be told DONE");
  }
  return VPIN_OK;
}

}  // namespace

extern "C" {

int vpin_net_server_create(vpin_ctx* c, const vpin_net_cfg* cfg, size_t max_batch, vpin_net_server** out) {
  if (out) *out = nullptr;
  if (!c || !cfg || !out) return fail(VPIN_EINVAL, "vpin_net_server_create: null argument");
  std::vector<size_t> counts(8 + 3 * cfg->n_layers);
  int rc = vpin_net_cfg_counts(cfg, counts.data(), counts.size());
  if (rc) return rc;
  if (!cfg->layers[cfg->n_layers - 1].has_round)
    return fail(VPIN_EINVAL, "vpin_net_server_create: the last layer has no round: its result would never reach the clients");
  if (!max_batch || max_batch > VPIN_NET_MAX_BATCH) return fail(VPIN_EINVAL, "vpin_net_server_create: max_batch is outside 1 .. VPIN_NET_MAX_BATCH");
  // a dropped client's images are copied from a round's input to its output at ONE per-image size (compact, above)
  for (size_t i = 0; i < cfg->n_layers; i++)
    if (cfg->layers[i].round_pool_k)
      return fail(VPIN_EINVAL, ("vpin_net_server_create: layer " + std::to_string(i) + ": a round with max pooling is not served to several clients yet").c_str());
  std::unique_ptr<vpin_net_server> s(new (std::nothrow) vpin_net_server());
  if (!s) return VPIN_ENOMEM;
  s->c = c; s->cfg = cfg; s->max_batch = max_batch;
  s->k = counts[6]; s->r = counts[7]; s->per = cfg->C * cfg->H * cfg->W;
  if ((rc = vpin_e2_base_create(c, nullptr, nullptr, &s->g))) return rc;
  s->stats[4] = 1;
  *out = s.release();
  return VPIN_OK;
}

void vpin_net_server_free(vpin_net_server* s) {
  if (!s) return;
  vpin_e2_base_free(s->g);
  delete s;
}

int vpin_net_server_stats(const vpin_net_server* s, uint64_t out[5]) {
  if (!s || !out) return fail(VPIN_EINVAL, "vpin_net_server_stats: null argument");
  for (int i = 0; i < 5; i++) out[i] = s->stats[i];
  return VPIN_OK;
}

int vpin_net_server_set_isolation(vpin_net_server* s, int on) {
  if (!s) return fail(VPIN_EINVAL, "vpin_net_server_set_isolation: null argument");
  s->isolation = on != 0;
  return VPIN_OK;
}

int vpin_net_server_stats_isolation(const vpin_net_server* s, uint64_t out[3]) {
  if (!s || !out) return fail(VPIN_EINVAL, "vpin_net_server_stats_isolation: null argument");
  for (int i = 0; i < 3; i++) out[i] = s->isolated[i];
  return VPIN_OK;
}

int vpin_net_serve_multi(vpin_net_server* s, vpin_wire* const* wires, size_t n_wires, const uint8_t* keys32, size_t n_keys,
                         const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_peer_status* status, vpin_net_trace** out) {
  if (out) *out = nullptr;
  if (!s || !wires || !status || !out || (s->k && !keys32) || (s->r && !bias_r_le32)) return fail(VPIN_EINVAL, "vpin_net_serve_multi: null argument");
  if (!n_wires || n_wires > s->max_batch) return fail(VPIN_EINVAL, "vpin_net_serve_multi: n_wires is outside 1 .. max_batch");
  for (size_t i = 0; i < n_wires; i++) {
    if (!wires[i]) return fail(VPIN_EINVAL, "vpin_net_serve_multi: null argument");
    for (size_t j = 0; j < i; j++)
      if (wires[j] == wires[i]) return fail(VPIN_EINVAL, "vpin_net_serve_multi: the same wire is given twice");
  }
  if (n_keys != s->max_batch * s->k || n_bias_r != s->max_batch * s->r)
    return fail(VPIN_EINVAL, "vpin_net_serve_multi: n_keys or n_bias_r is not max_batch times what one image consumes");
  memset(status, 0, n_wires * sizeof *status);
  Roster r;
  r.who = kWho; r.max_batch = s->max_batch; r.status = status;
  s->stats[0]++;
  return serve(s, wires, n_wires, keys32, bias_r_le32, &r, out);
}

int vpin_net_server_send_proofs(vpin_net_server* s, const vpin_net_trace* t, vpin_wire* const* wires, size_t n_wires, vpin_net_peer_status* status,
                                int per_layer, const uint8_t master_seed64[64]) {
  const char* who = "vpin_net_server_send_proofs";
  if (!s || !t || !wires || !status) return fail(VPIN_EINVAL, "vpin_net_server_send_proofs: null argument");
  if (!n_wires || n_wires > s->max_batch) return fail(VPIN_EINVAL, "vpin_net_server_send_proofs: n_wires is outside 1 .. max_batch");
  for (size_t i = 0; i < n_wires; i++)
    if (!wires[i]) return fail(VPIN_EINVAL, "vpin_net_server_send_proofs: null argument");
  uint8_t master[64];  // one for the call: a slot's seeds do not depend on which wire holds it
  if (master_seed64) memcpy(master, master_seed64, 64);
  else if (getrandom(master, 64, 0) != 64) return fail(VPIN_ENOMEM, "vpin_net_server_send_proofs: the operating system gave no randomness");
  size_t ended = 0, asked = 0;
  int last = VPIN_OK;
  std::string last_text;
  for (size_t i = 0; i < n_wires; i++) {
    vpin_net_peer_status& st = status[i];
    if (st.code != VPIN_OK || st.stage != VPIN_NET_STAGE_DONE) continue;  // it left before DONE: nothing was computed for it to the end
    asked++;
    const int rc = vpin_net_send_proofs(s->c, t, st.first_image, st.n_images, wires[i], per_layer, master, nullptr);
    if (!rc) { ended++; continue; }
    last = rc;
    last_text = std::string(who) + ": " + vpin_last_error();
    st.code = rc;
    st.stage = VPIN_NET_STAGE_PROOFS;
    snprintf(st.text, sizeof st.text, "%s", last_text.c_str());
  }
  if (ended) return VPIN_OK;
  if (!asked) return fail(VPIN_ESHAPE, "vpin_net_server_send_proofs: no client was served to DONE");
  return fail(last, last_text.c_str());
}

}  // extern "C"
