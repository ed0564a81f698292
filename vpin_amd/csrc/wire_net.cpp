// wire_net.cpp -- the server's endpoint of an inference between two processes: vpin_wire_round, the round callback of the driver
// (infer_core.cpp interact) over a byte stream, and vpin_net_serve, which reads the client's public key and encrypted input off the
// stream, runs vpin_net_infer with that callback and reports the end, or its failure, to the peer.  The server holds no secret
// key.  Everything that arrives is unpacked on the device (e2_wire.hip) and so validated before a layer sees it.
// vpin_net_serve_batch is the same endpoint for up to max_batch images: it reads B off INPUT's cnt and runs vpin_net_infer_batch;
// every frame is as it was, with B times the single run's cnt.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "enc_conv.h"
#include "wire.h"

namespace vpin::wire {

void set_error(const char* text) { set_last_error_text(text); }

// c1 | c2 as one run of 2 cnt packed points, one launch
int pack_pair(vpin_ctx* c, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y,
              const uint8_t* c2inf, size_t cnt, std::vector<uint8_t>* out) {
  std::vector<uint8_t> x(64 * cnt), y(64 * cnt), f(2 * cnt);
  memcpy(x.data(), c1x, 32 * cnt); memcpy(x.data() + 32 * cnt, c2x, 32 * cnt);
  memcpy(y.data(), c1y, 32 * cnt); memcpy(y.data() + 32 * cnt, c2y, 32 * cnt);
  memcpy(f.data(), c1inf, cnt); memcpy(f.data() + cnt, c2inf, cnt);
  out->resize(64 * cnt);
  return vpin_e2_pack(c, x.data(), y.data(), f.data(), 2 * cnt, out->data());
}

int pack_pair_timed(vpin_wire* w, size_t slot, vpin_ctx* c, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x,
                    const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, std::vector<uint8_t>* out) {
  Lap lap;
  const int rc = pack_pair(c, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, out);
  add_ms(w, slot, kPack, lap());
  return rc;
}

int unpack_pair_timed(vpin_wire* w, size_t slot, vpin_ctx* c, const std::vector<uint8_t>& in, size_t cnt, uint8_t* c1x, uint8_t* c1y,
                      uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf) {
  Lap lap;
  std::vector<uint8_t> x(64 * cnt), y(64 * cnt), f(2 * cnt);
  const int rc = vpin_e2_unpack(c, in.data(), 2 * cnt, x.data(), y.data(), f.data());
  add_ms(w, slot, kUnpack, lap());
  if (rc) return rc;
  memcpy(c1x, x.data(), 32 * cnt); memcpy(c2x, x.data() + 32 * cnt, 32 * cnt);
  memcpy(c1y, y.data(), 32 * cnt); memcpy(c2y, y.data() + 32 * cnt, 32 * cnt);
  memcpy(c1inf, f.data(), cnt); memcpy(c2inf, f.data() + cnt, cnt);
  return VPIN_OK;
}

int send_frame_timed(vpin_wire* w, size_t slot, const vpin_wire_header& h, const void* payload) {
  Lap lap;
  const int rc = send_frame(w, h, payload);
  add_ms(w, slot, kSend, lap());
  return rc;
}

int recv_payload_timed(vpin_wire* w, size_t slot, const vpin_wire_header& h, std::vector<uint8_t>* payload) {
  Lap lap;
  const int rc = recv_payload(w, h, payload);
  add_ms(w, slot, kRecv, lap());
  return rc;
}

}  // namespace vpin::wire

using namespace vpin::wire;

namespace {

// the text of a failing call behind the endpoint's name
int named(int rc, const char* who) {
  const std::string why = std::string(who) + ": " + vpin_last_error();
  return fail(rc, why.c_str());
}

struct Bases {
  vpin_e2_base *g = nullptr, *h = nullptr;
  ~Bases() { vpin_e2_base_free(h); vpin_e2_base_free(g); }
};

// max_batch = 0: vpin_net_serve, one image and its own texts; otherwise vpin_net_serve_batch, B read off INPUT, k and r the
// configuration's keys and bias r per image
int serve(const char* who, vpin_ctx* c, const vpin_net_cfg* cfg, vpin_wire* w, size_t max_batch, size_t k, size_t r, const uint8_t* keys32,
          size_t n_keys, const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_trace** out) {
  char why[240];
  vpin_wire_header h;
  std::vector<uint8_t> p;
  int rc = recv_header(w, &h);
  if (rc) return named(rc, who);
  if (h.type == VPIN_WIRE_ERROR) return peer_error(w, h, who);
  if (h.type != VPIN_WIRE_HELLO) {
    snprintf(why, sizeof why, "%s: expected HELLO, the peer sent type %u", who, (unsigned)h.type);
    return fail(VPIN_ESHAPE, why);
  }
  if ((rc = recv_payload_timed(w, 0, h, &p))) return named(rc, who);
  uint8_t hx[32], hy[32], hinf = 0;
  Lap lap;
  rc = vpin_e2_unpack(c, p.data(), 1, hx, hy, &hinf);
  add_ms(w, 0, kUnpack, lap());
  if (rc) return named(rc, (std::string(who) + ": HELLO").c_str());
  if (hinf) return fail(VPIN_EINVAL, (std::string(who) + ": HELLO: the public key is the identity").c_str());
  Bases b;
  if ((rc = vpin_e2_base_create(c, nullptr, nullptr, &b.g)) || (rc = vpin_e2_base_create(c, hx, hy, &b.h))) return named(rc, who);
  if ((rc = recv_header(w, &h))) return named(rc, who);
  if (h.type == VPIN_WIRE_ERROR) return peer_error(w, h, who);
  const size_t per = cfg->C * cfg->H * cfg->W;
  if (h.type != VPIN_WIRE_INPUT || (!max_batch && h.cnt != per)) {
    snprintf(why, sizeof why, "%s: expected INPUT of %zu ciphertexts, the peer sent type %u with cnt %u", who, per, (unsigned)h.type, (unsigned)h.cnt);
    return fail(VPIN_ESHAPE, why);
  }
  const size_t n = h.cnt, B = n / per;
  if (max_batch && (n % per || B < 1 || B > max_batch)) {
    snprintf(why, sizeof why, "%s: expected INPUT of 1 .. %zu images of %zu ciphertexts, the peer sent cnt %u", who, max_batch, per, (unsigned)h.cnt);
    return fail(VPIN_ESHAPE, why);
  }
  if ((rc = recv_payload_timed(w, 0, h, &p))) return named(rc, who);
  std::vector<uint8_t> x1(32 * n), y1(32 * n), f1(n), x2(32 * n), y2(32 * n), f2(n);
  if ((rc = unpack_pair_timed(w, 0, c, p, n, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data())))
    return named(rc, (std::string(who) + ": INPUT").c_str());
  p.clear();
  w->ctx = c;
  if (!max_batch)
    rc = vpin_net_infer(c, cfg, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data(), b.g, b.h, keys32, n_keys, bias_r_le32, n_bias_r,
                        vpin_wire_round, w, out);
  else  // the first B * k keys and B * r values
    rc = vpin_net_infer_batch(c, cfg, B, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data(), b.g, b.h, keys32, B * k, bias_r_le32,
                              B * r, vpin_wire_round, w, out);
  if (rc) return rc;
  memset(&h, 0, sizeof h);
  h.type = VPIN_WIRE_DONE;
  if ((rc = send_frame(w, h, nullptr))) {
    vpin_net_trace_free(*out);
    *out = nullptr;
    return named(rc, who);
  }
  return VPIN_OK;
}

}  // namespace

extern "C" {

int vpin_wire_bind_ctx(vpin_wire* w, vpin_ctx* c) {
  if (!w) return fail(VPIN_EINVAL, "vpin_wire_bind_ctx: null argument");
  w->ctx = c;
  return VPIN_OK;
}

int vpin_wire_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                    const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf,
                    uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  const char* who = "vpin_wire_round";
  vpin_wire* w = (vpin_wire*)user;
  const bool re = (flags & VPIN_LENET_REENCRYPT) != 0;
  if (!w || !w->ctx) return fail(VPIN_EINVAL, "vpin_wire_round: null wire, or a wire not bound to a context");
  if (!c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || (re && (!o1x || !o1y || !o1inf || !o2x || !o2y || !o2inf)))
    return fail(VPIN_EINVAL, "vpin_wire_round: null argument");
  if (round < 0 || cnt == 0 || cnt > VPIN_WIRE_MAX_CNT || shift_bits < 0 || shift_bits > 255 || (flags & ~0xff))
    return fail(VPIN_EINVAL, "vpin_wire_round: a round, cnt (1 .. VPIN_WIRE_MAX_CNT), shift_bits or flags that no header holds");
  const size_t slot = 1 + (size_t)round;
  char why[200];
  std::vector<uint8_t> p;
  int rc = pack_pair_timed(w, slot, w->ctx, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, &p);
  if (rc) return named(rc, who);
  vpin_wire_header h;
  memset(&h, 0, sizeof h);
  h.type = VPIN_WIRE_ROUND; h.flags = (uint8_t)flags; h.shift_bits = (uint8_t)shift_bits;
  h.round = (uint32_t)round; h.cnt = (uint32_t)cnt; h.payload_len = 64 * (uint64_t)cnt;
  if ((rc = send_frame_timed(w, slot, h, p.data()))) return named(rc, who);
  if ((rc = recv_header(w, &h))) return named(rc, who);
  if (h.type == VPIN_WIRE_ERROR) return peer_error(w, h, who);
  if (h.type != VPIN_WIRE_REPLY) {
    snprintf(why, sizeof why, "%s: round %d: expected REPLY, the peer sent type %u", who, round, (unsigned)h.type);
    return fail(VPIN_ESHAPE, why);
  }
  if (h.round != (uint32_t)round) {
    snprintf(why, sizeof why, "%s: round %d: the reply is for round %u", who, round, (unsigned)h.round);
    return fail(VPIN_ESHAPE, why);
  }
  if (h.cnt != (re ? cnt : 0)) {
    snprintf(why, sizeof why, "%s: round %d: the reply holds %u ciphertexts, the round asked for %zu", who, round, (unsigned)h.cnt, re ? cnt : (size_t)0);
    return fail(VPIN_ESHAPE, why);
  }
  if ((rc = recv_payload_timed(w, slot, h, &p))) return named(rc, who);
  if (!re) return VPIN_OK;
  if ((rc = unpack_pair_timed(w, slot, w->ctx, p, cnt, o1x, o1y, o1inf, o2x, o2y, o2inf))) {
    snprintf(why, sizeof why, "%s: round %d: the reply (c1, then c2)", who, round);
    return named(rc, why);
  }
  return VPIN_OK;
}

namespace {

int serve_checked(const char* who, vpin_ctx* c, const vpin_net_cfg* cfg, vpin_wire* w, size_t max_batch, const uint8_t* keys32, size_t n_keys,
                  const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_trace** out) {
  const std::string name(who);
  if (out) *out = nullptr;
  if (!c || !cfg || !w || !out) return fail(VPIN_EINVAL, (name + ": null argument").c_str());
  std::vector<size_t> counts(8 + 3 * cfg->n_layers);
  int rc = vpin_net_cfg_counts(cfg, counts.data(), counts.size());  // the configuration's own rules, before anything is read
  if (!rc && (!cfg->n_layers || !cfg->layers[cfg->n_layers - 1].has_round))
    rc = fail(VPIN_EINVAL, (name + ": the last layer has no round: its result would never reach the client").c_str());
  if (!rc && max_batch > VPIN_NET_MAX_BATCH) rc = fail(VPIN_EINVAL, (name + ": max_batch is outside 1 .. VPIN_NET_MAX_BATCH").c_str());
  if (!rc && max_batch && (n_keys != max_batch * counts[6] || n_bias_r != max_batch * counts[7]))
    rc = fail(VPIN_EINVAL, (name + ": n_keys or n_bias_r is not max_batch times what one image consumes").c_str());
  if (!rc) {
    vpin_ctx* bound = w->ctx;
    rc = serve(who, c, cfg, w, max_batch, counts[6], counts[7], keys32, n_keys, bias_r_le32, n_bias_r, out);
    w->ctx = bound;
  }
  if (rc && rc != VPIN_ECOMM) send_error(w, rc, vpin_last_error());  // the peer is gone or has said so itself otherwise
  return rc;
}

}  // namespace

int vpin_net_serve(vpin_ctx* c, const vpin_net_cfg* cfg, vpin_wire* w, const uint8_t* keys32, size_t n_keys, const uint8_t* bias_r_le32,
                   size_t n_bias_r, vpin_net_trace** out) {
  return serve_checked("vpin_net_serve", c, cfg, w, 0, keys32, n_keys, bias_r_le32, n_bias_r, out);
}

int vpin_net_serve_batch(vpin_ctx* c, const vpin_net_cfg* cfg, vpin_wire* w, size_t max_batch, const uint8_t* keys32, size_t n_keys,
                         const uint8_t* bias_r_le32, size_t n_bias_r, vpin_net_trace** out) {
  if (!max_batch) {
    if (out) *out = nullptr;
    const int rc = fail(VPIN_EINVAL, "vpin_net_serve_batch: max_batch is outside 1 .. VPIN_NET_MAX_BATCH");
    if (w) send_error(w, rc, vpin_last_error());
    return rc;
  }
  return serve_checked("vpin_net_serve_batch", c, cfg, w, max_batch, keys32, n_keys, bias_r_le32, n_bias_r, out);
}

}  // extern "C"
