// wire_net.cpp -- the server's endpoint of an inference between two processes: vpin_wire_round, the round callback of the driver
// (infer_core.cpp interact) over a byte stream, and vpin_net_serve, which reads the client's public key and encrypted input off the
// stream, runs vpin_net_infer with that callback and reports the end, or its failure, to the peer.  The server holds no secret
// key.  Everything that arrives is unpacked on the device (e2_wire.hip) and so validated before a layer sees it.
// vpin_net_serve_batch is the same endpoint for up to max_batch images: it reads B off INPUT's cnt and runs vpin_net_infer_batch;
// every frame is as it was, with B times the single run's cnt.
// vpin_net_send_proofs follows DONE on the same stream: per image of a trace and per instance of its label (or of every layer) it
// builds the instance, proves it and sends one PROOF record (wire_proof.cpp), one instance at a time.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <sys/random.h>

#include "enc_conv.h"
#include "host/transcript.h"
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
  size_t n_reply = cnt;  // what REPLY must hold: of a round that pools, the pooled count (the driver's own shape, never the peer's)
  if (flags & VPIN_LENET_MAXPOOL) {
    size_t pool[5];
    int bad = vpin_net_round_pool(pool);
    if (!bad && (!pool[3] || pool[0] * pool[1] * pool[2] != cnt))
      bad = fail(VPIN_EINVAL, "vpin_wire_round: VPIN_LENET_MAXPOOL in a round whose driver names no pooling shape over cnt values");
    if (bad) return bad;
    n_reply = pool[0] * ((pool[1] - pool[3]) / pool[4] + 1) * ((pool[2] - pool[3]) / pool[4] + 1);
  }
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
  if (h.cnt != (re ? n_reply : 0)) {
    snprintf(why, sizeof why, "%s: round %d: the reply holds %u ciphertexts, the round asked for %zu", who, round, (unsigned)h.cnt, re ? n_reply : (size_t)0);
    return fail(VPIN_ESHAPE, why);
  }
  if ((rc = recv_payload_timed(w, slot, h, &p))) return named(rc, who);
  if (!re) return VPIN_OK;
  if ((rc = unpack_pair_timed(w, slot, w->ctx, p, n_reply, o1x, o1y, o1inf, o2x, o2y, o2inf))) {
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

namespace {

// the seeds of one proof: SHAKE256(master | "vPIN/wire-proof" | le32(slot) | le32(label) | u8(is_mult)) -> seed_commit | seed_proof
void proof_seeds(const uint8_t master64[64], uint32_t slot, uint32_t label, int is_mult, uint8_t out128[128]) {
  static const char domain[] = "vPIN/wire-proof";
  uint8_t tail[9];
  for (int i = 0; i < 4; i++) { tail[i] = (uint8_t)(slot >> (8 * i)); tail[4 + i] = (uint8_t)(label >> (8 * i)); }
  tail[8] = is_mult ? 1 : 0;
  vpin_host::Shake256 sh;
  sh.absorb(master64, 64);
  sh.absorb(reinterpret_cast<const uint8_t*>(domain), sizeof(domain) - 1);
  sh.absorb(tail, sizeof tail);
  sh.finalize();
  sh.squeeze(out128, 128);
}

struct InstanceGuard {
  vpin_ctx* c;
  vpin_dev_instance* g = nullptr;
  ~InstanceGuard() { vpin_dev_instance_free(c, g); }
};

// one list of a label as its instance: built, checked, proven, sent, freed.  *sent counts the PROOF records
int send_one(const char* who, vpin_ctx* c, const vpin_conv_trace* L, int is_mult, uint32_t slot, uint32_t image, uint32_t label, vpin_wire* w,
             const uint8_t master64[64], double ms[3], uint32_t* sent) {
  const size_t n_ops = is_mult ? L->n_mult : L->n_add;
  if (!n_ops) return VPIN_OK;  // a pooling label multiplies nothing; a 1 x 1 filter adds nothing
  char why[200];
  if (n_ops > VPIN_PROOF_MAX_OPS) {
    snprintf(why, sizeof why, "%s: image %u, label %u: %zu operations are above VPIN_PROOF_MAX_OPS", who, (unsigned)image, (unsigned)label, n_ops);
    return fail(VPIN_ESHAPE, why);
  }
  Lap lap;
  InstanceGuard inst{c};
  int rc = is_mult ? vpin_gadget_point_mult_dev(c, L->m_w.data(), L->m_px.data(), L->m_py.data(), n_ops, &inst.g)
                   : vpin_gadget_point_add_dev(c, L->a_px.data(), L->a_py.data(), L->a_rx.data(), L->a_ry.data(), L->a_rz.data(), n_ops, &inst.g);
  if (rc) {
    snprintf(why, sizeof why, "%s: image %u, label %u: the instance of %zu %s could not be built", who, (unsigned)image, (unsigned)label, n_ops,
             is_mult ? "multiplications" : "additions");
    return fail(rc, why);
  }
  const int sat = vpin_dev_instance_is_sat(c, inst.g);
  ms[0] += lap();
  if (sat != 1) {
    snprintf(why, sizeof why, "%s: image %u, label %u: the witness of %zu %s does not satisfy the gadget", who, (unsigned)image, (unsigned)label, n_ops,
             is_mult ? "multiplications" : "additions");
    return fail(sat < 0 ? sat : VPIN_EVERIFY, why);
  }
  uint8_t seeds[128];
  proof_seeds(master64, slot, label, is_mult, seeds);
  const size_t cap = vpin_dev_instance_proof_max_bytes(inst.g), ccap = vpin_dev_instance_comm_bytes(inst.g);
  const size_t rows = vpin_gadget_vars_rows(is_mult, n_ops);
  if (cap != vpin_gadget_proof_max_bytes(is_mult, n_ops) || ccap != vpin_gadget_comm_bytes(is_mult, n_ops)) {
    snprintf(why, sizeof why, "%s: the instance of %zu %s does not have the sizes of its shape", who, n_ops, is_mult ? "multiplications" : "additions");
    return fail(VPIN_ESHAPE, why);
  }
  // proof | comm | comm_para | comm_input, the proof at its largest first and the rest moved up behind its real length
  std::vector<uint8_t> p(cap + ccap + 64 * rows), rest(ccap + 64 * rows);
  size_t len = 0, clen = 0;
  rc = vpin_snark_prove_dev(c, inst.g, seeds, seeds + 64, p.data(), cap, &len, rest.data(), ccap, &clen, rest.data() + ccap, rest.data() + ccap + 32 * rows);
  ms[1] += lap();
  if (rc) {
    snprintf(why, sizeof why, "%s: image %u, label %u: vpin_snark_prove_dev failed", who, (unsigned)image, (unsigned)label);
    return fail(rc, why);
  }
  if (clen != ccap) return fail(VPIN_ESHAPE, (std::string(who) + ": the commitment does not have the length of its shape").c_str());
  memcpy(p.data() + len, rest.data(), rest.size());
  vpin_proof_header h;
  memset(&h, 0, sizeof h);
  h.kind = VPIN_PROOF_RECORD; h.is_mult = is_mult ? 1 : 0; h.image = image; h.label = label;
  h.n_ops = n_ops; h.proof_len = len; h.comm_len = clen;
  rc = send_proof(w, h, p.data());
  ms[2] += lap();
  if (rc) return named(rc, who);
  ++*sent;
  return VPIN_OK;
}

}  // namespace

int vpin_net_send_proofs(vpin_ctx* c, const vpin_net_trace* t, size_t first_image, size_t n_images, vpin_wire* w, int per_layer,
                         const uint8_t master_seed64[64], double ms_out[3]) {
  const char* who = "vpin_net_send_proofs";
  if (ms_out) ms_out[0] = ms_out[1] = ms_out[2] = 0.0;
  if (!c || !t || !w) return fail(VPIN_EINVAL, "vpin_net_send_proofs: null argument");
  size_t B = 0, n_layers = 0;
  int rc = vpin_net_trace_images(t, &B);
  if (!rc) rc = vpin_net_trace_layers(t, &n_layers);
  if (rc) return rc;
  if (!n_images || first_image >= B || n_images > B - first_image)
    return fail(VPIN_EINVAL, "vpin_net_send_proofs: the images are not images of the trace");
  uint8_t master[64];
  if (master_seed64) memcpy(master, master_seed64, 64);
  else if (getrandom(master, 64, 0) != 64) return fail(VPIN_ENOMEM, "vpin_net_send_proofs: the operating system gave no randomness");
  double ms[3] = {0.0, 0.0, 0.0};
  uint32_t sent = 0;
  for (size_t i = 0; i < n_images && !rc; i++) {
    const uint32_t slot = (uint32_t)(first_image + i);
    for (size_t l = 0; l < (per_layer ? n_layers : 1) && !rc; l++) {
      const vpin_conv_trace* L = nullptr;
      Lap lap;
      rc = per_layer ? vpin_net_trace_image_layer(t, slot, l, &L) : vpin_net_trace_image_label(t, slot, &L);
      ms[0] += lap();
      const uint32_t label = per_layer ? (uint32_t)(1 + l) : 0;
      for (int is_mult = 1; is_mult >= 0 && !rc; is_mult--) rc = send_one(who, c, L, is_mult, slot, (uint32_t)i, label, w, master, ms, &sent);
    }
  }
  if (ms_out) memcpy(ms_out, ms, sizeof ms);
  if (rc) {
    if (rc != VPIN_ECOMM) send_proof_error(w, rc, vpin_last_error());  // the peer is gone otherwise
    return rc;
  }
  vpin_proof_header h;
  memset(&h, 0, sizeof h);
  h.kind = VPIN_PROOF_END; h.image = sent;
  Lap lap;
  rc = send_proof(w, h, nullptr);
  if (ms_out) ms_out[2] += lap();
  return rc ? named(rc, who) : VPIN_OK;
}

}  // extern "C"
