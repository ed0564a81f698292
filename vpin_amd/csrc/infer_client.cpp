// infer_client.cpp -- the ready-made client of an encrypted inference, for any number of rounds: a vpin_lenet_round_fn over
// vpin_e2_client_round (what main of the reference's Client.py does between two layers) around an object that owns the key, the
// two base tables, the discrete-log table and the queue of encryption randomness, and keeps every round's values.
// Behind DONE the same client verifies the proofs of its images (vpin_net_verifier, vpin_net_client_verify): the records come off
// the stream through the state machine of wire_proof.cpp, the computation commitments are derived here, never taken from the peer.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"
#include "wire.h"

using vpin::enc::fail;

struct vpin_net_client {
  vpin_ctx* ctx = nullptr;
  vpin_e2_dlog* dlog = nullptr;
  vpin_e2_base *g = nullptr, *h = nullptr;
  uint8_t sk[32];
  std::vector<uint64_t> max_giant;  // per round
  std::vector<uint8_t> r;           // the queue of encryption randomness, 32 bytes each
  size_t r_pos = 0;
  std::vector<std::vector<int64_t>> v, act;
  std::vector<vpin_net_round_pool_spec> pools;  // per round, the client's own; all zero: the round does not pool
};

extern "C" {

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
  if (!n_rounds || n_rounds > 4096) return fail(VPIN_EINVAL, "vpin_net_client_create: n_rounds must be in 1 .. 4096");
  vpin_net_client* cl = new (std::nothrow) vpin_net_client();
  if (!cl) return VPIN_ENOMEM;
  cl->ctx = c;
  memcpy(cl->sk, sk_le32, 32);
  cl->max_giant.assign(max_giant, max_giant + n_rounds);
  cl->v.resize(n_rounds); cl->act.resize(n_rounds);
  cl->pools.assign(n_rounds, vpin_net_round_pool_spec{0, 0, 0, 0});
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

int vpin_net_client_act_count(const vpin_net_client* cl, size_t round, size_t* n) {
  if (!cl || !n || round >= cl->act.size()) return fail(VPIN_EINVAL, "vpin_net_client_act_count: null argument or no such round");
  *n = cl->act[round].size();
  return VPIN_OK;
}

int vpin_net_client_set_pools(vpin_net_client* cl, const vpin_net_round_pool_spec* pools, size_t n_rounds) {
  if (!cl || !pools) return fail(VPIN_EINVAL, "vpin_net_client_set_pools: null argument");
  if (n_rounds != cl->pools.size()) return fail(VPIN_EINVAL, "vpin_net_client_set_pools: n_rounds is not the rounds the client was made for");
  for (size_t i = 0; i < n_rounds; i++) {
    const vpin_net_round_pool_spec& p = pools[i];
    if (!p.H && !p.W && !p.k && !p.stride) continue;
    if (!p.H || !p.W || !p.k || !p.stride || p.k > p.H || p.k > p.W || p.H >= ((size_t)1 << 30) || p.W >= ((size_t)1 << 30))
      return fail(VPIN_EINVAL, ("vpin_net_client_set_pools: round " + std::to_string(i) +
                                ": H, W, k and stride are neither all zero nor a window that fits its plane").c_str());
  }
  cl->pools.assign(pools, pools + n_rounds);
  return VPIN_OK;
}

int vpin_net_client_round(void* user, int round, int flags, int shift_bits, const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                          const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf,
                          uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  vpin_net_client* cl = (vpin_net_client*)user;
  if (!cl || round < 0 || (size_t)round >= cl->v.size()) return fail(VPIN_EINVAL, "vpin_net_client_round: null client or a round it was not made for");
  const bool re = (flags & VPIN_LENET_REENCRYPT) != 0;
  // the pooling schedule is the client's: it does not pool, or leave it, because a server says so.  Before anything is decrypted
  const vpin_net_round_pool_spec& pool = cl->pools[round];
  if (((flags & VPIN_LENET_MAXPOOL) != 0) != (pool.k != 0)) {
    cl->v[round].clear(); cl->act[round].clear();
    char why[240];
    if (pool.k)
      snprintf(why, sizeof why, "vpin_net_client_round: round %d: the server asks for a round without max pooling, the client's schedule pools "
               "%zu x %zu planes by k = %zu, stride = %zu", round, pool.H, pool.W, pool.k, pool.stride);
    else
      snprintf(why, sizeof why, "vpin_net_client_round: round %d: the server asks for max pooling (flags %d), the client's schedule has none in this round",
               round, flags);
    return fail(VPIN_ESHAPE, why);
  }
  if (pool.k && (cnt == 0 || cnt % (pool.H * pool.W))) {
    cl->v[round].clear(); cl->act[round].clear();
    char why[240];
    snprintf(why, sizeof why, "vpin_net_client_round: round %d: the server sends %zu ciphertexts, the client's schedule pools planes of %zu x %zu = %zu",
             round, cnt, pool.H, pool.W, pool.H * pool.W);
    return fail(VPIN_ESHAPE, why);
  }
  const size_t planes = pool.k ? cnt / (pool.H * pool.W) : 0;
  const size_t n_out = pool.k ? planes * ((pool.H - pool.k) / pool.stride + 1) * ((pool.W - pool.k) / pool.stride + 1) : cnt;
  if (re && cl->r.size() / 32 - cl->r_pos < n_out) return fail(VPIN_EINVAL, "vpin_net_client_round: the queue of randomness r is used up");
  cl->v[round].assign(cnt, 0);
  cl->act[round].assign(n_out, 0);
  const uint8_t* r = re ? &cl->r[32 * cl->r_pos] : nullptr;
  const int rc = pool.k ? vpin_e2_client_round_pool(cl->ctx, cl->dlog, cl->g, cl->h, cl->sk, c1x, c1y, c1inf, c2x, c2y, c2inf, planes, pool.H, pool.W,
                                                    pool.k, pool.stride, cl->max_giant[round], (flags & VPIN_LENET_RELU) != 0, shift_bits, re, r,
                                                    cl->v[round].data(), cl->act[round].data(), o1x, o1y, o1inf, o2x, o2y, o2inf)
                        : vpin_e2_client_round(cl->ctx, cl->dlog, cl->g, cl->h, cl->sk, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, cl->max_giant[round],
                                               (flags & VPIN_LENET_RELU) != 0, shift_bits, re, r, cl->v[round].data(), cl->act[round].data(), o1x,
                                               o1y, o1inf, o2x, o2y, o2inf);
  if (re && rc == VPIN_OK) cl->r_pos += n_out;  // a failed round consumes nothing: the client can be used again
  return rc;
}

// The client's endpoint over a byte stream (wire.h): HELLO and INPUT, then one vpin_net_client_round per ROUND frame that is
// exactly what the client's own schedule says comes next.  A mismatch is answered with ERROR before anything is decrypted
int vpin_net_client_run(vpin_net_client* cl, vpin_wire* w, const int64_t* image, const uint8_t* image_r_le32, size_t n_input,
                        const vpin_wire_round_spec* schedule, size_t n_rounds) {
  namespace wr = vpin::wire;
  const char* who = "vpin_net_client_run";
  if (!cl || !w || !image || !image_r_le32 || !schedule) return fail(VPIN_EINVAL, "vpin_net_client_run: null argument");
  if (n_input == 0 || n_input > VPIN_WIRE_MAX_CNT) return fail(VPIN_EINVAL, "vpin_net_client_run: n_input must be in 1 .. VPIN_WIRE_MAX_CNT");
  if (n_rounds == 0 || n_rounds > cl->v.size()) return fail(VPIN_EINVAL, "vpin_net_client_run: n_rounds must be in 1 .. the rounds the client was made for");
  char why[240];
  // the failing call's text behind this endpoint's name; told: the peer hears of it too
  auto failed = [&](int rc, const std::string& where, bool told) {
    const std::string text = std::string(who) + ": " + where + vpin_last_error();
    if (told) wr::send_error(w, rc, text.c_str());
    return fail(rc, text.c_str());
  };
  vpin_wire_header h;
  std::vector<uint8_t> p;
  // HELLO: H = sk * G
  uint8_t hx[32], hy[32], hinf = 0;
  int rc = vpin_e2_base_mul(cl->ctx, cl->g, cl->sk, 1, hx, hy, &hinf);
  if (rc) return failed(rc, "", false);
  p.resize(32);
  wr::Lap lap;
  rc = vpin_e2_pack(cl->ctx, hx, hy, &hinf, 1, p.data());
  wr::add_ms(w, 0, wr::kPack, lap());
  if (rc) return failed(rc, "", false);
  memset(&h, 0, sizeof h);
  h.type = VPIN_WIRE_HELLO; h.cnt = 1; h.payload_len = 32;
  if ((rc = wr::send_frame_timed(w, 0, h, p.data()))) return failed(rc, "", false);
  // INPUT: the image under the client's key
  {
    std::vector<uint8_t> x1(32 * n_input), y1(32 * n_input), f1(n_input), x2(32 * n_input), y2(32 * n_input), f2(n_input);
    rc = vpin_e2_encrypt(cl->ctx, cl->g, cl->h, image, image_r_le32, n_input, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data());
    if (!rc) rc = wr::pack_pair_timed(w, 0, cl->ctx, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data(), n_input, &p);
    if (rc) return failed(rc, "the input: ", true);
  }
  h.type = VPIN_WIRE_INPUT; h.cnt = (uint32_t)n_input; h.payload_len = 64 * (uint64_t)n_input;
  if ((rc = wr::send_frame_timed(w, 0, h, p.data()))) return failed(rc, "", false);
  for (size_t done = 0;;) {
    if ((rc = wr::recv_header(w, &h))) return failed(rc, "", rc != VPIN_ECOMM);
    if (h.type == VPIN_WIRE_ERROR) return wr::peer_error(w, h, who);
    if (h.type == VPIN_WIRE_DONE) {
      if (done == n_rounds) return VPIN_OK;
      snprintf(why, sizeof why, "%s: the server is done after %zu of %zu rounds", who, done, n_rounds);
      return fail(VPIN_ESHAPE, why);
    }
    why[0] = 0;
    if (h.type != VPIN_WIRE_ROUND) {
      snprintf(why, sizeof why, "%s: expected ROUND or DONE, the server sent type %u", who, (unsigned)h.type);
    } else if (done == n_rounds) {
      snprintf(why, sizeof why, "%s: the server asks for round %u, the schedule ends after %zu rounds", who, (unsigned)h.round, n_rounds);
    } else {
      const vpin_wire_round_spec& s = schedule[done];
      if (h.round != done)
        snprintf(why, sizeof why, "%s: the server asks for round %u, the schedule says round %zu comes next", who, (unsigned)h.round, done);
      else if ((int)h.flags != s.flags)
        snprintf(why, sizeof why, "%s: round %zu: the server asks for flags %d (relu %d, reencrypt %d), the schedule says %d", who, done,
                 (int)h.flags, (h.flags & VPIN_LENET_RELU) != 0, (h.flags & VPIN_LENET_REENCRYPT) != 0, s.flags);
      else if ((int)h.shift_bits != s.shift_bits)
        snprintf(why, sizeof why, "%s: round %zu: the server asks for shift_bits %d, the schedule says %d", who, done, (int)h.shift_bits, s.shift_bits);
      else if ((size_t)h.cnt != s.cnt)
        snprintf(why, sizeof why, "%s: round %zu: the server sends %u ciphertexts, the schedule says %zu", who, done, (unsigned)h.cnt, s.cnt);
    }
    if (why[0]) {  // nothing is decrypted: the payload is read into nothing, so that the peer is not left writing, and refused
      const std::string text = why;
      if (wr::discard_payload(w, h) == VPIN_OK) wr::send_error(w, VPIN_ESHAPE, text.c_str());
      return fail(VPIN_ESHAPE, text.c_str());
    }
    const size_t slot = 1 + done, cnt = h.cnt;
    const int flags = h.flags, bits = h.shift_bits;
    const bool re = (flags & VPIN_LENET_REENCRYPT) != 0;
    snprintf(why, sizeof why, "round %zu: ", done);
    if ((rc = wr::recv_payload_timed(w, slot, h, &p))) return failed(rc, why, false);
    std::vector<uint8_t> x1(32 * cnt), y1(32 * cnt), f1(cnt), x2(32 * cnt), y2(32 * cnt), f2(cnt);
    if ((rc = wr::unpack_pair_timed(w, slot, cl->ctx, p, cnt, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data())))
      return failed(rc, why, true);
    std::vector<uint8_t> o1x, o1y, o1f, o2x, o2y, o2f;
    if (re) { o1x.resize(32 * cnt); o1y.resize(32 * cnt); o1f.resize(cnt); o2x.resize(32 * cnt); o2y.resize(32 * cnt); o2f.resize(cnt); }
    rc = vpin_net_client_round(cl, (int)done, flags, bits, x1.data(), y1.data(), f1.data(), x2.data(), y2.data(), f2.data(), cnt,
                               re ? o1x.data() : nullptr, re ? o1y.data() : nullptr, re ? o1f.data() : nullptr, re ? o2x.data() : nullptr,
                               re ? o2y.data() : nullptr, re ? o2f.data() : nullptr);
    if (rc) return failed(rc, why, true);
    const size_t n_out = cl->act[done].size();  // cnt, or the pooled count of a round that pools
    p.clear();
    if (re && (rc = wr::pack_pair_timed(w, slot, cl->ctx, o1x.data(), o1y.data(), o1f.data(), o2x.data(), o2y.data(), o2f.data(), n_out, &p)))
      return failed(rc, why, true);
    memset(&h, 0, sizeof h);
    h.type = VPIN_WIRE_REPLY; h.round = (uint32_t)done; h.cnt = re ? (uint32_t)n_out : 0; h.payload_len = re ? 64 * (uint64_t)n_out : 0;
    if ((rc = wr::send_frame_timed(w, slot, h, p.data()))) return failed(rc, why, false);
    done++;
  }
}

}  // extern "C"

// what the verifier keeps of a shape
struct DerivedShape {
  std::vector<uint8_t> comm, inputs;  // bincode(R1CSCommitment); num_inputs x 32 bytes
  size_t num_inputs = 0;
};

struct vpin_net_verifier {
  vpin_ctx* ctx = nullptr;
  std::map<std::pair<int, uint64_t>, DerivedShape> shapes;
  uint64_t stats[4] = {0, 0, 0, 0};  // shapes derived, lookups, proofs accepted, proofs rejected
  double ms[3] = {0.0, 0.0, 0.0};    // the last vpin_net_client_verify: receive, derive and compare, verify
};

namespace {

// SNARK::encode of the gadget over n_ops placeholder operations: A, B, C depend on the kind and the count alone
int derive_shape(vpin_ctx* c, int is_mult, size_t n_ops, DerivedShape* out) {
  std::vector<uint8_t> x(32 * 2 * n_ops), y(32 * 2 * n_ops);
  // 2 n distinct 64-bit multiples of G: P = the first n, R = the last n, so no R is P (a doubling) or -P (the identity)
  int rc = vpin_synthetic_points(0x7650494e, 2 * n_ops, x.data(), y.data());
  if (rc) return rc;
  vpin_dev_instance* g = nullptr;
  if (is_mult) {
    std::vector<uint8_t> w(16 * n_ops, 0);
    for (size_t i = 0; i < n_ops; i++) {
      const uint64_t v = (0x9e3779b97f4a7c15ull * (i + 1)) | 1;
      memcpy(&w[16 * i], &v, 8);
    }
    rc = vpin_gadget_point_mult_dev(c, w.data(), x.data(), y.data(), n_ops, &g);
  } else {
    const std::vector<uint8_t> rz(n_ops, 0);
    rc = vpin_gadget_point_add_dev(c, x.data(), y.data(), x.data() + 32 * n_ops, y.data() + 32 * n_ops, rz.data(), n_ops, &g);
  }
  if (rc) return rc;
  vpin_spark_decomm* d = nullptr;
  out->comm.resize(vpin_dev_instance_comm_bytes(g));
  size_t len = 0, nc = 0, nv = 0;
  rc = vpin_spark_encode_dev(c, g, &d, out->comm.data(), out->comm.size(), &len);
  if (!rc) {
    out->comm.resize(len);
    vpin_r1cs_dims(vpin_dev_instance_r1cs(g), &nc, &nv, &out->num_inputs);
    const uint8_t* in = vpin_dev_instance_inputs(g);
    if (out->num_inputs && in) out->inputs.assign(in, in + 32 * out->num_inputs);
    else out->num_inputs = 0;
  }
  vpin_spark_decomm_free(c, d);
  vpin_dev_instance_free(c, g);
  return rc;
}

int shape_of(vpin_net_verifier* v, int is_mult, size_t n_ops, const DerivedShape** out) {
  const auto key = std::make_pair(is_mult ? 1 : 0, (uint64_t)n_ops);
  auto it = v->shapes.find(key);
  if (it != v->shapes.end()) {
    v->stats[1]++;
    *out = &it->second;
    return VPIN_OK;
  }
  DerivedShape s;
  const int rc = derive_shape(v->ctx, key.first, n_ops, &s);
  if (rc) return rc;
  v->stats[0]++;
  *out = &(v->shapes[key] = std::move(s));
  return VPIN_OK;
}

}  // namespace

extern "C" {

int vpin_net_verifier_create(vpin_ctx* c, vpin_net_verifier** out) {
  if (out) *out = nullptr;
  if (!c || !out) return fail(VPIN_EINVAL, "vpin_net_verifier_create: null argument");
  vpin_net_verifier* v = new (std::nothrow) vpin_net_verifier();
  if (!v) return VPIN_ENOMEM;
  v->ctx = c;
  *out = v;
  return VPIN_OK;
}

void vpin_net_verifier_free(vpin_net_verifier* v) { delete v; }

int vpin_net_verifier_shape(vpin_net_verifier* v, int is_mult, size_t n_ops, const uint8_t** comm, size_t* comm_len, const uint8_t** inputs,
                            size_t* num_inputs) {
  if (!v || !comm || !comm_len || !inputs || !num_inputs) return fail(VPIN_EINVAL, "vpin_net_verifier_shape: null argument");
  if (!n_ops || n_ops > VPIN_PROOF_MAX_OPS) return fail(VPIN_EINVAL, "vpin_net_verifier_shape: n_ops is outside 1 .. VPIN_PROOF_MAX_OPS");
  const DerivedShape* s = nullptr;
  const int rc = shape_of(v, is_mult, n_ops, &s);
  if (rc) return rc;
  *comm = s->comm.data(); *comm_len = s->comm.size();
  *inputs = s->num_inputs ? s->inputs.data() : nullptr; *num_inputs = s->num_inputs;
  return VPIN_OK;
}

int vpin_net_verifier_stats(const vpin_net_verifier* v, uint64_t out[4]) {
  if (!v || !out) return fail(VPIN_EINVAL, "vpin_net_verifier_stats: null argument");
  for (int i = 0; i < 4; i++) out[i] = v->stats[i];
  return VPIN_OK;
}

int vpin_net_verifier_timings(const vpin_net_verifier* v, double out[3]) {
  if (!v || !out) return fail(VPIN_EINVAL, "vpin_net_verifier_timings: null argument");
  for (int i = 0; i < 3; i++) out[i] = v->ms[i];
  return VPIN_OK;
}

int vpin_net_client_verify(vpin_net_verifier* v, vpin_wire* w, size_t n_images, const vpin_proof_expect* expect, size_t n_expect,
                           const uint8_t seed32[32], uint8_t* ok_out) {
  namespace wr = vpin::wire;
  const char* who = "vpin_net_client_verify";
  if (!v || !w || !expect || !ok_out) return fail(VPIN_EINVAL, "vpin_net_client_verify: null argument");
  if (!n_images || n_images > VPIN_NET_MAX_BATCH || !n_expect || n_expect > 4096)
    return fail(VPIN_EINVAL, "vpin_net_client_verify: n_images must be in 1 .. VPIN_NET_MAX_BATCH and n_expect in 1 .. 4096");
  for (size_t k = 0; k < n_expect; k++)
    if (expect[k].is_mult > 1 || !expect[k].n_ops || expect[k].n_ops > VPIN_PROOF_MAX_OPS)
      return fail(VPIN_EINVAL, "vpin_net_client_verify: an expectation with is_mult above 1 or n_ops outside 1 .. VPIN_PROOF_MAX_OPS");
  const size_t total = n_images * n_expect;
  memset(ok_out, 0, total);
  std::vector<wr::ProofRecord> recs;
  v->ms[0] = v->ms[1] = v->ms[2] = 0.0;
  int rc = wr::recv_proofs(w, who, n_images, expect, n_expect, &recs, &v->ms[0]);
  if (rc) return rc;
  wr::Lap lap;
  // the computation commitment is the client's own: a record under another one is not looked at any further
  std::vector<vpin_verify_item> items;
  std::vector<size_t> at;
  char why[200] = "";
  for (size_t k = 0; k < total; k++) {
    const wr::ProofRecord& r = recs[k];
    const DerivedShape* s = nullptr;
    if ((rc = shape_of(v, r.h.is_mult, (size_t)r.h.n_ops, &s))) return rc;
    if (r.h.comm_len != s->comm.size() || memcmp(r.comm(), s->comm.data(), s->comm.size())) {
      if (!why[0])
        snprintf(why, sizeof why, "%s: image %u, label %u, %s: the server's commitment is not the shape's commitment", who, (unsigned)r.h.image,
                 (unsigned)r.h.label, r.h.is_mult ? "multiplications" : "additions");
      continue;
    }
    vpin_verify_item it;
    it.proof = r.proof(); it.proof_len = (size_t)r.h.proof_len;
    it.comm = s->comm.data(); it.comm_len = s->comm.size();
    it.inputs = s->num_inputs ? s->inputs.data() : nullptr; it.num_inputs = s->num_inputs;
    it.comm_para = r.comm_para(); it.comm_input = r.comm_input();
    items.push_back(it);
    at.push_back(k);
  }
  std::vector<uint8_t> ok(items.size(), 0);
  v->ms[1] = lap();
  rc = vpin_snark_verify_batch(v->ctx, items.data(), items.size(), seed32, ok.data());
  v->ms[2] = lap();
  if (rc && rc != VPIN_EVERIFY) return rc;
  size_t good = 0;
  for (size_t j = 0; j < items.size(); j++) {
    ok_out[at[j]] = ok[j] ? 1 : 0;
    good += ok[j] ? 1 : 0;
    if (!ok[j] && !why[0])
      snprintf(why, sizeof why, "%s: image %u, label %u, %s: the proof is rejected", who, (unsigned)recs[at[j]].h.image, (unsigned)recs[at[j]].h.label,
               recs[at[j]].h.is_mult ? "multiplications" : "additions");
  }
  v->stats[2] += good;
  v->stats[3] += total - good;
  return good == total ? VPIN_OK : fail(VPIN_EVERIFY, why);
}

}  // extern "C"
