// infer_client.cpp -- the ready-made client of an encrypted inference, for any number of rounds: a vpin_lenet_round_fn over
// vpin_e2_client_round (what main of the reference's Client.py does between two layers) around an object that owns the key, the
// two base tables, the discrete-log table and the queue of encryption randomness, and keeps every round's values.
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"

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
