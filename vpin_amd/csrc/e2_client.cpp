// e2_client.cpp -- the client side of vPIN's exponential ElGamal on E2 behind the C ABI: input validation and the handles of
// the two device-resident tables.  The arithmetic runs on the device (e2_client.hip).  Restates the key generation, `encrypt`
// and `decrypt` / `bsgs` of the reference's src/LeNet/Client.py with the randomness and the key as explicit inputs, and
// with the baby-step table built on the device instead of read from a pickle.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vpin_hip.h"
#include "e2_client.h"
#include "enc_conv.h"

using vpin::enc::fail;
namespace cl = vpin::client;

namespace {

// the order n of E2's group (prime, 252 bits), little-endian
const uint8_t kOrder[32] = {0xdd, 0x85, 0xee, 0xdf, 0xec, 0xb0, 0x05, 0x88, 0x99, 0x55, 0xcc, 0xc4, 0x7e, 0x1a, 0x40, 0xa2,
                            0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x0f};

bool below_order(const uint8_t* s) {
  for (int i = 31; i >= 0; i--)
    if (s[i] != kOrder[i]) return s[i] < kOrder[i];
  return false;
}

bool is_zero32(const uint8_t* s) {
  uint8_t o = 0;
  for (int i = 0; i < 32; i++) o |= s[i];
  return o == 0;
}

// 0: every scalar is in range; 1: one is >= n; 2: one is zero although nonzero is asked for
int check_scalars(const uint8_t* s, size_t cnt, bool nonzero) {
  for (size_t i = 0; i < cnt; i++) {
    if (!below_order(s + 32 * i)) return 1;
    if (nonzero && is_zero32(s + 32 * i)) return 2;
  }
  return 0;
}

// max_giant * nb <= 2^62, so that every value of the walk fits an int64
bool walk_fits(uint64_t max_giant, uint64_t nb) {
  return (unsigned __int128)max_giant * nb <= ((unsigned __int128)1 << 62);
}

// the messages as the device takes them: the magnitude as a 32-byte scalar and a sign byte.  false when one is 2^62 or more
bool split_messages(const int64_t* msgs, size_t cnt, std::vector<uint8_t>* m, std::vector<uint8_t>* neg) {
  m->assign(cnt * 32, 0);
  neg->assign(cnt, 0);
  for (size_t i = 0; i < cnt; i++) {
    const uint64_t mag = msgs[i] < 0 ? 0 - (uint64_t)msgs[i] : (uint64_t)msgs[i];
    if (mag >= ((uint64_t)1 << 62)) return false;
    memcpy(&(*m)[32 * i], &mag, 8);
    (*neg)[i] = msgs[i] < 0 ? 1 : 0;
  }
  return true;
}

// what vpin_e2_client_round and vpin_e2_client_round_pool reject alike, behind the entry point's name.  n_r: the scalars of r_le32
int round_nulls(const char* who, const void* c, const void* t, const void* baseG, const void* baseH, const void* sk, const void* c1x, const void* c1y,
                const void* c1inf, const void* c2x, const void* c2y, const void* c2inf, int reencrypt, const void* r, const void* v_out,
                const void* act_out, const void* o1x, const void* o1y, const void* o1inf, const void* o2x, const void* o2y, const void* o2inf) {
  if (!c || !t || !sk || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || !v_out || !act_out ||
      (reencrypt && (!baseG || !baseH || !r || !o1x || !o1y || !o1inf || !o2x || !o2y || !o2inf)))
    return fail(VPIN_EINVAL, (std::string(who) + ": null argument").c_str());
  return VPIN_OK;
}

int round_rules(const char* who, const vpin_e2_dlog* t, const uint8_t* sk_le32, uint64_t max_giant, int shift_bits, const uint8_t* r_le32, size_t n_r) {
  const std::string name = std::string(who) + ": ";
  if (shift_bits < 0 || shift_bits > 62) return fail(VPIN_EINVAL, (name + "shift_bits must be 0 (no shifting) or in 1 .. 62").c_str());
  if (!walk_fits(max_giant, t->nb)) return fail(VPIN_EINVAL, (name + "max_giant * nb is past 2^62").c_str());
  switch (check_scalars(sk_le32, 1, true)) {
    case 1: return fail(VPIN_EINVAL, (name + "the key sk is not below the group order").c_str());
    case 2: return fail(VPIN_EINVAL, (name + "the key sk is zero").c_str());
  }
  if (r_le32) switch (check_scalars(r_le32, n_r, true)) {
    case 1: return fail(VPIN_EINVAL, (name + "a randomness r is not below the group order").c_str());
    case 2: return fail(VPIN_EINVAL, (name + "a randomness r is zero").c_str());
  }
  return VPIN_OK;
}

}  // namespace

extern "C" {

int vpin_e2_base_create_w(vpin_ctx* c, const uint8_t* x, const uint8_t* y, int w, vpin_e2_base** out) {
  if (out) *out = nullptr;
  if (!c || !out || (x == nullptr) != (y == nullptr)) return fail(VPIN_EINVAL, "vpin_e2_base_create: null argument");
  if (w < 4 || w > 12) return fail(VPIN_EINVAL, "vpin_e2_base_create: the window width must be in 4 .. 12");
  if (x && is_zero32(x) && is_zero32(y)) return fail(VPIN_EINVAL, "vpin_e2_base_create: the base point is the identity");
  return cl::base_build(c, x, y, w, out);
}

int vpin_e2_base_create(vpin_ctx* c, const uint8_t* x, const uint8_t* y, vpin_e2_base** out) {
  return vpin_e2_base_create_w(c, x, y, cl::kDefaultWindow, out);
}

void vpin_e2_base_free(vpin_e2_base* b) { cl::base_free(b); }

int vpin_e2_base_mul(vpin_ctx* c, const vpin_e2_base* b, const uint8_t* scalars_le32, size_t cnt, uint8_t* out_x, uint8_t* out_y,
                     uint8_t* out_inf) {
  if (!c || !b || !scalars_le32 || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_base_mul: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 31)) return fail(VPIN_EINVAL, "vpin_e2_base_mul: cnt must be in 1 .. 2^31 - 1");
  if (check_scalars(scalars_le32, cnt, false)) return fail(VPIN_EINVAL, "vpin_e2_base_mul: a scalar is not below the group order");
  return cl::base_mul(c, b, scalars_le32, cnt, out_x, out_y, out_inf);
}

int vpin_e2_mul256(vpin_ctx* c, const uint8_t* scalars_le32, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt,
                   uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  if (!c || !scalars_le32 || !px || !py || !pinf || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_mul256: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 31)) return fail(VPIN_EINVAL, "vpin_e2_mul256: cnt must be in 1 .. 2^31 - 1");
  if (check_scalars(scalars_le32, cnt, false)) return fail(VPIN_EINVAL, "vpin_e2_mul256: a scalar is not below the group order");
  return cl::mul256(c, scalars_le32, false, px, py, pinf, cnt, out_x, out_y, out_inf);
}

int vpin_e2_encrypt(vpin_ctx* c, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const int64_t* msgs, const uint8_t* r_le32, size_t cnt,
                    uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf) {
  if (!c || !baseG || !baseH || !msgs || !r_le32 || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf)
    return fail(VPIN_EINVAL, "vpin_e2_encrypt: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 30)) return fail(VPIN_EINVAL, "vpin_e2_encrypt: cnt must be in 1 .. 2^30 - 1");
  switch (check_scalars(r_le32, cnt, true)) {
    case 1: return fail(VPIN_EINVAL, "vpin_e2_encrypt: a randomness r is not below the group order");
    case 2: return fail(VPIN_EINVAL, "vpin_e2_encrypt: a randomness r is zero");
  }
  std::vector<uint8_t> m, neg;
  if (!split_messages(msgs, cnt, &m, &neg)) return fail(VPIN_EINVAL, "vpin_e2_encrypt: a message is not in -(2^62) < msg < 2^62");
  return cl::encrypt(c, baseG, baseH, r_le32, m.data(), neg.data(), cnt, c1x, c1y, c1inf, c2x, c2y, c2inf);
}

int vpin_e2_encrypt_keyed(vpin_ctx* c, const vpin_e2_base* baseG, const uint8_t* hx, const uint8_t* hy, size_t n_pub, const uint32_t* key_of,
                          const int64_t* msgs, const uint8_t* r_le32, size_t cnt, uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x,
                          uint8_t* c2y, uint8_t* c2inf) {
  if (!c || !baseG || !hx || !hy || !key_of || !msgs || !r_le32 || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf)
    return fail(VPIN_EINVAL, "vpin_e2_encrypt_keyed: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 30)) return fail(VPIN_EINVAL, "vpin_e2_encrypt_keyed: cnt must be in 1 .. 2^30 - 1");
  if (n_pub == 0 || n_pub >= ((size_t)1 << 30)) return fail(VPIN_EINVAL, "vpin_e2_encrypt_keyed: n_pub must be in 1 .. 2^30 - 1");
  char why[160];
  for (size_t i = 0; i < cnt; i++)
    if (key_of[i] >= n_pub) {
      snprintf(why, sizeof why, "vpin_e2_encrypt_keyed: key_of[%zu] = %u is not below n_pub = %zu", i, (unsigned)key_of[i], n_pub);
      return fail(VPIN_EINVAL, why);
    }
  for (size_t k = 0; k < n_pub; k++)
    if (is_zero32(hx + 32 * k) && is_zero32(hy + 32 * k)) {
      snprintf(why, sizeof why, "vpin_e2_encrypt_keyed: public key %zu is the identity", k);
      return fail(VPIN_EINVAL, why);
    }
  switch (check_scalars(r_le32, cnt, true)) {
    case 1: return fail(VPIN_EINVAL, "vpin_e2_encrypt_keyed: a randomness r is not below the group order");
    case 2: return fail(VPIN_EINVAL, "vpin_e2_encrypt_keyed: a randomness r is zero");
  }
  std::vector<uint8_t> m, neg;
  if (!split_messages(msgs, cnt, &m, &neg)) return fail(VPIN_EINVAL, "vpin_e2_encrypt_keyed: a message is not in -(2^62) < msg < 2^62");
  size_t bad_key = n_pub;
  const int rc = cl::encrypt_keyed(c, baseG, hx, hy, n_pub, key_of, r_le32, m.data(), neg.data(), cnt, &bad_key, c1x, c1y, c1inf, c2x, c2y, c2inf);
  if (rc == VPIN_EINVAL && bad_key < n_pub) {  // "vpin_e2_encrypt_keyed: <rule>" with the key's index behind it
    const std::string text = std::string(vpin_last_error()) + " (public key " + std::to_string(bad_key) + ")";
    return fail(rc, text.c_str());
  }
  return rc;
}

int vpin_e2_dlog_create(vpin_ctx* c, uint64_t nb, vpin_e2_dlog** out) {
  if (out) *out = nullptr;
  if (!c || !out) return fail(VPIN_EINVAL, "vpin_e2_dlog_create: null argument");
  if (nb < 2 || nb > ((uint64_t)1 << 28)) return fail(VPIN_EINVAL, "vpin_e2_dlog_create: nb must be in 2 .. 2^28");
  return cl::dlog_build(c, nb, out);
}

void vpin_e2_dlog_free(vpin_e2_dlog* t) { cl::dlog_free(t); }

int vpin_e2_dlog_info(const vpin_e2_dlog* t, uint64_t out[2]) {
  if (!t || !out) return fail(VPIN_EINVAL, "vpin_e2_dlog_info: null argument");
  out[0] = t->nb;
  out[1] = t->bytes;
  return VPIN_OK;
}

int vpin_e2_dlog_solve(vpin_ctx* c, const vpin_e2_dlog* t, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt,
                       uint64_t max_giant, int64_t* v_out, uint8_t* found_out) {
  if (!c || !t || !px || !py || !pinf || !v_out || !found_out) return fail(VPIN_EINVAL, "vpin_e2_dlog_solve: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 31)) return fail(VPIN_EINVAL, "vpin_e2_dlog_solve: cnt must be in 1 .. 2^31 - 1");
  if (!walk_fits(max_giant, t->nb)) return fail(VPIN_EINVAL, "vpin_e2_dlog_solve: max_giant * nb is past 2^62");
  return cl::dlog_solve(c, t, px, py, pinf, cnt, max_giant, v_out, found_out);
}

int vpin_e2_decrypt(vpin_ctx* c, const vpin_e2_dlog* t, const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
                    const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint64_t max_giant, int64_t* v_out,
                    uint8_t* found_out) {
  if (!c || !t || !sk_le32 || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || !v_out || !found_out)
    return fail(VPIN_EINVAL, "vpin_e2_decrypt: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 31)) return fail(VPIN_EINVAL, "vpin_e2_decrypt: cnt must be in 1 .. 2^31 - 1");
  if (!walk_fits(max_giant, t->nb)) return fail(VPIN_EINVAL, "vpin_e2_decrypt: max_giant * nb is past 2^62");
  switch (check_scalars(sk_le32, 1, true)) {
    case 1: return fail(VPIN_EINVAL, "vpin_e2_decrypt: the key sk is not below the group order");
    case 2: return fail(VPIN_EINVAL, "vpin_e2_decrypt: the key sk is zero");
  }
  return cl::decrypt(c, t, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, max_giant, v_out, found_out);
}

int vpin_e2_client_round(vpin_ctx* c, const vpin_e2_dlog* t, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const uint8_t sk_le32[32],
                         const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y,
                         const uint8_t* c2inf, size_t cnt, uint64_t max_giant, int relu, int shift_bits, int reencrypt, const uint8_t* r_le32,
                         int64_t* v_out, int64_t* act_out, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y,
                         uint8_t* o2inf) {
  const char* who = "vpin_e2_client_round";
  int rc = round_nulls(who, c, t, baseG, baseH, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, reencrypt, r_le32, v_out, act_out, o1x, o1y, o1inf, o2x,
                       o2y, o2inf);
  if (rc) return rc;
  if (cnt == 0 || cnt >= ((size_t)1 << 30)) return fail(VPIN_EINVAL, "vpin_e2_client_round: cnt must be in 1 .. 2^30 - 1");
  if ((rc = round_rules(who, t, sk_le32, max_giant, shift_bits, reencrypt ? r_le32 : nullptr, cnt))) return rc;
  std::vector<uint8_t> bad(cnt, 0);
  rc = cl::round(c, t, baseG, baseH, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, max_giant, relu != 0, shift_bits,
                 reencrypt ? r_le32 : nullptr, v_out, act_out, bad.data(), o1x, o1y, o1inf, o2x, o2y, o2inf);
  if (rc) return rc;
  for (size_t i = 0; i < cnt; i++) {
    if (!bad[i]) continue;
    char why[160];
    if (bad[i] & 1)
      snprintf(why, sizeof why, "vpin_e2_client_round: element %zu has no value within the walk's range", i);
    else
      snprintf(why, sizeof why, "vpin_e2_client_round: the activated value of element %zu (decrypted %lld) does not fit", i, (long long)v_out[i]);
    return fail(VPIN_ESHAPE, why);
  }
  return VPIN_OK;
}

int vpin_e2_client_round_pool(vpin_ctx* c, const vpin_e2_dlog* t, const vpin_e2_base* baseG, const vpin_e2_base* baseH, const uint8_t sk_le32[32],
                              const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y,
                              const uint8_t* c2inf, size_t planes, size_t H, size_t W, size_t k, size_t stride, uint64_t max_giant, int relu,
                              int shift_bits, int reencrypt, const uint8_t* r_le32, int64_t* v_out, int64_t* act_out, uint8_t* o1x, uint8_t* o1y,
                              uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf) {
  const char* who = "vpin_e2_client_round_pool";
  int rc = round_nulls(who, c, t, baseG, baseH, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, reencrypt, r_le32, v_out, act_out, o1x, o1y, o1inf, o2x,
                       o2y, o2inf);
  if (rc) return rc;
  if (!planes || !H || !W) return fail(VPIN_EINVAL, "vpin_e2_client_round_pool: planes, H or W is zero");
  if (!k || !stride) return fail(VPIN_EINVAL, "vpin_e2_client_round_pool: the window k or the stride is zero");
  if (k > H || k > W) return fail(VPIN_EINVAL, "vpin_e2_client_round_pool: the window k does not fit the H x W plane");
  if ((unsigned __int128)planes * H * W >= ((unsigned __int128)1 << 30) || planes >= ((size_t)1 << 30) || H >= ((size_t)1 << 30) ||
      W >= ((size_t)1 << 30))
    return fail(VPIN_EINVAL, "vpin_e2_client_round_pool: planes * H * W must be in 1 .. 2^30 - 1");
  const cl::PoolShape pool{planes, H, W, k, stride};
  const size_t cnt = planes * H * W, Ho = pool.Ho(), Wo = pool.Wo(), n_out = planes * Ho * Wo;
  if ((rc = round_rules(who, t, sk_le32, max_giant, shift_bits, reencrypt ? r_le32 : nullptr, n_out))) return rc;
  std::vector<uint8_t> bad(n_out, 0), found(cnt, 1);
  rc = cl::round_pool(c, t, baseG, baseH, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, pool, max_giant, relu != 0, shift_bits,
                      reencrypt ? r_le32 : nullptr, v_out, act_out, bad.data(), found.data(), o1x, o1y, o1inf, o2x, o2y, o2inf);
  if (rc) return rc;
  char why[200];
  // the maximum needs every value of its window: the first input element inside a window that has none, before any value's fit
  for (size_t i = 0; i < cnt; i++) {
    if (found[i]) continue;
    const size_t y = i % (H * W) / W, x = i % W;
    const size_t oy = y / stride < Ho ? y / stride : Ho - 1, ox = x / stride < Wo ? x / stride : Wo - 1;
    if (y - oy * stride >= k || x - ox * stride >= k) continue;  // in no window: a dropped remainder, or a gap of stride > k
    snprintf(why, sizeof why, "vpin_e2_client_round_pool: element %zu, inside a window, has no value within the walk's range", i);
    return fail(VPIN_ESHAPE, why);
  }
  for (size_t o = 0; o < n_out; o++) {
    if (!bad[o]) continue;
    const size_t p = o / (Ho * Wo), at = p * H * W + (o % (Ho * Wo) / Wo) * stride * W + (o % Wo) * stride;
    long long a = v_out[at];
    for (size_t i = 0; i < k; i++)
      for (size_t j = 0; j < k; j++) a = v_out[at + i * W + j] > a ? v_out[at + i * W + j] : a;
    snprintf(why, sizeof why, "vpin_e2_client_round_pool: the activated value of output element %zu (the maximum decrypted, %lld) does not fit", o, a);
    return fail(VPIN_ESHAPE, why);
  }
  return VPIN_OK;
}

}  // extern "C"
