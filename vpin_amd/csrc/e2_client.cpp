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
  if (!c || !t || !sk_le32 || !c1x || !c1y || !c1inf || !c2x || !c2y || !c2inf || !v_out || !act_out)
    return fail(VPIN_EINVAL, "vpin_e2_client_round: null argument");
  if (reencrypt && (!baseG || !baseH || !r_le32 || !o1x || !o1y || !o1inf || !o2x || !o2y || !o2inf))
    return fail(VPIN_EINVAL, "vpin_e2_client_round: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 30)) return fail(VPIN_EINVAL, "vpin_e2_client_round: cnt must be in 1 .. 2^30 - 1");
  if (shift_bits < 0 || shift_bits > 62) return fail(VPIN_EINVAL, "vpin_e2_client_round: shift_bits must be 0 (no shifting) or in 1 .. 62");
  if (!walk_fits(max_giant, t->nb)) return fail(VPIN_EINVAL, "vpin_e2_client_round: max_giant * nb is past 2^62");
  switch (check_scalars(sk_le32, 1, true)) {
    case 1: return fail(VPIN_EINVAL, "vpin_e2_client_round: the key sk is not below the group order");
    case 2: return fail(VPIN_EINVAL, "vpin_e2_client_round: the key sk is zero");
  }
  if (reencrypt) switch (check_scalars(r_le32, cnt, true)) {
    case 1: return fail(VPIN_EINVAL, "vpin_e2_client_round: a randomness r is not below the group order");
    case 2: return fail(VPIN_EINVAL, "vpin_e2_client_round: a randomness r is zero");
  }
  std::vector<uint8_t> bad(cnt, 0);
  const int rc = cl::round(c, t, baseG, baseH, sk_le32, c1x, c1y, c1inf, c2x, c2y, c2inf, cnt, max_giant, relu != 0, shift_bits,
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

}  // extern "C"
