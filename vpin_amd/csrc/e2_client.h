// e2_client.h -- the client side of vPIN's exponential ElGamal on E2, device stages (e2_client.hip) as the entry points of
// e2_client.cpp drive them.  Every stage validates its points on the device (E2Points::load: range and curve equation),
// works on the context's stream and synchronises it before it returns.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ctx.h"

// window table of one fixed base point B: entry k * (2^w - 1) + d - 1 = d * 2^(w k) * B, affine, Montgomery form
struct vpin_e2_base {
  vpin_ctx* owner = nullptr;
  int w = 0, nwin = 0;
  void *tx = nullptr, *ty = nullptr;  // device, nwin * (2^w - 1) coordinates each
};

// baby steps j * G, 0 <= j < nb: the affine x (Montgomery form) and the parity of the canonical y of every entry, and an
// open-addressing index of `slots` (a power of two >= 2 nb) 64-bit words keyed on x: 0 = empty, else (tag << 32) | j.
// Entry 0 (the identity) has no coordinates and is not in the index.
struct vpin_e2_dlog {
  vpin_ctx* owner = nullptr;
  uint64_t nb = 0, slots = 0, bytes = 0;
  void *tx = nullptr, *par = nullptr, *idx = nullptr;
  void *dmx = nullptr, *dmy = nullptr;  // l * D for l = 1 .. kDlogLanes, D = nb * G the giant step: affine, Montgomery form
};

namespace vpin {
namespace client {

constexpr int kDefaultWindow = 10;  // measured against 4, 6, 8 and 12: DESIGN.md section 9
// the walk gives a point up to this many lanes: lane l visits the giant steps l, l + L, l + 2 L, .. (strides of L * D)
constexpr int kDlogLanes = 64;

// x, y: the base point, canonical little-endian.  VPIN_EINVAL (E2Points::load) when it is not on the curve
int base_build(vpin_ctx* c, const uint8_t x[32], const uint8_t y[32], int w, vpin_e2_base** out);
void base_free(vpin_e2_base* b);
// out[i] = s_i * B (scalars: cnt x 32 bytes little-endian, already checked to be below the group order)
int base_mul(vpin_ctx* c, const vpin_e2_base* b, const uint8_t* scalars_le32, size_t cnt, uint8_t* ox, uint8_t* oy, uint8_t* oinf);
// c1[i] = r_i * G, c2[i] = (+-)m_i * G + r_i * H with m_i = |msg_i| as a 32-byte scalar and neg[i] = 1 for a negative message
int encrypt(vpin_ctx* c, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t* r_le32, const uint8_t* m_le32, const uint8_t* neg,
            size_t cnt, uint8_t* c1x, uint8_t* c1y, uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf);
// encrypt with one public key per element and no table of any H: c2[i] = (+-)m_i * G + r_i * (hx, hy)[key_of[i]], the n_pub keys
// canonical little-endian and none the identity, every key_of[i] < n_pub (both checked by the caller).  The keys go through
// E2Points::load; when it rejects one, *bad_key is the first such key's index (n_pub otherwise) and the text that key's own rule
int encrypt_keyed(vpin_ctx* c, const vpin_e2_base* g, const uint8_t* hx, const uint8_t* hy, size_t n_pub, const uint32_t* key_of,
                  const uint8_t* r_le32, const uint8_t* m_le32, const uint8_t* neg, size_t cnt, size_t* bad_key, uint8_t* c1x, uint8_t* c1y,
                  uint8_t* c1inf, uint8_t* c2x, uint8_t* c2y, uint8_t* c2inf);
// out[i] = s_i * P_i, or s_0 * P_i for every i when one_scalar
int mul256(vpin_ctx* c, const uint8_t* scalars_le32, bool one_scalar, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt,
           uint8_t* ox, uint8_t* oy, uint8_t* oinf);
int dlog_build(vpin_ctx* c, uint64_t nb, vpin_e2_dlog** out);
void dlog_free(vpin_e2_dlog* t);
int dlog_solve(vpin_ctx* c, const vpin_e2_dlog* t, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt, uint64_t max_giant,
               int64_t* v_out, uint8_t* found_out);
int decrypt(vpin_ctx* c, const vpin_e2_dlog* t, const uint8_t sk_le32[32], const uint8_t* c1x, const uint8_t* c1y, const uint8_t* c1inf,
            const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt, uint64_t max_giant, int64_t* v_out,
            uint8_t* found_out);
// One round of the client between two layers as one launch chain: decrypt (as above), the activation (ReLU when relu, then
// the reference's float32 `shifting` when shift_bits != 0) and, when r_le32 is not null, the encryption of the activated values
// under r.  v_out: the raw decryptions; act_out: the activated values; bad_out: per element 0, or bit 0 = no value in the
// walk's range, bit 1 = the activated value does not fit (int32 after a shift, |.| < 2^62 otherwise)
int round(vpin_ctx* c, const vpin_e2_dlog* t, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t sk_le32[32], const uint8_t* c1x,
          const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, size_t cnt,
          uint64_t max_giant, bool relu, int shift_bits, const uint8_t* r_le32, int64_t* v_out, int64_t* act_out, uint8_t* bad_out,
          uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf);
// the input of a round that pools: planes x H x W values, windows of k x k at a stride; a remainder of rows or columns is dropped
struct PoolShape {
  size_t planes, H, W, k, stride;
  size_t Ho() const { return (H - k) / stride + 1; }
  size_t Wo() const { return (W - k) / stride + 1; }
};
// round over pool.planes * H * W elements with the maximum of every window in front of the activation (e2_act_pool_kernel): act_out,
// bad_out and the ciphertexts have planes * Ho * Wo elements, r_le32 as many scalars.  bad_out bit 0: an element of that window
// has no value; found_out (cnt bytes) is then, and only then, read back from the walk
int round_pool(vpin_ctx* c, const vpin_e2_dlog* t, const vpin_e2_base* g, const vpin_e2_base* h, const uint8_t sk_le32[32], const uint8_t* c1x,
               const uint8_t* c1y, const uint8_t* c1inf, const uint8_t* c2x, const uint8_t* c2y, const uint8_t* c2inf, const PoolShape& pool,
               uint64_t max_giant, bool relu, int shift_bits, const uint8_t* r_le32, int64_t* v_out, int64_t* act_out, uint8_t* bad_out,
               uint8_t* found_out, uint8_t* o1x, uint8_t* o1y, uint8_t* o1inf, uint8_t* o2x, uint8_t* o2y, uint8_t* o2inf);

}  // namespace client
}  // namespace vpin
