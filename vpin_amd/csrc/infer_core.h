// infer_core.h -- the one server loop behind vpin_lenet_infer and vpin_net_infer (infer_core.cpp): a list of steps over the
// server's (c1, c2) planes, each a layer call with the client's round after it.  Internal: the two entry points translate their
// configuration into steps and keep their own trace types around the Result.
#pragma once
#include <string>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"
#include "infer_slots.h"

namespace vpin::infer {

// vpin_net_infer_isolated: an image that makes a layer refuse, whose point a layer's load refuses or that the round callback
// drops leaves the batch with its status written, and the step runs again over the others (infer_core.cpp, run)
struct Isolation {
  vpin_net_image_status* status = nullptr;        // [B]
  uint64_t refused = 0, dropped = 0, repeats = 0;  // images a layer refused, images dropped in a round, layer calls repeated
};

struct Step {
  enum Kind { kConv, kPool, kFc, kConvMc, kFcs, kAdd } kind = kConv;
  // what the step reads, as vpin_net_layer says it: 0 the previous step's output (skip_from: none), k the output of step k - 1
  // after its round, kFromInput the encrypted input.  kAdd: vpin_enc_add over the 2 C planes, kBlocked, the second operand the
  // tensor skip_from names.  run() keeps, as host Pts pairs, exactly the tensors a later step names, each until its last use
  static constexpr size_t kFromInput = (size_t)-1;
  size_t input_from = 0, skip_from = 0;
  // how c1 and c2 make up the layer call's P = 2 C planes, and how its output splits back: all c1 planes and then all c2 planes
  // (first half, second half), or (0, c1), (0, c2), (1, c1), .. (even planes, odd planes).  For kFc and kFcs, P = 2, they coincide
  enum Order { kBlocked, kInterleaved } order = kBlocked;
  const uint8_t* filter_le16 = nullptr;  // kConv
  size_t fh = 0, fw = 0, pad = 0;
  size_t stride = 1;                     // kConv and kPool
  size_t k = 0;                          // kPool
  const uint8_t* scale_le16 = nullptr;
  size_t K = 0, N = 0;                   // kFc, and kFcs: vpin_enc_fc_signed, w signed
  const int32_t* w = nullptr;
  const int64_t* bias = nullptr;         // kFc, kFcs: N values; kConvMc: NULL or n_out values (vpin_enc_conv2d_mc_bias)
  size_t n_out = 0;                      // kConvMc (with fh, fw, pad, stride): vpin_enc_conv2d_mc with groups = 2, kBlocked
  const int32_t* w_mc = nullptr;
  const uint8_t* connect = nullptr;
  // before the call: vpin_e2_plane_sums_batch by this table on every image's c1 and c2 (sum_out planes each), when there is one ..
  const uint8_t* sum_table = nullptr;
  size_t sum_out = 0;
  size_t repeat = 1;  // .. and then the planes handed to the call this many times over
  size_t keys = 0;    // PRF keys the call consumes
  std::string name;   // in error texts: "<who>: <name>: .."
  // the client's round after the call
  bool has_round = false;
  int round = 0, relu = 0, shift_bits = 0, reencrypt = 1;
  size_t round_pool_k = 0, round_pool_stride = 0;  // both non-zero: the client pools by maximum inside the round (VPIN_LENET_MAXPOOL)
  std::string round_name;
};

// what both entry points are given, and the input's shape.  B images go through every step in ONE layer call and every round in
// ONE callback: c1 and c2 hold [b][C][H][W], a layer call's planes are [b] of what Step::Order says for one image, keys32 and
// bias_r_le32 are image-major (n_keys, n_bias_r: B times what the steps consume), and each step is handed its keys and bias r of
// all images, image after image; the sums of a step with a sum_table are one call over the groups [b][half]
struct Call {
  vpin_ctx* c;
  const char* who;  // the entry point's name, in front of every error text
  int prf_bytes;
  size_t C, H, W;
  const uint8_t *c1x, *c1y, *c1inf, *c2x, *c2y, *c2inf;
  const vpin_e2_base *baseG, *baseH;
  const uint8_t* keys32;
  size_t n_keys;
  const uint8_t* bias_r_le32;
  size_t n_bias_r;
  vpin_lenet_round_fn round_fn;
  void* user;
  size_t B = 1;  // the images; behind everything a caller of one image names
  // the images of several clients: n_pub public keys (canonical little-endian, n_pub x 32 bytes each) and per image the index
  // of its client's.  n_pub = 0: every image is under baseH's key.  Otherwise baseH is not read and the bias of image b is
  // encrypted under key key_of_image[b] (vpin_e2_encrypt_keyed)
  const uint8_t *hx = nullptr, *hy = nullptr;
  size_t n_pub = 0;
  const uint32_t* key_of_image = nullptr;
  Isolation* iso = nullptr;  // NULL: a refusal fails the whole batch
};

// per step the trace of its layer call, owned, and the slots of the images in that call (0 .. B - 1 unless images left);
// host-clock milliseconds per step (plane sums included), per round (0: none) and in all
struct Result {
  std::vector<vpin_conv_trace*> step;
  std::vector<std::vector<uint32_t>> slots;
  std::vector<uint32_t> survivors;  // the slots still there after the last round
  std::vector<double> step_ms, round_ms;
  double total_ms = 0.0;
  Result() = default;
  Result(const Result&) = delete;
  Result& operator=(const Result&) = delete;
  ~Result() {
    for (vpin_conv_trace* t : step) vpin_conv_trace_free(t);
  }
};

// VPIN_EINVAL when n_keys or n_bias_r is not B times what the steps consume, or an array they need is NULL; a failing step or round
// returns its code behind "<who>: <name>: ".  The timings are filled as far as the run got; the caller drops `out` on failure
int run(const Call& call, const std::vector<Step>& steps, Result* out);

bool any_negative(const int32_t* w, size_t n);

}  // namespace vpin::infer
