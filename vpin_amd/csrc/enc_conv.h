// enc_conv.h -- device stages of the encrypted convolution layer (enc_conv.hip), driven by enc_conv.cpp
#pragma once
#include <cstddef>
#include <cstdint>

#include "ctx.h"

namespace vpin {

struct ConvGeom {
  size_t P = 1, H = 0, W = 0, fh = 0, fw = 0, pad = 0, stride = 1, oh = 0, ow = 0;
  size_t pixels() const { return P * H * W; }
  size_t outputs() const { return P * oh * ow; }
  size_t taps() const { return fh * fw; }
};

constexpr uint32_t kE2FlagRange = 1u;     // a coordinate >= q
constexpr uint32_t kE2FlagOffCurve = 2u;  // a non-identity point that does not satisfy the curve equation

// The device side of one layer.  Stages run in this order, each synchronises the context's stream before it returns:
//   load   pixels (x, y: n x 32 LE bytes; inf: n flag bytes) -> Montgomery coordinates in HBM, range and curve checks
//   conv   out[p][i][j] = sum_k w[k] * X[p][i s + ii][j s + jj] (e2_conv_kernel), normalised to affine (batched inversion);
//          the outputs stay resident for rlc and are copied to the host as canonical bytes
//   rlc    for every plane the taps() + 1 sums  sum_t r[p][t] * window[t][k]  and  sum_t r[p][t] * out[p][t]
//          (e2_rlc_kernel + e2_reduce_kernel), returned as Jacobian Montgomery triples: (P x (taps() + 1)) x 96 bytes
// msm is rlc with no taps over the loaded points themselves: one sum of n terms.
struct EncConvDev {
  vpin_ctx* c;
  ConvGeom g;
  DevBuf px, py, pinf, ox, oy, oinf, filt;
  explicit EncConvDev(vpin_ctx* ctx) : c(ctx), px(ctx), py(ctx), pinf(ctx), ox(ctx), oy(ctx), oinf(ctx), filt(ctx) {}
  int load(const uint8_t* x, const uint8_t* y, const uint8_t* inf, size_t n, uint32_t* flags);
  int conv(const ConvGeom& geom, const uint8_t* filter_le16, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf);
  int rlc(const uint8_t* r_le16, uint8_t* sums_jac);
  int msm(const uint8_t* r_le16, size_t n, uint8_t sum_jac[96]);
};

void set_last_error_text(const char* text);

}  // namespace vpin
