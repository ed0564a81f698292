// enc_add.cpp -- the addition layer, host side: out[p][t] = X[p][t] + R[p][t] over two encrypted tensors of the same shape, the
// skip connection of a residual block.  Input validation, the refusal of an identity first operand and the addition list; the
// additions and the scan of the first operands' flags run on the device (enc_add.hip).  The rules are those
// vpin_enc_conv2d_mc_bias settled for (C[t], bias): here the second operand is per element instead of per plane.
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/vpin_hip.h"
#include "enc_conv.h"

using namespace vpin::enc;
using vpin::E2Points;

extern "C" {

int vpin_enc_add(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, const uint8_t* rx, const uint8_t* ry,
                 const uint8_t* rinf, size_t P, size_t H, size_t W, vpin_conv_trace** out) {
  clear_refusals();
  if (out) *out = nullptr;
  if (!c || !px || !py || !pinf || !rx || !ry || !rinf || !out) return fail(VPIN_EINVAL, "vpin_enc_add: null argument");
  if (!P || !H || !W) return fail(VPIN_EINVAL, "vpin_enc_add: a dimension is zero");
  if (P > 65535) return fail(VPIN_EINVAL, ("vpin_enc_add: P = " + std::to_string(P) + " planes are more than 65535").c_str());
  if (H > kMaxDim || W > kMaxDim || H * W >= ((size_t)1 << 31) || P * H * W >= ((size_t)1 << 31))
    return fail(VPIN_EINVAL, "vpin_enc_add: a dimension is out of range");
  double* tm = reset_timings();
  Lap total, lap;
  std::unique_ptr<vpin_conv_trace> t(new (std::nothrow) vpin_conv_trace());
  if (!t) return VPIN_ENOMEM;
  const size_t per_plane = H * W, n = P * per_plane;
  t->P = P; t->oh = H; t->ow = W; t->n_add = n;

  // validate: upload, range and curve checks on the device
  E2Points x(c), r(c);
  int rc;
  if ((rc = x.load(c, px, py, pinf, n, "vpin_enc_add", "first operand"))) return rc;
  if ((rc = r.load(c, rx, ry, rinf, n, "vpin_enc_add", "second operand"))) return rc;
  tm[0] = lap();

  // the additions, and which planes hold an identity first operand
  t->out_x.resize(n * 32); t->out_y.resize(n * 32); t->out_inf.resize(n);
  std::vector<uint8_t> bad(P);
  if ((rc = vpin::e2_pair_add(c, x, r, P, per_plane, t->out_x.data(), t->out_y.data(), t->out_inf.data(), bad.data()))) return rc;
  tm[1] = lap();
  size_t first = P;
  for (size_t p = 0; p < P; p++)
    if (bad[p]) { note_refusal(p); if (first == P) first = p; }
  if (first != P) {  // the failure path: the element of the first plane named, from the caller's flags
    size_t e = 0;
    while (e + 1 < per_plane && !pinf[first * per_plane + e]) e++;
    return fail(VPIN_ESHAPE, ("vpin_enc_add: the first operand X[" + std::to_string(first) + "][" + std::to_string(e) +
                              "] is the identity (the first operand of an addition has no flag in the witness format)").c_str());
  }

  // host tail: the list (X[p][t], R[p][t], rz) from the caller's bytes; an identity R is written as zeros
  t->resize_lists();
  memcpy(t->a_px.data(), px, 32 * n); memcpy(t->a_py.data(), py, 32 * n);
#pragma omp parallel for schedule(static) num_threads(team_size())
  for (long li = 0; li < (long)n; li++) {
    const size_t i = (size_t)li;
    if (rinf[i]) {
      t->a_rz[i] = 1;  // rx, ry stay zero
    } else {
      memcpy(&t->a_rx[32 * i], rx + 32 * i, 32); memcpy(&t->a_ry[32 * i], ry + 32 * i, 32);
    }
  }
  tm[4] = lap();
  tm[5] = total();
  *out = t.release();
  return VPIN_OK;
}

}  // extern "C"
