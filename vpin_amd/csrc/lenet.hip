// lenet.hip -- what the LeNet server loop needs on the device beyond the layers of enc_conv.hip and enc_fc.hip: the channel
// sums in front of the second and third convolution (secondConv / thirdConv of the reference's src/LeNet/Server.py add whole
// ciphertext planes pixel by pixel, np.sum(.., axis=0), the second by LeNet's connection table, the third over all planes).
//
//   e2_plane_sum_kernel  one lane per (output plane, pixel): a Jacobian accumulator over the connected input planes with the
//                        mixed addition, complete by case (e2_dev.h): an identity pixel is skipped, the same point in two planes
//                        falls to the doubling, P and -P cancel to the identity
// E2Points::load (e2_load_kernel: range and curve checks) comes before it and e2_emit (e2_to_affine_kernel) after it, both of
// enc_conv.hip.  The plane
// additions are not part of any witness list: the reference does not prove them.
#include "e2_dev.h"
#include "enc_conv.h"

#include "../../include/vpin_hip.h"

namespace vpin {

namespace {

// X, Y, inf: n_in planes of hw pixels; connect: n_out x n_in bytes; out: n_out planes of hw sums
__global__ __launch_bounds__(kE2Block) void e2_plane_sum_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                                const uint8_t* __restrict__ inf, size_t n_in, size_t hw,
                                                                const uint8_t* __restrict__ connect, size_t n_out, fq a,
                                                                e2_jac* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n_out * hw) return;
  const size_t o = i / hw, p = i % hw;
  e2_jac acc = e2_identity();
  for (size_t j = 0; j < n_in; j++) {
    if (!connect[o * n_in + j]) continue;  // the same for every lane of a plane
    const size_t idx = j * hw + p;
    if (inf[idx]) continue;
    acc = e2_add_mixed(acc, fq_load(X + idx), fq_load(Y + idx), a);
  }
  e2_store(out + i, acc);
}

int plane_sums(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t n_in, size_t hw, const uint8_t* connect,
               size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  (void)hipSetDevice(c->device);
  E2Points pts(c);
  const int rc = pts.load(c, px, py, pinf, n_in * hw, "vpin_e2_plane_sums", "pixel");
  if (rc) return rc;
  const size_t n = n_out * hw;
  DevBuf con(c), jac(c);
  if (con.alloc(n_out * n_in) || jac.alloc(n * sizeof(e2_jac))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(con.p, connect, n_out * n_in, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_plane_sum_kernel, dim3(blocks_of(n, kE2Block)), dim3(kE2Block), 0, c->stream, pts.X(), pts.Y(), pts.F(), n_in, hw,
                     (const uint8_t*)con.p, n_out, e2_curve_a(), (e2_jac*)jac.p);
  VPIN_HIP_TRY(hipGetLastError());
  return e2_emit(c, (const e2_jac*)jac.p, n, out_x, out_y, out_inf);
}

}  // namespace

}  // namespace vpin

using vpin::enc::fail;

extern "C" int vpin_e2_plane_sums(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t n_in, size_t H, size_t W,
                                  const uint8_t* connect, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  if (!c || !px || !py || !pinf || !connect || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_plane_sums: null argument");
  if (!n_in || !H || !W || !n_out) return fail(VPIN_EINVAL, "vpin_e2_plane_sums: a dimension is zero");
  if (n_in > 65535 || n_out > 65535 || H > vpin::enc::kMaxDim || W > vpin::enc::kMaxDim || H * W * (n_in > n_out ? n_in : n_out) >= ((size_t)1 << 31))
    return fail(VPIN_EINVAL, "vpin_e2_plane_sums: a dimension is out of range");
  for (size_t o = 0; o < n_out; o++) {
    bool any = false;
    for (size_t j = 0; j < n_in; j++) any = any || connect[o * n_in + j] != 0;
    if (!any) return fail(VPIN_EINVAL, "vpin_e2_plane_sums: a row of the connection table selects no plane");
  }
  return vpin::plane_sums(c, px, py, pinf, n_in, H * W, connect, n_out, out_x, out_y, out_inf);
}
