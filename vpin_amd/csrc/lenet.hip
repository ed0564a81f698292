// lenet.hip -- what the LeNet server loop needs on the device beyond the layers of enc_conv.hip and enc_fc.hip: the channel
// sums in front of the second and third convolution (secondConv / thirdConv of the reference's src/LeNet/Server.py add whole
// ciphertext planes pixel by pixel, np.sum(.., axis=0), the second by LeNet's connection table, the third over all planes).
//
//   e2_plane_sums_batch_kernel  groups x n_out output planes (a batch hands its 2 B halves as the groups; vpin_e2_plane_sums is
//                        the call of one group), one lane per output pixel, a workgroup inside one output plane of one group:
//                        a Jacobian accumulator over the connected input planes of that group with the mixed addition,
//                        complete by case (e2_dev.h): an identity pixel is skipped, the same point in two planes falls to the
//                        doubling, P and -P cancel to the identity.  No LDS, no scratch
// E2Points::load (e2_load_kernel: range and curve checks) comes before it and e2_emit (e2_to_affine_kernel) after it, both of
// enc_conv.hip.  The plane additions are not part of any witness list: the reference does not prove them.
#include <string>

#include "e2_dev.h"
#include "enc_conv.h"

#include "../../include/vpin_hip.h"

namespace vpin {

namespace {

// X, Y, inf: groups x n_in planes of hw pixels, group-major; connect: n_out x n_in bytes; out: groups x n_out planes of hw sums.
// blockIdx: x a block of pixels, y the output plane o (n_out = gridDim.y), z the group.  o and the group are the workgroup's, so
// the walk over row o of connect is the same for every lane and only flagged pixels make lanes differ
__global__ __launch_bounds__(kE2Block) void e2_plane_sums_batch_kernel(const fq* __restrict__ X, const fq* __restrict__ Y,
                                                                       const uint8_t* __restrict__ inf, uint32_t n_in, uint32_t hw,
                                                                       const uint8_t* __restrict__ connect, fq a,
                                                                       e2_jac* __restrict__ out) {
  const uint32_t p = blockIdx.x * kE2Block + threadIdx.x;
  if (p >= hw) return;
  const uint8_t* row = connect + (size_t)blockIdx.y * n_in;
  const size_t in0 = (size_t)blockIdx.z * n_in * hw + p;  // below 2^31 with every plane of every group (checked by the caller)
  e2_jac acc = e2_identity();
  for (uint32_t j = 0; j < n_in; j++) {
    if (!row[j]) continue;
    const size_t idx = in0 + (size_t)j * hw;
    if (inf[idx]) continue;
    acc = e2_add_mixed(acc, fq_load(X + idx), fq_load(Y + idx), a);
  }
  e2_store(out + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * hw + p, acc);
}

// both entry points behind their checks: one load, one launch, one e2_emit
int plane_sums(vpin_ctx* c, const char* who, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t n_in, size_t hw,
               const uint8_t* connect, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  (void)hipSetDevice(c->device);
  E2Points pts(c);
  const int rc = pts.load(c, px, py, pinf, groups * n_in * hw, who, "pixel");
  if (rc) return rc;
  const size_t n = groups * n_out * hw;
  DevBuf con(c), jac(c);
  if (con.alloc(n_out * n_in) || jac.alloc(n * sizeof(e2_jac))) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(con.p, connect, n_out * n_in, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_plane_sums_batch_kernel, dim3(blocks_of(hw, kE2Block), (unsigned)n_out, (unsigned)groups), dim3(kE2Block), 0, c->stream,
                     pts.X(), pts.Y(), pts.F(), (uint32_t)n_in, (uint32_t)hw, (const uint8_t*)con.p, e2_curve_a(), (e2_jac*)jac.p);
  VPIN_HIP_TRY(hipGetLastError());
  return e2_emit(c, (const e2_jac*)jac.p, n, out_x, out_y, out_inf);
}

// VPIN_EINVAL with a text before anything is uploaded: the dimensions are grid axes and the point counts ints
int check_sums(const std::string& who, size_t groups, size_t n_in, size_t H, size_t W, const uint8_t* connect, size_t n_out) {
  if (!groups || !n_in || !H || !W || !n_out) return enc::fail(VPIN_EINVAL, (who + ": a dimension is zero").c_str());
  const size_t lim = (size_t)1 << 31;
  const auto range = [&] {  // a product is formed once the one before it is below 2^31: none wraps
    if (groups > 65535 || n_in > 65535 || n_out > 65535 || H > enc::kMaxDim || W > enc::kMaxDim) return false;
    const size_t per_group = H * W * (n_in > n_out ? n_in : n_out);
    return per_group < lim && groups * per_group < lim;
  };
  if (!range()) return enc::fail(VPIN_EINVAL, (who + ": a dimension is out of range").c_str());
  for (size_t o = 0; o < n_out; o++) {
    bool any = false;
    for (size_t j = 0; j < n_in; j++) any = any || connect[o * n_in + j] != 0;
    if (!any) return enc::fail(VPIN_EINVAL, (who + ": a row of the connection table selects no plane").c_str());
  }
  return VPIN_OK;
}

}  // namespace

}  // namespace vpin

using vpin::enc::fail;

extern "C" int vpin_e2_plane_sums(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t n_in, size_t H, size_t W,
                                  const uint8_t* connect, size_t n_out, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf) {
  const char* who = "vpin_e2_plane_sums";
  if (!c || !px || !py || !pinf || !connect || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_plane_sums: null argument");
  const int bad = vpin::check_sums(who, 1, n_in, H, W, connect, n_out);
  return bad ? bad : vpin::plane_sums(c, who, px, py, pinf, 1, n_in, H * W, connect, n_out, out_x, out_y, out_inf);
}

extern "C" int vpin_e2_plane_sums_batch(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t groups, size_t n_in,
                                        size_t H, size_t W, const uint8_t* connect, size_t n_out, uint8_t* out_x, uint8_t* out_y,
                                        uint8_t* out_inf) {
  const char* who = "vpin_e2_plane_sums_batch";
  if (!c || !px || !py || !pinf || !connect || !out_x || !out_y || !out_inf) return fail(VPIN_EINVAL, "vpin_e2_plane_sums_batch: null argument");
  const int bad = vpin::check_sums(who, groups, n_in, H, W, connect, n_out);
  return bad ? bad : vpin::plane_sums(c, who, px, py, pinf, groups, n_in, H * W, connect, n_out, out_x, out_y, out_inf);
}
