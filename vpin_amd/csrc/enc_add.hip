// enc_add.hip -- the device stage of the addition layer (driven by enc_add.cpp): out[p][t] = X[p][t] + R[p][t] over P planes of
// two resident point sets of the same shape, the skip connection of a residual block.  Beside enc_convmc.hip, whose
// e2_bias_add_kernel is the same addition with one second operand per plane; here there is one per element.
//
//   e2_pair_add_kernel  one lane per element, one wave per workgroup, the plane on the grid's y axis: one mixed addition,
//                       complete by case (e2_dev.h): R = X doubles, R = -X gives the flagged identity, a flagged R adds nothing.
//                       The lane that finds X[p][t] flagged marks its plane in `bad`: the first operand of an addition has no
//                       flag in the witness format, and the scan runs here, on the flags, beside the addition
// Results are Jacobian; the one normalisation follows (e2_emit).
#include "e2_dev.h"
#include "enc_conv.h"

namespace vpin {

namespace {

constexpr int kPairBlock = 64;  // one wave: a lane is one mixed addition

// grid: x = blocks of kPairBlock elements of a plane, y = plane.  bad: one byte per plane, zeroed by the caller; every lane that
// writes it writes 1
__global__ __launch_bounds__(kPairBlock) void e2_pair_add_kernel(const fq* __restrict__ XX, const fq* __restrict__ XY,
                                                                 const uint8_t* __restrict__ xinf, const fq* __restrict__ RX,
                                                                 const fq* __restrict__ RY, const uint8_t* __restrict__ rinf, size_t n_pix,
                                                                 fq a, e2_jac* __restrict__ out, uint8_t* __restrict__ bad) {
  const size_t t = (size_t)blockIdx.x * kPairBlock + threadIdx.x, plane = blockIdx.y;
  if (t >= n_pix) return;
  const size_t i = plane * n_pix + t;
  e2_jac acc = e2_identity();
  if (!rinf[i]) { acc.X = fq_load(RX + i); acc.Y = fq_load(RY + i); acc.Z = fq_one(); }
  if (xinf[i]) bad[plane] = 1;
  else acc = e2_add_mixed(acc, fq_load(XX + i), fq_load(XY + i), a);
  e2_store(out + i, acc);
}

}  // namespace

int e2_pair_add(vpin_ctx* c, const E2Points& x, const E2Points& r, size_t P, size_t per_plane, uint8_t* out_x, uint8_t* out_y, uint8_t* out_inf,
                uint8_t* bad_plane) {
  (void)hipSetDevice(c->device);
  const size_t n = P * per_plane;
  DevBuf jac(c), bad(c);
  if (jac.alloc(n * sizeof(e2_jac)) || bad.alloc(P)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemsetAsync(bad.p, 0, P, c->stream));
  hipLaunchKernelGGL(e2_pair_add_kernel, dim3(blocks_of(per_plane, kPairBlock), (unsigned)P), dim3(kPairBlock), 0, c->stream, x.X(), x.Y(), x.F(),
                     r.X(), r.Y(), r.F(), per_plane, e2_curve_a(), (e2_jac*)jac.p, (uint8_t*)bad.p);
  VPIN_HIP_TRY(hipGetLastError());
  VPIN_HIP_TRY(hipMemcpyAsync(bad_plane, bad.p, P, hipMemcpyDeviceToHost, c->stream));
  return e2_emit(c, (const e2_jac*)jac.p, n, out_x, out_y, out_inf);  // synchronises: bad_plane has arrived too
}

}  // namespace vpin
