// e2_wire.hip -- points of E2 as they cross a byte stream: 32 bytes each instead of 32 + 32 + a flag byte.  E2's group order is
// prime and the only multiple of itself inside the Hasse interval, so every point of the curve is in the group and a point is
// its x, the parity of its y and an identity bit.  A packed point is one 256-bit little-endian integer:
//   bits 0 .. 252  the canonical x, x < q        bit 254  the identity; all other bits are zero then
//   bit 253        zero                          bit 255  bit 0 of the canonical y in [0, q)
// What arrives packed is untrusted input, so the receiver's work is on the device:
//   e2_pack_kernel    one lane per point: the range and curve checks of e2_load_kernel, then the parity of the canonical y
//   e2_unpack_kernel  one lane per point: x to Montgomery form, rhs = x^3 + a x + b, y = fq_sqrt(rhs) by one fixed exponentiation
//                     (e2_wire_dev.h), the check y^2 == rhs, y to canonical form, y or q - y by bit 255.  A lane with a bad
//                     encoding writes its rule into `bad` and stays on the common path: the chain is the same for every lane
// Both write one rule byte per point; the host names the first bad index (as vpin_e2_client_round names its first element), or,
// for the replies of several clients in one launch (wire::unpack_rules), finds whose point it is.
#include "e2_wire_dev.h"
#include "enc_conv.h"
#include "wire.h"

#include <cstdio>
#include <vector>

namespace vpin {

namespace {

constexpr uint8_t kWireRange = 1;     // x (pack: a coordinate) is not below q
constexpr uint8_t kWireBit253 = 2;    // bit 253 is set
constexpr uint8_t kWireIdentity = 3;  // the identity bit together with any other bit
constexpr uint8_t kWireNoRoot = 4;    // rhs is not a square (pack: the point is off the curve)
constexpr uint8_t kWireParity = 5;    // y = 0 with the parity bit (no such point on E2; never a second encoding of one)

__device__ __forceinline__ bool below_q(const fq& v) {
  unsigned bw = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) (void)__builtin_subc(v.v[k], fq_modulus_limb(k), bw, &bw);
  return bw != 0;  // a borrow: the value is below q
}

__device__ __forceinline__ fq curve_rhs(const fq& x, const fq& a, const fq& b) { return fq_add(e2_fqm(fq_add(e2_fqm(x, x), a), x), b); }

__global__ __launch_bounds__(kE2Block) void e2_pack_kernel(const fq* __restrict__ xb, const fq* __restrict__ yb, const uint8_t* __restrict__ inf,
                                                           size_t n, fq a, fq b, fq* __restrict__ out, uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  fq xr = fq_load(xb + i);
  const fq yr = fq_load(yb + i);
  const bool idn = inf[i] != 0;
  uint8_t f = (below_q(xr) && below_q(yr)) ? 0 : kWireRange;
  const fq x = e2_fqm(xr, e2_fq_r2()), y = e2_fqm(yr, e2_fq_r2());
  if (!f && !idn && !fq_eq(e2_fqm(y, y), curve_rhs(x, a, b))) f = kWireNoRoot;
  if (idn) xr = fq_zero();
  xr.v[7] |= idn ? 0x40000000u : (yr.v[0] & 1u) << 31;
  fq_store(out + i, f ? fq_zero() : xr);
  bad[i] = f;
}

__global__ __launch_bounds__(kE2Block) void e2_unpack_kernel(const fq* __restrict__ in, size_t n, fq a, fq b, fq* __restrict__ X,
                                                             fq* __restrict__ Y, uint8_t* __restrict__ inf, uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * kE2Block + threadIdx.x;
  if (i >= n) return;
  const fq v = fq_load(in + i);
  const uint32_t par = v.v[7] >> 31;
  const bool idn = ((v.v[7] >> 30) & 1u) != 0;
  fq xr = v;
  xr.v[7] &= 0x1fffffffu;
  uint8_t f = 0;
  if (idn) {
    uint32_t o = v.v[7] ^ 0x40000000u;
#pragma unroll
    for (int k = 0; k < 7; k++) o |= v.v[k];
    if (o) f = kWireIdentity;
  } else if ((v.v[7] >> 29) & 1u) {
    f = kWireBit253;
  } else if (!below_q(xr)) {
    f = kWireRange;  // x is never reduced: x = q is not x = 0
  }
  // the common path, whatever the lane holds
  const fq x = e2_fqm(xr, e2_fq_r2());
  const fq rhs = curve_rhs(x, a, b);
  fq y;
  const bool ok = fq_sqrt(rhs, &y);
  fq yc = fq_from_mont(y);
  if (!f && !idn && !ok) f = kWireNoRoot;
  if ((yc.v[0] & 1u) != par) yc = fq_neg(yc);  // q - y: the other parity, q being odd; 0 stays 0
  if (!f && !idn && (yc.v[0] & 1u) != par) f = kWireParity;
  const bool blank = f || idn;
  fq_store(X + i, blank ? fq_zero() : xr);
  fq_store(Y + i, blank ? fq_zero() : yc);
  inf[i] = (!f && idn) ? 1 : 0;
  bad[i] = f;
}

// the coefficient b of E2, canonical little-endian
const uint8_t kBBytes[32] = {86, 83, 202, 68, 110, 236, 64, 249, 56, 118, 236, 1, 191, 143, 126, 100,
                             4, 149, 41, 137, 111, 171, 93, 146, 250, 112, 171, 90, 44, 184, 8, 8};

const char* rule_text(uint8_t f, bool pack) {
  switch (f) {
    case kWireRange: return pack ? "a coordinate is not below q" : "x is not below q";
    case kWireBit253: return "bit 253 is set";
    case kWireIdentity: return "the identity bit is set together with other bits";
    case kWireNoRoot: return pack ? "the point is not on the curve E2" : "x is not on the curve E2 (x^3 + a x + b is not a square)";
    default: return "the parity bit is set over y = 0";
  }
}

int first_bad(const std::vector<uint8_t>& bad, const char* who, bool pack) {
  for (size_t i = 0; i < bad.size(); i++) {
    if (!bad[i]) continue;
    char why[200];
    snprintf(why, sizeof why, "%s: point %zu: %s", who, i, rule_text(bad[i], pack));
    return enc::fail(VPIN_EINVAL, why);
  }
  return VPIN_OK;
}

}  // namespace

namespace wire {

const char* unpack_rule_text(uint8_t rule) { return rule_text(rule, false); }

int unpack_rules(vpin_ctx* c, const uint8_t* in32, size_t cnt, uint8_t* px, uint8_t* py, uint8_t* pinf, uint8_t* bad) {
  (void)hipSetDevice(c->device);
  DevBuf in(c), x(c), y(c), f(c), b(c);
  if (in.alloc(cnt * 32) || x.alloc(cnt * 32) || y.alloc(cnt * 32) || f.alloc(cnt) || b.alloc(cnt)) return VPIN_ENOMEM;
  VPIN_HIP_TRY(hipMemcpyAsync(in.p, in32, cnt * 32, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_unpack_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, (const fq*)in.p, cnt, e2_curve_a(),
                     fq_of_le32(kBBytes), (fq*)x.p, (fq*)y.p, (uint8_t*)f.p, (uint8_t*)b.p);
  VPIN_HIP_TRY(hipGetLastError());
  VPIN_HIP_TRY(hipMemcpyAsync(px, x.p, cnt * 32, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(py, y.p, cnt * 32, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(pinf, f.p, cnt, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(bad, b.p, cnt, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return VPIN_OK;
}

}  // namespace wire

}  // namespace vpin

using namespace vpin;

extern "C" {

int vpin_e2_pack(vpin_ctx* c, const uint8_t* px, const uint8_t* py, const uint8_t* pinf, size_t cnt, uint8_t* out32) {
  if (!c || !px || !py || !pinf || !out32) return enc::fail(VPIN_EINVAL, "vpin_e2_pack: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 31)) return enc::fail(VPIN_EINVAL, "vpin_e2_pack: cnt must be in 1 .. 2^31 - 1");
  (void)hipSetDevice(c->device);
  DevBuf x(c), y(c), f(c), o(c), b(c);
  if (x.alloc(cnt * 32) || y.alloc(cnt * 32) || f.alloc(cnt) || o.alloc(cnt * 32) || b.alloc(cnt)) return VPIN_ENOMEM;
  std::vector<uint8_t> bad(cnt);
  VPIN_HIP_TRY(hipMemcpyAsync(x.p, px, cnt * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(y.p, py, cnt * 32, hipMemcpyHostToDevice, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(f.p, pinf, cnt, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(e2_pack_kernel, dim3(blocks_of(cnt, kE2Block)), dim3(kE2Block), 0, c->stream, (const fq*)x.p, (const fq*)y.p,
                     (const uint8_t*)f.p, cnt, e2_curve_a(), fq_of_le32(kBBytes), (fq*)o.p, (uint8_t*)b.p);
  VPIN_HIP_TRY(hipGetLastError());
  VPIN_HIP_TRY(hipMemcpyAsync(out32, o.p, cnt * 32, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipMemcpyAsync(bad.data(), b.p, cnt, hipMemcpyDeviceToHost, c->stream));
  VPIN_HIP_TRY(hipStreamSynchronize(c->stream));
  return first_bad(bad, "vpin_e2_pack", true);
}

int vpin_e2_unpack(vpin_ctx* c, const uint8_t* in32, size_t cnt, uint8_t* px, uint8_t* py, uint8_t* pinf) {
  if (!c || !in32 || !px || !py || !pinf) return enc::fail(VPIN_EINVAL, "vpin_e2_unpack: null argument");
  if (cnt == 0 || cnt >= ((size_t)1 << 31)) return enc::fail(VPIN_EINVAL, "vpin_e2_unpack: cnt must be in 1 .. 2^31 - 1");
  std::vector<uint8_t> bad(cnt);
  const int rc = wire::unpack_rules(c, in32, cnt, px, py, pinf, bad.data());
  if (rc) return rc;
  return first_bad(bad, "vpin_e2_unpack", false);
}

}  // extern "C"
