// e2_wire_dev.h -- the square root in F_q that unpacking a point of E2 takes (e2_wire.hip).  q = 5 (mod 8), so a root is one
// fixed exponentiation (Atkin): with beta = (2 n)^((q - 5) / 8) and i = 2 n beta^2 (a square root of -1 whenever n is a square),
// y = n beta (i - 1) satisfies y^2 = n.  The exponent is a constant of 250 bits, 71 of them set: every lane of a wave runs the
// same chain of 249 squarings and 70 products, whatever its input.  For a non-square the chain gives some element whose square
// is not n: the caller compares, and never trusts the root unchecked.
#pragma once
#include "e2_dev.h"

namespace vpin {

// limb i of (q - 5) / 8
__device__ __forceinline__ constexpr uint32_t e2_sqrt_exp_limb(int i) {
  return i == 0 ? 0x4b9eba7du : i == 1 ? 0xcb024c63u : i == 2 ? 0xd45ef39au : i == 3 ? 0x029bdf3bu : i == 7 ? 0x02000000u : 0u;
}

// a^((q - 5) / 8), square-and-multiply from the top bit (bit 249) down, as e2_fq_inv walks q - 2
__device__ __noinline__ fq e2_fq_pow_sqrt_exp(fq a) {
  fq acc = a;
#pragma unroll
  for (int w = 7; w >= 0; w--) {
    const uint32_t e = e2_sqrt_exp_limb(w);
#pragma nounroll
    for (int b = (w == 7 ? 24 : 31); b >= 0; b--) {
      acc = e2_fqm(acc, acc);
      if ((e >> b) & 1u) acc = e2_fqm(acc, a);
    }
  }
  return acc;
}

// *y = a square root of n (Montgomery form in and out) and true, or false when n is not a square.  n = 0 gives y = 0
__device__ __forceinline__ bool fq_sqrt(const fq& n, fq* y) {
  const fq n2 = fq_dbl(n);
  const fq beta = e2_fq_pow_sqrt_exp(n2);
  const fq i = e2_fqm(n2, e2_fqm(beta, beta));
  *y = e2_fqm(e2_fqm(n, beta), fq_sub(i, fq_one()));
  return fq_eq(e2_fqm(*y, *y), n);
}

}  // namespace vpin
