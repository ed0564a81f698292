// hostarith.cpp -- test-only harness: every function of host/field.h and host/curve.h, and the UniPoly / eq / batch-inversion
// helpers of host/prover_common.h, behind one extern "C" function each, so that tests/test_host_arith.py can hand them chosen
// LIMB PATTERNS (not only chosen values) and compare with plain integer arithmetic (tests/host_vectors.py).
//
// Conventions (those of tests/devarith/devarith.hip): inputs and outputs are flat arrays of raw 64-bit words, IW words in and
// OW words out per case, n cases per call; a function returns 0 and never aborts.  An Fq is its four limbs as they lie in
// memory (Montgomery form where the function multiplies), an Fe its five limbs AS THEY ARE -- not bytes: the bounds of
// field.h are about representatives, and from_bytes can only make carried ones.  32 bytes are four little-endian words, a point
// is X | Y | Z | T (20 words), a flag or a digit is one word (digits sign-extended).  hv_table lists every function with its
// IW and OW; tests/hostarith/hostarith_main.cpp drives the same table from a vector file.
//
// KNOWN LIMIT.  The harness checks the arithmetic as written in the headers and compiled at -O3 into THIS library.  It does
// not check the copy that the compiler inlined into prover.cpp, verify.cpp and spark.cpp.
//
// Built by vpin_amd.build.build_hosttest() into vpin_amd/lib/libvpin_hosttest.so: a library of its own, no part of
// libvpin_hip.so and of include/vpin_hip.h, and with no reference to either.
#include <cstdint>
#include <cstring>
#include <vector>

#include "host/field.h"
#include "host/curve.h"
#include "host/prover_common.h"  // unipoly_from_evals, unipoly_eval, combine_bot, fq_batch_invert, host_eq (all static)

using namespace vpin_host;

namespace {

Fq ldq(const uint64_t* p) { Fq r; memcpy(r.l, p, 32); return r; }
void stq(uint64_t* p, const Fq& a) { memcpy(p, a.l, 32); }
Fe lde(const uint64_t* p) { Fe r; memcpy(r.l, p, 40); return r; }
void ste(uint64_t* p, const Fe& a) { memcpy(p, a.l, 40); }
Point ldp(const uint64_t* p) { return Point{lde(p), lde(p + 5), lde(p + 10), lde(p + 15)}; }
void stp(uint64_t* p, const Point& a) { ste(p, a.X); ste(p + 5, a.Y); ste(p + 10, a.Z); ste(p + 15, a.T); }
const uint8_t* by(const uint64_t* p) { return reinterpret_cast<const uint8_t*>(p); }
uint8_t* by(uint64_t* p) { return reinterpret_cast<uint8_t*>(p); }

}  // namespace

#define HV(name, IW, OW, ...)                                           \
  extern "C" int hv_##name(const uint64_t* in_, uint64_t* out_, int n) { \
    for (int i_ = 0; i_ < n; i_++) {                                    \
      const uint64_t* in = in_ + (size_t)i_ * (IW);                     \
      uint64_t* out = out_ + (size_t)i_ * (OW);                         \
      (void)in; (void)out;                                              \
      __VA_ARGS__                                                       \
    }                                                                   \
    return 0;                                                           \
  }

// ---- Fq ---------------------------------------------------------------------------------------------------------------------
HV(fq_add, 8, 4, stq(out, ldq(in) + ldq(in + 4));)
HV(fq_sub, 8, 4, stq(out, ldq(in) - ldq(in + 4));)
HV(fq_neg, 4, 4, stq(out, ldq(in).neg());)
HV(fq_mul, 8, 4, stq(out, ldq(in) * ldq(in + 4));)
HV(fq_square, 4, 4, stq(out, ldq(in).square());)
HV(fq_mont_reduce, 8, 4, uint64_t r[8]; memcpy(r, in, 64); stq(out, Fq::mont_reduce(r));)
HV(fq_reduce_once, 4, 4, stq(out, Fq::reduce_once(in[0], in[1], in[2], in[3]));)
HV(fq_to_bytes, 4, 4, ldq(in).to_bytes(by(out));)
HV(fq_from_bytes_wide, 8, 4, stq(out, Fq::from_bytes_wide(by(in)));)
HV(fq_invert, 4, 4, stq(out, ldq(in).invert());)
HV(fq_from_u64, 1, 4, stq(out, Fq::from_u64(in[0]));)

// ---- Fe ---------------------------------------------------------------------------------------------------------------------
HV(fe_mul, 10, 5, ste(out, lde(in) * lde(in + 5));)
HV(fe_square, 5, 5, ste(out, lde(in).square());)
HV(fe_add, 10, 5, ste(out, lde(in) + lde(in + 5));)
HV(fe_sub, 10, 5, ste(out, lde(in) - lde(in + 5));)
HV(fe_neg, 5, 5, ste(out, lde(in).neg());)
HV(fe_abs, 5, 5, ste(out, lde(in).abs());)
HV(fe_add_lazy, 10, 5, ste(out, lde(in).add_lazy(lde(in + 5)));)
HV(fe_sub_lazy, 10, 5, ste(out, lde(in).sub_lazy(lde(in + 5)));)
HV(fe_carry, 5, 5, Fe t = lde(in); t.carry(); ste(out, t);)
HV(fe_to_bytes, 5, 4, lde(in).to_bytes(by(out));)
HV(fe_from_bytes, 4, 5, ste(out, Fe::from_bytes(by(in)));)
HV(fe_equals, 10, 1, out[0] = lde(in).equals(lde(in + 5));)
HV(fe_is_negative, 5, 1, out[0] = lde(in).is_negative();)
HV(fe_is_zero, 5, 1, out[0] = lde(in).is_zero();)
HV(fe_invert, 5, 5, ste(out, lde(in).invert());)
HV(fe_pow_p58, 5, 5, ste(out, lde(in).pow_p58());)
// u | v -> was_square, root
HV(sqrt_ratio_m1, 10, 6, Fe r; out[0] = sqrt_ratio_m1(r, lde(in), lde(in + 5)); ste(out + 1, r);)

// ---- Point ------------------------------------------------------------------------------------------------------------------
// P | Q | negq -> P + Q or P - Q through Q.cached()
HV(pt_add, 41, 20, stp(out, ldp(in).add(ldp(in + 20).cached(), in[40] != 0));)
HV(pt_dbl, 20, 20, stp(out, ldp(in).dbl());)
HV(pt_equals, 40, 1, out[0] = ldp(in).equals(ldp(in + 20));)
HV(pt_compress, 20, 4, ldp(in).compress(by(out));)
// 32 bytes -> accepted, point (zeros when refused)
HV(pt_decompress, 4, 21, Point p{Fe::zero(), Fe::zero(), Fe::zero(), Fe::zero()}; out[0] = Point::decompress(p, by(in)); stp(out + 1, p);)
HV(pt_elligator, 5, 20, stp(out, Point::elligator(lde(in)));)
HV(pt_from_uniform_bytes, 8, 20, stp(out, Point::from_uniform_bytes(by(in)));)
HV(pt_to_xyzt, 20, 16, ldp(in).to_xyzt(by(out));)
HV(pt_from_xyzt, 16, 20, stp(out, Point::from_xyzt(by(in)));)
// 32 scalar bytes -> top, 257 digits
HV(wnaf5, 4, 258, int8_t naf[257]; out[0] = (uint64_t)(int64_t)Point::wnaf5(by(in), naf);
   for (int k = 0; k < 257; k++) out[1 + k] = (uint64_t)(int64_t)naf[k];)
// P | 32 scalar bytes
HV(pt_mul_bytes, 24, 20, stp(out, ldp(in).mul_bytes(by(in + 20)));)
// a | P | b | Q
HV(pt_mul2_bytes, 48, 20, stp(out, Point::mul2_bytes(by(in), ldp(in + 4), by(in + 24), ldp(in + 28)));)
// acc | base | s (an Fq in Montgomery form) -> acc + s * base over the fixed-base table of base
HV(fb_mul_acc, 44, 20, Point acc = ldp(in); FixedBase fb(ldp(in + 20)); fb.mul_acc(acc, ldq(in + 40)); stp(out, acc);)
// P | niels (y+x, y-x, 2dxy) | negq
HV(fb_add_niels, 36, 20, Niels q{lde(in + 20), lde(in + 25), lde(in + 30)}; stp(out, FixedBase::add_niels(ldp(in), q, in[35] != 0));)

// s -> s through mul_acc over a MARKED table: entry [w][k] is (k + 1)(w + 1) B instead of (k + 1) 2^(10 w) B, so the result is
// (sum of digit_w (w + 1)) B and shows WHICH signed digits the recoder chose -- over the true table a tie at 512 taken as -512
// with a carry is the same group element and no result could tell
namespace {
const std::vector<Niels>& marked_table() {
  static const std::vector<Niels> tab = [] {
    std::vector<Niels> t((size_t)FixedBase::kWindows * FixedBase::kEntries);
    Point g = Point::identity();
    for (int w = 0; w < FixedBase::kWindows; w++) {
      g = g + Point::basepoint();
      Point q = g;
      for (int k = 0; k < FixedBase::kEntries; k++) {
        const Fe zi = q.Z.invert(), x = q.X * zi, y = q.Y * zi;
        t[(size_t)w * FixedBase::kEntries + k] = Niels{y + x, y - x, x * y * K().d2};
        q = q.add(g.cached());
      }
    }
    return t;
  }();
  return tab;
}
}  // namespace
HV(fb_mul_acc_marked, 4, 20, FixedBase fb; fb.t = marked_table().data(); Point acc = Point::identity(); fb.mul_acc(acc, ldq(in)); stp(out, acc);)

// ---- prover_common.h --------------------------------------------------------------------------------------------------------
HV(unipoly_from_evals3, 12, 12, Fq e[3], c[3]; for (int k = 0; k < 3; k++) e[k] = ldq(in + 4 * k);
   vpin_prover::unipoly_from_evals(e, 3, c); for (int k = 0; k < 3; k++) stq(out + 4 * k, c[k]);)
HV(unipoly_from_evals4, 16, 16, Fq e[4], c[4]; for (int k = 0; k < 4; k++) e[k] = ldq(in + 4 * k);
   vpin_prover::unipoly_from_evals(e, 4, c); for (int k = 0; k < 4; k++) stq(out + 4 * k, c[k]);)
// coefficients | r
HV(unipoly_eval3, 16, 4, Fq c[3]; for (int k = 0; k < 3; k++) c[k] = ldq(in + 4 * k); stq(out, vpin_prover::unipoly_eval(c, 3, ldq(in + 12)));)
HV(unipoly_eval4, 20, 4, Fq c[4]; for (int k = 0; k < 4; k++) c[k] = ldq(in + 4 * k); stq(out, vpin_prover::unipoly_eval(c, 4, ldq(in + 16)));)
// 8 evaluations | 3 challenges
HV(combine_bot3, 44, 4, std::vector<Fq> e(8), ch(3); for (int k = 0; k < 8; k++) e[k] = ldq(in + 4 * k);
   for (int k = 0; k < 3; k++) ch[k] = ldq(in + 32 + 4 * k); stq(out, vpin_prover::combine_bot(e, ch));)
// 3 challenges -> 8 evaluations
HV(host_eq3, 12, 32, Fq r[3], o[8]; for (int k = 0; k < 3; k++) r[k] = ldq(in + 4 * k); vpin_prover::host_eq(r, 3, o);
   for (int k = 0; k < 8; k++) stq(out + 4 * k, o[k]);)

// one batch of n non-zero elements (the one function whose n is the size of its single case)
extern "C" int hv_fq_batch_invert(const uint64_t* in, uint64_t* out, int n) {
  std::vector<Fq> v((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) v[(size_t)i] = ldq(in + 4 * i);
  vpin_prover::fq_batch_invert(v.data(), v.size());
  for (int i = 0; i < n; i++) stq(out + 4 * i, v[(size_t)i]);
  return 0;
}

struct hv_entry { const char* name; int iw, ow; int (*fn)(const uint64_t*, uint64_t*, int); };
#define E(name, iw, ow) {#name, iw, ow, hv_##name}
static const hv_entry kTable[] = {
    E(fq_add, 8, 4), E(fq_sub, 8, 4), E(fq_neg, 4, 4), E(fq_mul, 8, 4), E(fq_square, 4, 4), E(fq_mont_reduce, 8, 4),
    E(fq_reduce_once, 4, 4), E(fq_to_bytes, 4, 4), E(fq_from_bytes_wide, 8, 4), E(fq_invert, 4, 4), E(fq_from_u64, 1, 4),
    E(fe_mul, 10, 5), E(fe_square, 5, 5), E(fe_add, 10, 5), E(fe_sub, 10, 5), E(fe_neg, 5, 5), E(fe_abs, 5, 5),
    E(fe_add_lazy, 10, 5), E(fe_sub_lazy, 10, 5), E(fe_carry, 5, 5), E(fe_to_bytes, 5, 4), E(fe_from_bytes, 4, 5),
    E(fe_equals, 10, 1), E(fe_is_negative, 5, 1), E(fe_is_zero, 5, 1), E(fe_invert, 5, 5), E(fe_pow_p58, 5, 5),
    E(sqrt_ratio_m1, 10, 6), E(pt_add, 41, 20), E(pt_dbl, 20, 20), E(pt_equals, 40, 1), E(pt_compress, 20, 4),
    E(pt_decompress, 4, 21), E(pt_elligator, 5, 20), E(pt_from_uniform_bytes, 8, 20), E(pt_to_xyzt, 20, 16),
    E(pt_from_xyzt, 16, 20), E(wnaf5, 4, 258), E(pt_mul_bytes, 24, 20), E(pt_mul2_bytes, 48, 20), E(fb_mul_acc, 44, 20),
    E(fb_add_niels, 36, 20), E(fb_mul_acc_marked, 4, 20), E(unipoly_from_evals3, 12, 12), E(unipoly_from_evals4, 16, 16), E(unipoly_eval3, 16, 4),
    E(unipoly_eval4, 20, 4), E(combine_bot3, 44, 4), E(host_eq3, 12, 32), E(fq_batch_invert, 4, 4),
};
#undef E

// the table of every function above: name, words in and out per case (fq_batch_invert: per element)
extern "C" int hv_table(const hv_entry** out) {
  *out = kTable;
  return (int)(sizeof(kTable) / sizeof(kTable[0]));
}
