"""Chosen limb patterns, encodings and scalars for the HOST arithmetic (vpin_amd/csrc/host/field.h, curve.h, and the UniPoly /
eq / batch-inversion helpers of prover_common.h) and their expected values in plain Python integers.  Nothing here depends on
the code under test: tests/test_host_vectors.py checks on the CPU that every named class is present, tests/test_host_arith.py
runs the groups through tests/hostarith/hostarith.cpp, and the same groups go to the sanitizer program as a vector file.

Forms.  An Fq is four 64-bit limbs, a canonical value times 2^256 mod q where the function multiplies.  An Fe is five limbs of
weight 2^(51 i) AS THEY ARE: a product takes limbs up to 2^54 - 1 and returns limbs 0, 2, 3, 4 below 2^51 and limb 1 below
2^51 + 2^13; carry() returns limbs 1..4 below 2^51 and limb 0 below 2^51 + 19; operator- and sub_lazy add the limbs of 4p,
SUB_BIAS, so the subtrahend's limbs may reach SUB_BIAS and not one more.

A group is (function of the harness, input rows of 64-bit words, check(output rows)); check asserts exact equality."""
import hashlib
import json
import os
import random
from collections import OrderedDict, namedtuple

import digit_vectors as DV
import limb_vectors as LV
import pymodel as PM
import pymodel_group as PG

P, Q = LV.P, LV.Q
R, R2, RINV = LV.R, LV.R2, LV.RINV
R3 = R * R2 % Q
U64 = 1 << 64
M64 = U64 - 1
M51 = (1 << 51) - 1
TOP = (1 << 54) - 1                                   # the largest limb a product takes
SUB_BIAS = [4 * (M51 - 18)] + [4 * M51] * 4           # 4p, limb by limb
PROD_MAX = [M51, M51 + (1 << 13), M51, M51, M51]      # the largest limbs a product returns
CARRY_MAX = [M51 + 19, M51, M51, M51, M51]            # ... and carry()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Group = namedtuple("Group", "fn rows check")


def words(x, n=4):
    assert 0 <= x < 1 << (64 * n), hex(x)
    return [(x >> (64 * i)) & M64 for i in range(n)]


def unwords(ws):
    return sum(int(w) << (64 * i) for i, w in enumerate(ws))


def signed(w):
    w = int(w)
    return w - U64 if w >> 63 else w


def mont(x):
    return words(x % Q * R % Q)


def unmont(ws):
    v = unwords(ws)
    assert v < Q, "not canonical limbs: " + hex(v)
    return v * RINV % Q


# ---- F_q ---------------------------------------------------------------------------------------------------------------------
FQ_VALUES = LV._uniq([0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, 2**252 - 1, 2**252, R, R2] + [M64 << (64 * i) for i in range(3)]
                     + [0x0FFFFFFFFFFFFFFF << 192])   # a lone all-ones limb in each position, the top one capped below q
FQ_NONREDUCED = [Q, Q + 1, 2 * Q - 1, 2**256 - 1, M64 << 192]  # first operands from_bytes_wide hands to operator*
FQ_PAIRS = [(a, b) for a in FQ_VALUES for b in FQ_VALUES]
FQ_MUL_PAIRS = FQ_PAIRS + [(a, b) for a in FQ_NONREDUCED for b in FQ_VALUES + [R3]]
FQ_MONT_REDUCE = [0, 1, Q - 1, Q, 2**256 - 1, 2**256, Q * 2**256 - 1, (Q - 1) * 2**256, (Q - 1) ** 2, M64 << 256, (2**256 - 1) * (Q - 1)]
FQ_REDUCE_ONCE = LV._uniq([0, 1, Q - 1, Q, Q + 1, 2 * Q - 2, 2 * Q - 1, 2**252, 2**253 - 1] + [a + b for a, b in FQ_PAIRS])
FQ_WIDE = [2**512 - 1, (2**256 - 1) << 256, 2**256 - 1, 0, 1, Q, Q << 256, 2**256, (Q - 1) | ((Q - 1) << 256)]
FQ_INVERT = [0, 1, Q - 1, 2, Q - 2, R, 2**252]
FQ_U64 = [0, 1, 2, 6, 2**32, 2**63, M64]


def _rand_fq(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(Q) for _ in range(n)]


def fq_kat():
    with open(os.path.join(GOLDEN, "fq_kat.json")) as f:
        return json.load(f)


# ---- GF(2^255-19): the limb arithmetic of field.h restated on Python integers, every 64- and 128-bit wrap reported -----------
def fe_value(l):
    return sum(int(x) << (51 * i) for i, x in enumerate(l))


def fe_limbs(v):
    """the 51-bit slices of v < 2^256 + ..: limb 4 keeps what is above bit 204"""
    return [(v >> (51 * i)) & M51 for i in range(4)] + [v >> 204]


def fe_mul_model(x, y):
    """operator*: (limbs, facts).  facts: ok (nothing wrapped), c0 (the carry out of t0), c19 (19 * the carry out of t4)"""
    ok = True
    y19 = [19 * v for v in y]
    ok &= all(v < U64 for v in y19)
    t = []
    for k in range(5):
        s = 0
        for i in range(5):
            j = (k - i) % 5
            s += x[i] * (y19[j] if i + j >= 5 else y[j])
        t.append(s)
    ok &= all(v < 1 << 128 for v in t)
    r, facts = [0] * 5, {}
    for k in range(4):
        c = t[k] >> 51
        if k == 0:
            facts["c0"] = c
        ok &= c < U64
        t[k + 1] += c
        ok &= t[k + 1] < 1 << 128
        r[k] = t[k] & M51
    c = t[4] >> 51
    ok &= c < U64
    r[4] = t[4] & M51
    facts["c19"] = 19 * c
    r[0] += 19 * c
    ok &= r[0] < U64
    r[1] += r[0] >> 51
    r[0] &= M51
    facts["ok"] = bool(ok)
    return r, facts


def fe_carry_model(l, passes=2):
    l = list(l)
    for _ in range(passes):
        for i in range(4):
            l[i + 1] += l[i] >> 51
            l[i] &= M51
        c = l[4] >> 51
        l[4] &= M51
        l[0] += 19 * c
    return l


def fe_sub_lazy_model(a, b):
    """(limbs as the 64-bit machine leaves them, whether a limb went below zero)"""
    d = [x + s - y for x, s, y in zip(a, SUB_BIAS, b)]
    return [v % U64 for v in d], any(v < 0 for v in d)


def fe_sub_model(a, b):
    l, under = fe_sub_lazy_model(a, b)
    return fe_carry_model(l), under


def within(l, bound):
    return all(0 <= int(x) <= m for x, m in zip(l, bound))


FE_LIMB_CHOICES = [0, 1, M51, M51 + 1, TOP - 1, TOP]


def fe_mul_cases():
    rng = random.Random(0x51)
    top, z = [TOP] * 5, [0] * 5
    single = [[TOP if k == i else 0 for k in range(5)] for i in range(5)]
    cases = [(top, top), (top, z), (z, top), (top, [1, 0, 0, 0, 0]), ([1, 0, 0, 0, 0], top)]
    cases += [(a, b) for a in single for b in single] + [(a, top) for a in single] + [(top, b) for b in single]
    mixed = [[TOP if (k + s) % 2 else 0 for k in range(5)] for s in (0, 1)] + [[TOP if (k + s) % 2 else M51 + 1 for k in range(5)] for s in (0, 1)]
    mixed += [[M51 + 1] * 5, [M51] * 5, [0, M51 + 1, TOP, 0, M51 + 1], [TOP, 0, M51 + 1, TOP, 0]]
    cases += [(a, b) for a in mixed for b in mixed + [top]]
    cases += [([rng.choice(FE_LIMB_CHOICES) for _ in range(5)], [rng.choice(FE_LIMB_CHOICES) for _ in range(5)]) for _ in range(512)]
    cases += [([rng.randrange(TOP + 1) for _ in range(5)], [rng.randrange(TOP + 1) for _ in range(5)]) for _ in range(512)]
    return cases


def fe_square_cases():
    return LV._uniq([tuple(a) for a, _ in fe_mul_cases()])


def fe_sub_cases():
    """(a, b) fed to operator- and sub_lazy: b at SUB_BIAS in each limb alone and in all, a zero, carried or at a product's top"""
    rng = random.Random(0x5B)
    z = [0] * 5
    firsts = [z, [M51] * 5, list(PROD_MAX), list(CARRY_MAX)]
    seconds = [[SUB_BIAS[k] if k == i else 0 for k in range(5)] for i in range(5)] + [list(SUB_BIAS), z, [M51] * 5, list(PROD_MAX), list(CARRY_MAX)]
    cases = [(a, b) for a in firsts for b in seconds]
    cases += [([rng.randrange(m + 1) for m in PROD_MAX], [rng.randrange(m + 1) for m in SUB_BIAS]) for _ in range(256)]
    return cases


def fe_sub_lazy_cases():
    """sub_lazy feeds products: its first operand may be a lazy sum as add_niels forms it (2 Z, limbs up to 2 PROD_MAX)"""
    return fe_sub_cases() + [([2 * m for m in PROD_MAX], b) for b in (list(SUB_BIAS), list(PROD_MAX))]


def fe_sub_above_cases():
    """one above the bound, for the CPU model alone -- NEVER fed to the library"""
    z = [0] * 5
    return [(z, [SUB_BIAS[k] + (1 if k == i else 0) for k in range(5)]) for i in range(5)]


# representatives for to_bytes / equals / is_negative / is_zero: (label, limbs)
def fe_reps():
    named = [("0", 0), ("1", 1), ("18", 18), ("19", 19), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^255-1", 2**255 - 1),
             ("2^255", 2**255), ("2^255+18", 2**255 + 18), ("2p-1", 2 * P - 1), ("2p", 2 * P), ("2p+1", 2 * P + 1)]
    out = [(n, fe_limbs(v)) for n, v in named]
    out.append(("2^255+18 as limb 0 = 2^51+18", [M51 + 19, M51, M51, M51, M51]))   # what one pass of carry leaves of the next
    out.append(("limb 4 = 2^52-1, the rest 2^51-1", [M51, M51, M51, M51, 2 * M51 + 1]))
    out.append(("p in lazy limbs", [2 * (M51 - 18) - (M51 - 18)] + [M51] * 4))
    out.append(("4p", list(SUB_BIAS)))
    out.append(("every limb 2^54-1", [TOP] * 5))
    out.append(("product top", list(PROD_MAX)))
    return out


FE_POW_VALUES = [("1", [1, 0, 0, 0, 0]), ("p-1", fe_limbs(P - 1)), ("2", [2, 0, 0, 0, 0]), ("every limb 2^51-1", [M51] * 5),
                 ("every limb 2^54-1", [TOP] * 5), ("0", [0] * 5), ("sqrt(-1)", fe_limbs(PG.SQRT_M1))]


def sqrt_ratio_outcome(u, v):
    """which of the four ways SQRT_RATIO_M1 leaves: correct, flipped, flipped_i, none"""
    u, v = u % P, v % P
    v3 = v * v % P * v % P
    v7 = v3 * v3 % P * v % P
    r = u * v3 % P * pow(u * v7 % P, (P - 5) // 8, P) % P
    check = v * r % P * r % P
    if check == u:
        return "correct"
    if check == (-u) % P:
        return "flipped"
    if check == (-u) * PG.SQRT_M1 % P:
        return "flipped_i"
    return "none"


def sqrt_ratio_cases():
    """(u, v, limbs of u, limbs of v)"""
    uv = [(u, v) for u in range(0, 24) for v in range(0, 6)] + [(P - 1, 1), (1, P - 1), (PG.SQRT_M1, 1), (4, 9), (P - 4, 9), (0, 0)]
    out = [(u, v, fe_limbs(u), fe_limbs(v)) for u, v in uv]
    out += [(u, v, fe_limbs(u + P), fe_limbs(v + P)) for u, v in uv[:40]]
    # a lazy representative of u: + 2p limb by limb, within what u.neg() inside the function may take
    out += [(u, v, [x + y // 2 for x, y in zip(fe_limbs(u), SUB_BIAS)], fe_limbs(v)) for u, v in uv[6:30]]
    return out


# ---- points ------------------------------------------------------------------------------------------------------------------
def pt_limbs(pt, lazy=0):
    """extended coordinates as 20 limbs; lazy = 1: every coordinate + p, 2: + 2p limb by limb (limbs up to 2^52 + 2^51, still a
    subtrahend operator- may take)"""
    co = [pt.X, pt.Y, pt.Z, pt.T]
    if lazy == 1:
        return [w for c in co for w in fe_limbs(c + P)]
    if lazy == 2:
        return [x + s // 2 for c in co for x, s in zip(fe_limbs(c), SUB_BIAS)]
    return [w for c in co for w in fe_limbs(c)]


def pt_of(ws):
    """20 output limbs -> Pt, with the curve equation and X Y = Z T checked"""
    X, Y, Z, T = (fe_value(ws[5 * i:5 * i + 5]) % P for i in range(4))
    assert (X * Y - Z * T) % P == 0, "X Y != Z T"
    assert (-X * X + Y * Y - Z * Z - PG.D * T * T) % P == 0 and Z != 0, "not on the curve"
    return PG.Pt(X, Y, Z, T)


def _torsion4():
    """the 4-torsion subgroup: identity, (0, -1), (+-i, 0) -- a point's ristretto coset is P + each of them"""
    i = PG.SQRT_M1
    return [PG.Pt.identity(), PG.Pt(i, 0, 1, 0), PG.Pt(0, P - 1, 1, 0), PG.Pt(P - i, 0, 1, 0)]


TORSION4 = _torsion4()


def base_points():
    return LV.base_points() + [5 * PG.basepoint(), gens_point(0), gens_point(3)]


def coset(pt):
    return [pt + t for t in TORSION4]


def compress_rotates(pt):
    """does RFC 9496 4.3.2 take the rotate branch on this representative"""
    x0, y0, z0, t0 = pt.X, pt.Y, pt.Z, pt.T
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = PG.sqrt_ratio_m1(1, u1 * u2 % P * u2 % P)
    z_inv = invsqrt * u1 % P * (invsqrt * u2 % P) % P * t0 % P
    return bool((t0 * z_inv % P) & 1)


_GENS = {}


def gens_stream(nb, label=b"gens_r1cs_sat"):
    """MultiCommitGens::new: SHAKE256(label || B compressed) -> nb x 64 bytes"""
    return hashlib.shake_256(label + PG.basepoint().encode()).digest(64 * nb)


def gens_point(i):
    if i not in _GENS:
        _GENS[i] = PG.from_uniform_bytes(gens_stream(i + 1)[64 * i:64 * i + 64])
    return _GENS[i]


def decode_steps(s):
    """RFC 9496 4.3.1 on a canonical even s, step by step: (was_square, x was negated, t is negative, y == 0)"""
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2s = u2 * u2 % P
    v = (-(PG.D * u1 % P * u1) - u2s) % P
    ok, invsqrt = PG.sqrt_ratio_m1(1, v * u2s % P)
    den_x = invsqrt * u2 % P
    x0 = 2 * s * den_x % P
    x = P - x0 if x0 & 1 else x0
    y = u1 * (invsqrt * den_x % P * v % P) % P
    return ok, bool(x0 & 1), bool((x * y % P) & 1), y == 0


def _enc(pt):
    return int.from_bytes(pt.encode(), "little")


def decompress_classes():
    """name -> encodings (integers below 2^256).  'good*' decode, every other class is refused -- and for the reason in its name
    ALONE where that is possible, so that dropping one test of Point::decompress lets a class through"""
    B = PG.basepoint()
    good = sorted({_enc(p) for p in base_points()} | {_enc(k * B) for k in range(2, 40)})
    small = list(range(2, 200, 2))
    cl = OrderedDict()
    cl["identity"] = [0]
    cl["good, x negated"] = [s for s in good if decode_steps(s)[1]]
    cl["good, x not negated"] = [s for s in good if not decode_steps(s)[1]]
    cl["s >= p"] = [P, P + 2, 2**255 - 1] + [P + 1, P + 3, 2**255 - 2] + [s + P for s in good if s + P < 2**255]
    cl["bit 255 set"] = [s + 2**255 for s in good[:8]] + [2**255, 2**256 - 1, 2**256 - 2]
    cl["odd s, the negative root of a good one"] = [P - s for s in good[:8]]
    cl["odd s"] = [1, 3, P - 2] + [s + 1 for s in good[:4]]
    cl["s = p - 1 (y = 0)"] = [P - 1]
    cl["non-square"] = [s for s in small if not decode_steps(s)[0]]
    cl["negative t"] = [s for s in small if decode_steps(s)[0] and decode_steps(s)[2]]
    cl["good, small"] = [s for s in small if PG.decode(s.to_bytes(32, "little")) is not None]
    # even and at least p (p + v, v odd below 19): the parity test passes them, the canonical check alone refuses them
    cl["s >= p, even"] = [P + v for v in (1, 3, 5, 7, 9, 11, 13, 15, 17)]
    return cl


def decompress_all():
    seen, out = set(), []
    for name, xs in decompress_classes().items():
        for s in xs:
            if s not in seen:
                seen.add(s)
                out.append((name, s))
    return out


# ---- wnaf5 -------------------------------------------------------------------------------------------------------------------
def wnaf5_model(k):
    """the textbook width-5 NAF: (257 digits, index of the top non-zero digit or -1)"""
    d, i, top = [0] * 257, 0, -1
    while k:
        if k & 1:
            v = k & 31
            if v > 16:
                v -= 32
            d[i], top = v, i
            k -= v
        k >>= 1
        i += 1
    return d, top


def wnaf5_cases():
    """(name, scalar).  straddle: the first set bit at bit b = 59..63 of word w, a window value above 16 (a negative digit, so
    2^(pos+5) is carried in), the bits above the window all ones up to the end of the next word, or of the next two"""
    out = [("0", 0), ("1", 1), ("2^253-1", 2**253 - 1), ("q-1", Q - 1), ("2^252", 2**252), ("15", 15), ("17", 17), ("31", 31)]
    for w in range(3):
        for b in range(59, 64):
            pos = 64 * w + b
            for d in (17, 31):
                for span in (1, 2):
                    end = min(64 * (w + 1 + span), 252)
                    if end <= pos + 5:
                        continue
                    ones = ((1 << end) - 1) ^ ((1 << (pos + 5)) - 1)
                    out.append((f"straddle w={w} b={b} d={d} ones to bit {end}", (d << pos) | ones))
                out.append((f"straddle w={w} b={b} d={d} alone", d << pos))
                out.append((f"straddle w={w} b={b} d={d - 16} positive", ((d - 16) | 0) << pos))
    rng = random.Random(0xAF)
    out += [(f"random {i}", rng.randrange(Q)) for i in range(64)]
    return out


# ---- fixed-base windows ------------------------------------------------------------------------------------------------------
FB_BITS, FB_WINDOWS, FB_HALF = 10, 26, 512


def fb_digits(s):
    """FixedBase::mul_acc's signed 10-bit digits of a canonical s: (26 digits, the window values v = bits + carry, last carry)"""
    out, vs, carry = [], [], 0
    for w in range(FB_WINDOWS):
        v = ((s >> (FB_BITS * w)) & 1023) + carry
        neg = v > FB_HALF
        out.append(v - 1024 if neg else v)
        vs.append(v)
        carry = 1 if neg else 0
    return out, vs, carry


def fb_cases():
    """(name, scalar): window values exactly 512, 513, 1023, and 1023 with a carry in (v = 1024: magnitude 0 and a carry out),
    in window 0, in middle windows and in window 24; a carry into the top window 25, which a canonical scalar fills with at most
    4 and so can never make negative itself"""
    out = [("q-1", Q - 1), ("1", 1), ("2^252", 2**252)]
    for w in (0, 1, 13, 24):
        sh = FB_BITS * w
        for v in (512, 513, 1023):
            out.append((f"window {w} = {v}", v << sh))
            out.append((f"window {w} = {v}, 1 above", (v << sh) | (1 << (sh + FB_BITS))))
        if w:
            out.append((f"window {w} = 1023 with a carry in", (1023 << sh) | (513 << (sh - FB_BITS))))
            out.append((f"windows 0..{w} = 1023", (1 << (sh + FB_BITS)) - 1))
    for top in (0, 1, 3):
        out.append((f"carry into window 25 = {top}", (top << 250) | (1023 << 240)))
    out.append(("every window 513", sum(513 << (FB_BITS * w) for w in range(25))))
    out.append(("every window 512", sum(512 << (FB_BITS * w) for w in range(25))))
    assert all(0 <= s < Q for _, s in out)
    return out


def mul_scalars():
    """every scalar of digit_vectors at c = 10, then the fixed-base classes and the wnaf straddles that are canonical"""
    named = [(f"digit_vectors: {v.name}", v.s) for v in DV.edge_scalars(FB_BITS, FB_WINDOWS)] + fb_cases()
    named += [(n, s) for n, s in wnaf5_cases() if s < Q and ("straddle" in n and "ones" in n or not n.startswith(("straddle", "random")))]
    seen, out = set(), []
    for n, s in named:
        if s not in seen:
            seen.add(s)
            out.append((n, s))
    return out


# ---- the groups --------------------------------------------------------------------------------------------------------------
def _eq(got, exp, label):
    assert got == exp, f"{label}: got {got!r}, expected {exp!r}"


def _fq_group(fn, cases, inputs, expect):
    """expect(case) -> four words"""
    def check(outs):
        assert len(outs) == len(cases)
        for c, o in zip(cases, outs):
            _eq([int(w) for w in o], expect(c), f"{fn}{c!r}")
    return Group(fn, [inputs(c) for c in cases], check)


def _fe_group(fn, cases, labels, expect_value, bound):
    """cases: rows of limbs; the output's value mod p and its limb bounds"""
    def check(outs):
        assert len(outs) == len(cases)
        for c, lab, o in zip(cases, labels, outs):
            o = [int(w) for w in o]
            _eq(fe_value(o) % P, expect_value(c) % P, f"{fn} {lab}: value")
            assert within(o, bound(c)), f"{fn} {lab}: limbs {[hex(x) for x in o]} leave the bound {[hex(x) for x in bound(c)]}"
    return Group(fn, [list(c) for c in cases], check)


def _pt_group(fn, rows, labels, expect):
    """the output point against expect (a Pt), compared as compressed bytes"""
    def check(outs):
        assert len(outs) == len(rows)
        for lab, e, o in zip(labels, expect, outs):
            o = [int(w) for w in o]
            for k in range(4):
                assert within(o[5 * k:5 * k + 5], PROD_MAX) or within(o[5 * k:5 * k + 5], CARRY_MAX), f"{fn} {lab}: coordinate {k} is not carried"
            _eq(pt_of(o).encode().hex(), e.encode().hex(), f"{fn} {lab}")
    return Group(fn, rows, check)


def _flag_group(fn, rows, labels, expect):
    def check(outs):
        assert len(outs) == len(rows)
        for lab, e, o in zip(labels, expect, outs):
            _eq(int(o[0]), int(e), f"{fn} {lab}")
    return Group(fn, rows, check)


def fq_groups():
    g = OrderedDict()
    g["fq_add"] = _fq_group("fq_add", FQ_PAIRS, lambda c: words(c[0]) + words(c[1]), lambda c: words((c[0] + c[1]) % Q))
    g["fq_sub"] = _fq_group("fq_sub", FQ_PAIRS, lambda c: words(c[0]) + words(c[1]), lambda c: words((c[0] - c[1]) % Q))
    g["fq_neg"] = _fq_group("fq_neg", FQ_VALUES, words, lambda c: words(-c % Q))
    mul = FQ_MUL_PAIRS + list(zip(_rand_fq(1, 256), _rand_fq(2, 256)))
    g["fq_mul"] = _fq_group("fq_mul", mul, lambda c: words(c[0]) + words(c[1]), lambda c: words(c[0] * c[1] * RINV % Q))
    g["fq_square"] = _fq_group("fq_square", FQ_VALUES, words, lambda c: words(c * c * RINV % Q))
    g["fq_mont_reduce"] = _fq_group("fq_mont_reduce", FQ_MONT_REDUCE, lambda c: words(c, 8), lambda c: words(c * RINV % Q))
    g["fq_reduce_once"] = _fq_group("fq_reduce_once", FQ_REDUCE_ONCE, words, lambda c: words(c - Q if c >= Q else c))
    g["fq_to_bytes"] = _fq_group("fq_to_bytes", FQ_VALUES, mont, lambda c: words(c))
    kat = fq_kat()
    wide = [(x, words(x % Q * R % Q)) for x in FQ_WIDE]
    # the reference's own KATs (ristretto255.rs): 64 bytes of 0xff are Scalar::from_raw of these limbs, 2^256 - 1 of those
    wide.append((2**512 - 1, mont(unwords(int(w, 16) for w in kat["from_bytes_wide_max_raw"]))))
    wide.append((2**256 - 1, mont(unwords(int(w, 16) for w in kat["from_raw_all_ones_equiv_raw"]))))
    g["fq_from_bytes_wide"] = _fq_group("fq_from_bytes_wide", wide, lambda c: words(c[0], 8), lambda c: c[1])
    g["fq_invert"] = _fq_group("fq_invert", FQ_INVERT + _rand_fq(3, 8), mont, lambda c: mont(pow(c, Q - 2, Q)))
    g["fq_from_u64"] = _fq_group("fq_from_u64", FQ_U64, lambda c: [c], mont)
    return g


def poly_values():
    return [0, 1, Q - 1, 2, Q - 2, (Q - 1) // 2, R]


def poly_groups():
    g = OrderedDict()
    vals, rng = poly_values(), random.Random(0x9017)

    def tuples(n, extra=96):
        out = [[vals[(i + 3 * k) % len(vals)] for k in range(n)] for i in range(len(vals))] + [[v] * n for v in vals]
        return out + [[rng.randrange(Q) for _ in range(n)] for _ in range(extra)]

    def flat(xs):
        return [w for x in xs for w in mont(x)]

    def multi(fn, cases, expect):
        def check(outs):
            assert len(outs) == len(cases)
            for c, o in zip(cases, outs):
                _eq([unmont(o[4 * k:4 * k + 4]) for k in range(len(o) // 4)], [v % Q for v in expect(c)], f"{fn}{c!r}")
        return Group(fn, [flat(c) for c in cases], check)

    g["unipoly_from_evals3"] = multi("unipoly_from_evals3", tuples(3), PM.unipoly_from_evals)
    g["unipoly_from_evals4"] = multi("unipoly_from_evals4", tuples(4), PM.unipoly_from_evals)
    g["unipoly_eval3"] = multi("unipoly_eval3", tuples(4), lambda c: [PM.unipoly_eval(c[:3], c[3])])
    g["unipoly_eval4"] = multi("unipoly_eval4", tuples(5), lambda c: [PM.unipoly_eval(c[:4], c[4])])

    def combine(c):
        e, ch = list(c[:8]), c[8:]
        for r in reversed(ch):
            e = [(e[2 * i] + r * (e[2 * i + 1] - e[2 * i])) % Q for i in range(len(e) // 2)]
        return [e[0]]

    g["combine_bot3"] = multi("combine_bot3", tuples(11, 32), combine)
    g["host_eq3"] = multi("host_eq3", tuples(3, 32), PM.eq_evals)
    for batch in batch_invert_cases():   # one batch per call: the rows are its elements
        def check(outs, batch=batch):
            _eq([unmont(o) for o in outs], [pow(v, -1, Q) for v in batch], f"fq_batch_invert n={len(batch)}")
        g[f"fq_batch_invert n={len(batch)} [{batch[0] % 997}]"] = Group("fq_batch_invert", [mont(v) for v in batch], check)
    return g


def batch_invert_cases():
    """n = 1, 2, 257; 1 and q - 1 among the values (0 is outside the function's contract: 'every v[i] must be non-zero')"""
    rng = random.Random(0xB1)
    return [[Q - 1], [1], [1, Q - 1], [2, (Q + 1) // 2], [1, Q - 1, 2, R] + [rng.randrange(1, Q) for _ in range(253)]]


def fe_groups():
    g = OrderedDict()
    mul = fe_mul_cases()
    assert all(fe_mul_model(a, b)[1]["ok"] for a, b in mul)
    g["fe_mul"] = _fe_group("fe_mul", [a + b for a, b in mul], [f"#{i}" for i in range(len(mul))],
                            lambda c: fe_value(c[:5]) * fe_value(c[5:]), lambda c: PROD_MAX)
    sq = fe_square_cases()
    g["fe_square"] = _fe_group("fe_square", sq, [f"#{i}" for i in range(len(sq))], lambda c: fe_value(c) ** 2, lambda c: PROD_MAX)
    sub = fe_sub_cases()
    assert not any(fe_sub_lazy_model(a, b)[1] for a, b in sub)
    g["fe_sub"] = _fe_group("fe_sub", [a + b for a, b in sub], [f"#{i}" for i in range(len(sub))],
                            lambda c: fe_value(c[:5]) - fe_value(c[5:]), lambda c: CARRY_MAX)
    subl = fe_sub_lazy_cases()
    assert not any(fe_sub_lazy_model(a, b)[1] for a, b in subl)
    g["fe_sub_lazy"] = _fe_group("fe_sub_lazy", [a + b for a, b in subl], [f"#{i}" for i in range(len(subl))],
                                 lambda c: fe_value(c[:5]) - fe_value(c[5:]), lambda c: [x + s for x, s in zip(c[:5], SUB_BIAS)])
    addl = [(list(PROD_MAX), list(PROD_MAX)), ([2 * m for m in PROD_MAX], list(PROD_MAX)), ([0] * 5, [0] * 5), ([TOP - M51] * 5, [M51] * 5)]
    g["fe_add_lazy"] = _fe_group("fe_add_lazy", [a + b for a, b in addl], [f"#{i}" for i in range(len(addl))],
                                 lambda c: fe_value(c[:5]) + fe_value(c[5:]), lambda c: [x + y for x, y in zip(c[:5], c[5:])])
    add = addl[:2] + [(a, b) for _, a in fe_reps()[:13] for _, b in fe_reps()[4:8]]
    g["fe_add"] = _fe_group("fe_add", [a + b for a, b in add], [f"#{i}" for i in range(len(add))],
                            lambda c: fe_value(c[:5]) + fe_value(c[5:]), lambda c: CARRY_MAX)
    carry = [[x + y for x, y in zip(PROD_MAX, PROD_MAX)], [M51, M51, M51, M51, (1 << 51) + M51], [TOP] * 5, list(SUB_BIAS),
             [M64 >> 1] * 5, [0] * 5] + [l for _, l in fe_reps()]
    g["fe_carry"] = _fe_group("fe_carry", carry, [f"#{i}" for i in range(len(carry))], fe_value, lambda c: CARRY_MAX)
    reps = fe_reps()
    labels = [n for n, _ in reps]
    g["fe_neg"] = _fe_group("fe_neg", [l for n, l in reps if within(l, SUB_BIAS)], [n for n, l in reps if within(l, SUB_BIAS)],
                            lambda c: -fe_value(c), lambda c: CARRY_MAX)
    g["fe_abs"] = _fe_group("fe_abs", [l for n, l in reps if within(l, SUB_BIAS)], [n for n, l in reps if within(l, SUB_BIAS)],
                            lambda c: PG._abs(fe_value(c)), lambda c: [max(a, b) for a, b in zip(c, CARRY_MAX)])

    def to_bytes_check(outs):
        for (n, l), o in zip(reps, outs):
            _eq(unwords(o), fe_value(l) % P, f"fe_to_bytes {n}")
    g["fe_to_bytes"] = Group("fe_to_bytes", [l for _, l in reps], to_bytes_check)
    g["fe_is_negative"] = _flag_group("fe_is_negative", [l for _, l in reps], labels, [(fe_value(l) % P) & 1 for _, l in reps])
    g["fe_is_zero"] = _flag_group("fe_is_zero", [l for _, l in reps], labels, [fe_value(l) % P == 0 for _, l in reps])
    pairs = [(a, b) for a in reps for b in reps]
    g["fe_equals"] = _flag_group("fe_equals", [a[1] + b[1] for a, b in pairs], [f"{a[0]} == {b[0]}" for a, b in pairs],
                                 [(fe_value(a[1]) - fe_value(b[1])) % P == 0 for a, b in pairs])
    fb = [0, 1, P - 1, P, 2**255 - 1, 2**255, 2**255 + 5, 2**256 - 1, (P - 1) | 2**255, int.from_bytes(bytes(range(32)), "little")]

    def from_bytes_check(outs):
        for x, o in zip(fb, outs):
            _eq([int(w) for w in o], fe_limbs(x & (2**255 - 1)), f"fe_from_bytes {hex(x)}")   # bit 255 is ignored, nothing is reduced
    g["fe_from_bytes"] = Group("fe_from_bytes", [words(x) for x in fb], from_bytes_check)
    pw = FE_POW_VALUES
    g["fe_invert"] = _fe_group("fe_invert", [l for _, l in pw], [n for n, _ in pw], lambda c: pow(fe_value(c) % P, P - 2, P), lambda c: PROD_MAX)
    g["fe_pow_p58"] = _fe_group("fe_pow_p58", [l for _, l in pw], [n for n, _ in pw], lambda c: pow(fe_value(c) % P, (P - 5) // 8, P), lambda c: PROD_MAX)
    sr = sqrt_ratio_cases()

    def sqrt_check(outs):
        for (u, v, _, _), o in zip(sr, outs):
            ok, root = PG.sqrt_ratio_m1(u, v)
            got = fe_value([int(w) for w in o[1:]]) % P
            _eq((int(o[0]), got), (int(ok), root), f"sqrt_ratio_m1({u}, {v})")
            assert got & 1 == 0, f"sqrt_ratio_m1({u}, {v}): the root is negative"
    g["sqrt_ratio_m1"] = Group("sqrt_ratio_m1", [lu + lv for _, _, lu, lv in sr], sqrt_check)
    return g


def niels_cases():
    """(P as four field elements in limbs, niels entry in limbs, negq): the lazy chains of FixedBase::add_niels at their top --
    P's coordinates at a product's largest limbs, the entry carried -- and real points"""
    rng = random.Random(0x1E15)
    top, carried = list(PROD_MAX), [M51] * 5
    cases = []
    for neg in (0, 1):
        cases.append((top * 4, carried * 3, neg))
        cases.append((top * 4, list(CARRY_MAX) * 3, neg))
        cases.append(([0] * 20, carried * 3, neg))
        cases.append((top + [0] * 5 + top + [0] * 5, carried * 3, neg))
        cases.append(([0] * 5 + top + top + top, carried + [0] * 5 + carried, neg))
        for _ in range(64):
            cases.append(([rng.randrange(m + 1) for _ in range(4) for m in PROD_MAX], [rng.randrange(M51 + 1) for _ in range(15)], neg))
    return cases


def niels_chain_model(p, q, neg):
    """E, F, G, H of add_niels in limbs (the exact lazy sums), and whether a limb of a sub_lazy went below zero"""
    X, Y, Z, T = (p[5 * i:5 * i + 5] for i in range(4))
    ypx, ymx, xy2d = (q[5 * i:5 * i + 5] for i in range(3))
    under = False
    s, u = fe_sub_lazy_model(Y, X)
    under |= u
    PP, f1 = fe_mul_model([a + b for a, b in zip(Y, X)], ymx if neg else ypx)
    MM, f2 = fe_mul_model(s, ypx if neg else ymx)
    TT, f3 = fe_mul_model(T, xy2d)
    ZZ2 = [2 * z for z in Z]
    E, u = fe_sub_lazy_model(PP, MM)
    under |= u
    H = [a + b for a, b in zip(PP, MM)]
    plus = [a + b for a, b in zip(ZZ2, TT)]
    minus, u = fe_sub_lazy_model(ZZ2, TT)
    under |= u
    G, F = (minus, plus) if neg else (plus, minus)
    ok = f1["ok"] and f2["ok"] and f3["ok"] and not under
    for a, b in ((E, F), (G, H), (F, G), (E, H)):
        ok = ok and fe_mul_model(a, b)[1]["ok"]
    return dict(E=E, F=F, G=G, H=H), ok


def niels_expected(p, q, neg):
    X, Y, Z, T = (fe_value(p[5 * i:5 * i + 5]) for i in range(4))
    ypx, ymx, xy2d = (fe_value(q[5 * i:5 * i + 5]) for i in range(3))
    PP, MM = (Y + X) * (ymx if neg else ypx), (Y - X) * (ypx if neg else ymx)
    TT, ZZ2 = T * xy2d, 2 * Z
    E, H = PP - MM, PP + MM
    G, F = (ZZ2 - TT, ZZ2 + TT) if neg else (ZZ2 + TT, ZZ2 - TT)
    return [E * F % P, G * H % P, F * G % P, E * H % P]


def niels_of(pt):
    zi = pow(pt.Z, -1, P)
    x, y = pt.X * zi % P, pt.Y * zi % P
    return fe_limbs((y + x) % P) + fe_limbs((y - x) % P) + fe_limbs(2 * PG.D * x * y % P)


def point_groups():
    g = OrderedDict()
    pts = base_points()
    ident = PG.Pt.identity()
    every = [("id", ident)] + [(f"pt{i}", p) for i, p in enumerate(pts)]
    for neg in (0, 1):
        cases = [(a, b, la, lb) for a in every for b in every for la, lb in ((0, 0), (1, 2), (2, 1))]
        g[f"pt_add neg={neg}"] = _pt_group("pt_add", [pt_limbs(a[1], la) + pt_limbs(b[1], lb) + [neg] for a, b, la, lb in cases],
                                          [f"{a[0]} {'-' if neg else '+'} {b[0]} lazy {la}{lb}" for a, b, la, lb in cases],
                                          [a[1] - b[1] if neg else a[1] + b[1] for a, b, _, _ in cases])
    dbl = [(n, p, l) for n, p in every + [(f"torsion{i}", t) for i, t in enumerate(TORSION4)] for l in (0, 1, 2)]
    g["pt_dbl"] = _pt_group("pt_dbl", [pt_limbs(p, l) for _, p, l in dbl], [f"{n} lazy {l}" for n, _, l in dbl], [p + p for _, p, _ in dbl])
    # equality: the four representatives of a coset are equal to each other, P and -P are not, nor are different points
    eq_cases = []
    for n, p in every[1:6]:
        cs = coset(p)
        eq_cases += [(f"{n}+T{i} == {n}+T{j}", cs[i], cs[j], True) for i in range(4) for j in range(4)]
        eq_cases += [(f"{n}+T{i} == -{n}", cs[i], -p, False) for i in range(4)]
        eq_cases += [(f"{n} == {m}", p, o, n == m) for m, o in every]
    eq_cases += [(f"id+T{i} == id", t, ident, True) for i, t in enumerate(TORSION4)]
    g["pt_equals"] = _flag_group("pt_equals", [pt_limbs(a) + pt_limbs(b, 1) for _, a, b, _ in eq_cases], [c[0] for c in eq_cases], [c[3] for c in eq_cases])
    comp = [(f"{n}+T{i} lazy {l}", c, p) for n, p in every for i, c in enumerate(coset(p)) for l in (0, 1)]
    comp.append(("the identity as (0, 1, 1, 0) lazy 0", ident, ident))

    def compress_check(outs):
        for (lab, _, p), o in zip(comp, outs):
            _eq(unwords(o).to_bytes(32, "little").hex(), p.encode().hex(), f"pt_compress {lab}")
    g["pt_compress"] = Group("pt_compress", [pt_limbs(c, int(lab[-1])) for lab, c, _ in comp], compress_check)
    dec = decompress_all()

    def decompress_check(outs):
        for (name, s), o in zip(dec, outs):
            pt = PG.decode(s.to_bytes(32, "little"))
            _eq(int(o[0]), int(pt is not None), f"pt_decompress [{name}] {hex(s)}: accepted")
            if pt is not None:
                X, Y, Z, T = (fe_value([int(w) for w in o[1 + 5 * i:6 + 5 * i]]) % P for i in range(4))
                _eq((X, Y, Z, T), (pt.X, pt.Y, pt.Z, pt.T), f"pt_decompress [{name}] {hex(s)}")
    g["pt_decompress"] = Group("pt_decompress", [words(s) for _, s in dec], decompress_check)
    with open(os.path.join(GOLDEN, "ristretto_kat.json")) as f:
        kat = json.load(f)
    uni = [(lab, hashlib.sha512(lab.encode()).digest(), bytes.fromhex(enc)) for lab, enc in kat["hash_to_group_sha512"]]
    stream = gens_stream(6)
    uni += [(f"gens_r1cs_sat[{i}]", stream[64 * i:64 * i + 64], None) for i in range(6)]
    uni += [("all ones", b"\xff" * 64, None), ("zeros", bytes(64), None)]

    def uniform_check(outs):
        for (lab, b, enc), o in zip(uni, outs):
            exp = PG.from_uniform_bytes(b).encode()
            assert enc is None or exp == enc, lab
            _eq(pt_of([int(w) for w in o]).encode().hex(), exp.hex(), f"pt_from_uniform_bytes {lab}")
    g["pt_from_uniform_bytes"] = Group("pt_from_uniform_bytes", [words(int.from_bytes(b, "little"), 8) for _, b, _ in uni], uniform_check)
    ell = [0, 1, 2, P - 1, PG.SQRT_M1, 2**255 - 20] + [int.from_bytes(b[:32], "little") & (2**255 - 1) for _, b, _ in uni]
    g["pt_elligator"] = _pt_group("pt_elligator", [fe_limbs(t) for t in ell], [hex(t) for t in ell], [PG.elligator(t % P) for t in ell])
    rt = [(n, p, l) for n, p in every for l in (0, 1)]

    def xyzt_check(outs):
        for (n, p, l), o in zip(rt, outs):
            _eq([unwords(o[4 * i:4 * i + 4]) for i in range(4)], [p.X, p.Y, p.Z, p.T], f"pt_to_xyzt {n} lazy {l}")
    g["pt_to_xyzt"] = Group("pt_to_xyzt", [pt_limbs(p, l) for _, p, l in rt], xyzt_check)

    def from_xyzt_check(outs):
        for (n, p), o in zip(every, outs):
            _eq([int(w) for w in o], pt_limbs(p), f"pt_from_xyzt {n}")
    g["pt_from_xyzt"] = Group("pt_from_xyzt", [[w for c in (p.X, p.Y, p.Z, p.T) for w in words(c)] for _, p in every], from_xyzt_check)
    nc = niels_cases()
    assert all(niels_chain_model(*c)[1] for c in nc)

    def niels_check(outs):
        for i, (c, o) in enumerate(zip(nc, outs)):
            o = [int(w) for w in o]
            _eq([fe_value(o[5 * k:5 * k + 5]) % P for k in range(4)], niels_expected(*c), f"fb_add_niels #{i}")
            assert all(within(o[5 * k:5 * k + 5], PROD_MAX) for k in range(4)), f"fb_add_niels #{i}: limbs leave a product's bound"
    g["fb_add_niels"] = Group("fb_add_niels", [p + q + [neg] for p, q, neg in nc], niels_check)
    real = [(a, b, neg) for a in every[:5] for b in every[1:5] for neg in (0, 1)]
    g["fb_add_niels points"] = _pt_group("fb_add_niels", [pt_limbs(a[1]) + niels_of(b[1]) + [neg] for a, b, neg in real],
                                         [f"{a[0]} {'-' if neg else '+'} {b[0]}" for a, b, neg in real],
                                         [a[1] - b[1] if neg else a[1] + b[1] for a, b, neg in real])
    return g


def wnaf_groups():
    cases = wnaf5_cases()

    def check(outs):
        for (name, s), o in zip(cases, outs):
            digits, top = wnaf5_model(s)
            got = [signed(w) for w in o[1:]]
            _eq(signed(o[0]), top, f"wnaf5 {name}: top")
            _eq(got, digits, f"wnaf5 {name}: digits")
            assert sum(d << i for i, d in enumerate(got)) == s, f"wnaf5 {name}: the digits do not sum to the scalar"
            nz = [i for i, d in enumerate(got) if d]
            assert all(d == 0 or (d & 1 and abs(d) <= 15) for d in got) and all(b - a >= 5 for a, b in zip(nz, nz[1:])), name
    return OrderedDict([("wnaf5", Group("wnaf5", [words(s) for _, s in cases], check))])


_MUL_CACHE = {}


def _smul(k, key, pt):
    if (k, key) not in _MUL_CACHE:
        _MUL_CACHE[(k, key)] = k * pt
    return _MUL_CACHE[(k, key)]


def mul_groups():
    g = OrderedDict()
    B, G0 = PG.basepoint(), gens_point(0)
    other = 0x1234567 * B + B   # Z != 1
    sc = mul_scalars()
    for key, pt in (("B", B), ("gens[0]", G0), ("Z!=1", other)):
        use = sc if key == "B" else sc[::3] + fb_cases()
        g[f"pt_mul_bytes {key}"] = _pt_group("pt_mul_bytes", [pt_limbs(pt) + words(s) for _, s in use], [f"{n} * {key}" for n, s in use],
                                            [_smul(s, key, pt) for _, s in use])
    half = sc[:len(sc) // 2 * 2]
    pairs = list(zip(half[0::2], half[1::2])) + [((n, s), ("0", 0)) for n, s in sc[:8]] + [(("0", 0), (n, s)) for n, s in sc[:8]] + [(("0", 0), ("0", 0))]
    g["pt_mul2_bytes"] = _pt_group("pt_mul2_bytes", [words(a[1]) + pt_limbs(B) + words(b[1]) + pt_limbs(G0) for a, b in pairs],
                                   [f"[{a[0]}] B + [{b[0]}] gens[0]" for a, b in pairs],
                                   [_smul(a[1], "B", B) + _smul(b[1], "gens[0]", G0) for a, b in pairs])
    for key, pt in (("B", B), ("gens[0]", G0)):
        for aname, acc in (("identity", PG.Pt.identity()), ("7B", 7 * B)):
            use = sc + [("0", 0)] if aname == "identity" else fb_cases() + [("0", 0)]
            g[f"fb_mul_acc {key} onto {aname}"] = _pt_group(
                "fb_mul_acc", [pt_limbs(acc) + pt_limbs(pt) + mont(s) for _, s in use], [f"{aname} + [{n}] {key}" for n, _ in use],
                [acc + _smul(s, key, pt) for _, s in use])
    # the digits themselves, over the harness's marked table: entry [w][k] = (k + 1)(w + 1) B
    def marked(s):
        return sum(d * (w + 1) for w, d in enumerate(fb_digits(s)[0])) % Q
    g["fb_mul_acc_marked"] = _pt_group("fb_mul_acc_marked", [mont(s) for _, s in sc], [f"digits of {n}" for n, _ in sc],
                                       [_smul(marked(s), "B", B) for _, s in sc])
    return g


def groups():
    g = OrderedDict()
    for part in (fq_groups(), poly_groups(), fe_groups(), point_groups(), wnaf_groups(), mul_groups()):
        for k, v in part.items():
            assert k not in g
            g[k] = v
    return g


# ---- the vector file of tests/hostarith/hostarith_main.cpp ---------------------------------------------------------------------
def write_vector_file(path, gs):
    with open(path, "w") as f:
        for grp in gs.values():
            f.write(f"{grp.fn} {len(grp.rows)}\n")
            for row in grp.rows:
                f.write(" ".join(f"{int(w):x}" for w in row) + "\n")


def parse_output(text, gs):
    """the program's output -> {group name: rows of ints}; the blocks come in the order of the file"""
    lines = text.split("\n")
    pos, out = 0, OrderedDict()
    for name, grp in gs.items():
        assert lines[pos] == f"{grp.fn} {len(grp.rows)}", (name, lines[pos])
        out[name] = [[int(w, 16) for w in lines[pos + 1 + i].split()] for i in range(len(grp.rows))]
        pos += 1 + len(grp.rows)
    assert [l for l in lines[pos:] if l] == [], "output after the last block"
    return out
