"""Chosen limb patterns for the device arithmetic (fq_dev.h, fp_dev.h, fp10_dev.h, ge_tree_dev.h) and their expected values
in plain Python integers.  Nothing here depends on the code under test: tests/test_limb_vectors.py checks on the CPU that the
sets reach the places where limb arithmetic goes wrong (second wraps, full borrow chains, maximal columns, representatives at
the top of their range), and tests/test_gpu_dev_*.py run them through tests/devarith/devarith.hip.

A field element of GF(2^255-19) is any representative below 2^256 in eight 32-bit limbs; an element of F_q is canonical
(below q), and where a function multiplies, the limbs are the Montgomery form (value * 2^256 mod q)."""
import random

import pymodel_group as PG

P = 2**255 - 19
Q = 2**252 + 27742317777372353535851937790883648493
B256 = 2**256
R = B256 % Q
R2 = R * R % Q
RINV = pow(B256, -1, Q)
MASK32 = 0xFFFFFFFF
N_RANDOM = 4096


def limbs(x, n=8):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & MASK32 for i in range(n)]


def from_limbs(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def _uniq(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def _seeds(top_limb, modulus):
    s = [0, 1, 2]
    s += [MASK32 << (32 * i) for i in range(7)] + [top_limb << 224]            # one limb all ones, the top one capped
    s += [min((1 << (32 * k)) - 1, (top_limb << 224) | ((1 << 224) - 1)) for k in range(1, 9)]  # low k limbs all ones
    s += [2**252 - 1, 2**252, 2**252 + 1, modulus - 2, modulus - 1, B256 % modulus, B256 * B256 % modulus]
    return s


FQ_SEEDS = _uniq(_seeds(0x0FFFFFFF, Q))
FP_SEEDS = _uniq(_seeds(MASK32, P) + [Q - 2, Q - 1, R, R2] + [
    18, 19, 37, 38, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**255 - 1, 2**255, B256 - 39, B256 - 38, B256 - 1])
assert all(0 <= x < Q for x in FQ_SEEDS) and all(0 <= x < B256 for x in FP_SEEDS)


def pairs(seeds, bound, seed):
    """the full cross product of the seed set, then N_RANDOM seeded random pairs below bound"""
    rng = random.Random(seed)
    return [(a, b) for a in seeds for b in seeds] + [(rng.randrange(bound), rng.randrange(bound)) for _ in range(N_RANDOM)]


FQ_PAIRS = pairs(FQ_SEEDS, Q, 0xF9)
FP_PAIRS = pairs(FP_SEEDS, B256, 0xF25519)


# ---- GF(2^255-19), eight limbs: how many times 2^256 is folded --------------------------------------------------------------
def fp_add_wraps(a, b):
    """0: no carry out of limb 7; 1: one fold of 38; 2: the fold itself carries out again"""
    t = a + b
    if t < B256:
        return 0
    return 2 if (t - B256) + 38 >= B256 else 1


def fp_sub_borrows(a, b):
    d = a - b
    if d >= 0:
        return 0
    return 2 if (d + B256) - 38 < 0 else 1


def fp_mul_fold_carry(a, b):
    """the carry c that fp_mul hands to its last fold: (low half + 38 * high half) >> 256"""
    full = a * b
    return ((full % B256) + 38 * (full >> 256)) >> 256


FP_MUL_MAX_FOLD_CARRY = 38  # lo + 38 hi < 39 * 2^256; (2^32 - 1) 2^224 times 2^256 - 39 gets there, (2^256 - 1)^2 gives 37


def fp_range(a):
    return 0 if a < P else 1 if a < 2 * P else 2


FP_FREEZE_EDGES = [0, 18, 19, 37, 38, P - 1, P, P + 1, 2**255 - 1, 2**255, 2 * P - 1, 2 * P, 2 * P + 1, B256 - 1]
FP_SMALL = [1, 38, 121666, 2**31 - 1]


# ---- F_q -------------------------------------------------------------------------------------------------------------------
def fq_mont_mul(a, b):
    return a * b * RINV % Q


FQ_COND_SUB_INPUTS = _uniq([a + b for a, b in FQ_PAIRS[:len(FQ_SEEDS) ** 2]])  # every t < 2q that fq_add can hand over


def fqw_cases():
    """(list of 1..7 operand pairs); expected value: sum of a b R^-1 mod q"""
    rng = random.Random(0xACC)
    cases = [[(Q - 1, Q - 1)] * n for n in range(1, 8)]
    cases += [[(a, b)] for a in (0, 1, Q - 1, 2**252 - 1) for b in (0, 1, 2, Q - 1, R)]
    cases += [[(FQ_SEEDS[(i + 3 * k) % len(FQ_SEEDS)], FQ_SEEDS[(5 * i + k) % len(FQ_SEEDS)]) for k in range(1 + i % 7)]
              for i in range(2 * len(FQ_SEEDS))]
    cases += [[(rng.randrange(Q), rng.randrange(Q)) for _ in range(1 + i % 7)] for i in range(256)]
    return cases


def fqw_sum(case):
    return sum(a * b for a, b in case)


def fq_const_cases():
    """(d, [T_0..T_7]): any canonical constants; expected sum d_i T_i mod q"""
    rng = random.Random(0xC0)
    top = [Q - 1] * 8
    cases = [(Q - 1, top), (2**252 - 1, top), (0, top), (1, top), (Q - 1, [0] * 8), (Q - 1, [1] * 8), (1, [1] + [0] * 7)]
    cases += [(d, [t] * 8) for d in FQ_SEEDS for t in (1, 2**252 - 1, Q - 1, R)]
    cases += [(d, [FQ_SEEDS[(i + j) % len(FQ_SEEDS)] for j in range(8)]) for i, d in enumerate(FQ_SEEDS)]
    cases += [(rng.randrange(Q), [rng.randrange(Q) for _ in range(8)]) for _ in range(512)]
    # small constants against a few set limbs of d: S stays far below 2^252 or just above it (both sides of the borrow)
    cases += [(1 << (32 * i), [1 << sh] * 8) for i in range(8) for sh in (0, 27, 28, 29, 220, 251)]
    return cases


def fq_const_S(d, T):
    return sum(w * t for w, t in zip(limbs(d), T))


FQ_C = Q - 2**252


def fq_const_borrows(d, T):
    """does S_lo - (S >> 252) c go below zero (then q is added back)"""
    S = fq_const_S(d, T)
    return (S & (2**252 - 1)) < (S >> 252) * FQ_C


WINDOW_SHAPES = [(c, (253 + c - 1) // c, (253 + c - 1) // c) for c in (9, 10, 11, 12)]  # msm_pip.hip: equal windows
WINDOW_SHAPES += [(c, 253 // c + 1, 254 - c - (253 // c) * (c - 1)) for c in range(4, 14)]  # msm_var.hip: c, then c - 1 bits


def window_widths(c, W, wide):
    return [c if w < wide else c - 1 for w in range(W)]


def window_scalars(c, W, wide):
    """0, 1, q - 1, all-ones windows, and every window in turn exactly at and just past half"""
    ws = window_widths(c, W, wide)
    offs = [sum(ws[:w]) for w in range(W)]
    out = [0, 1, Q - 1, 2**252 - 1, 2**252]
    out += [s for s in (sum(((1 << ws[w]) - 1) << offs[w] for w in range(0, W, 2)), sum(((1 << ws[w]) - 1) << offs[w] for w in range(1, W, 2)))]
    for w in range(W):
        half = 1 << (ws[w] - 1)
        out += [half << offs[w], (half + 1) << offs[w], (half - 1) << offs[w], sum(((1 << (x - 1)) + 1) << o for x, o in zip(ws[:w + 1], offs))]
    return _uniq([s % Q for s in out])


# ---- GF(2^255-19), ten limbs -------------------------------------------------------------------------------------------------
FE10_EXP = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
FE10_1X = [(1 << 26) - 1 if i % 2 == 0 else (1 << 25) + (1 << 17) - 1 for i in range(10)]  # the largest limb that is still 1x
FE10_SUB_BIAS = [0x7FFFFDA] + [0x3FFFFFE if i & 1 else 0x7FFFFFE for i in range(1, 10)]   # 2p in the ten-limb form


def fe10_value(v):
    return sum(int(x) << e for x, e in zip(v, FE10_EXP))


def fe10_split(a):
    """the bit slices fe10_from_fp takes of a < 2^256: limb 9 is bits 230..255"""
    return [(a >> FE10_EXP[i]) & ((1 << (FE10_EXP[i + 1] - FE10_EXP[i])) - 1) for i in range(9)] + [a >> 230]


def fe10_max(x):
    return [x * (m + 1) - 1 for m in FE10_1X]


def fe10_is_1x(v):
    return all(0 <= int(x) <= m for x, m in zip(v, FE10_1X))


def fe10_column_max(f, g):
    """the largest column of the schoolbook product as fe10_mul adds it up"""
    best = 0
    for k in range(10):
        s = 0
        for i in range(10):
            j = (k - i) % 10
            s += f[i] * (2 if (i & 1) and (j & 1) else 1) * g[j] * (19 if i + j >= 10 else 1)
        best = max(best, s)
    return best


def fe10_mul_cases():
    rng = random.Random(0x10)
    f4, g3, z = fe10_max(4), fe10_max(3), [0] * 10
    cases = [(f4, g3), (f4, fe10_max(1)), (fe10_max(1), g3), (z, g3), (f4, z)]
    for i in range(10):
        cases += [([f4[k] if k == i else 0 for k in range(10)], g3), (f4, [g3[k] if k == i else 0 for k in range(10)])]
        cases += [([f4[k] if k == i else 0 for k in range(10)], [g3[k] if k == j else 0 for k in range(10)]) for j in range(10)]
    cases += [([rng.randrange(m + 1) for m in FE10_1X], [rng.randrange(m + 1) for m in FE10_1X]) for _ in range(1024)]
    cases += [([rng.randrange(m + 1) for m in f4], [rng.randrange(m + 1) for m in g3]) for _ in range(1024)]
    return cases


def fe10_sub_cases():
    """a zero first operand against the second at each limb's 1x maximum, alone and all together; then random 1x pairs"""
    rng = random.Random(0x5B)
    z = [0] * 10
    cases = [(z, [FE10_1X[k] if k == i else 0 for k in range(10)]) for i in range(10)] + [(z, list(FE10_1X)), (z, z)]
    cases += [([rng.randrange(m + 1) for m in fe10_max(2)], [rng.randrange(m + 1) for m in FE10_1X]) for _ in range(256)]
    return cases


# ---- points ------------------------------------------------------------------------------------------------------------------
def _short_vector(c, bound):
    """(k, m) with m = k c mod p, 0 < k, 0 <= m, both below bound: Lagrange-Gauss on the lattice of (1, c) and (0, p), then a
    small combination of the reduced basis with both signs right"""
    u, v = (1, c % P), (0, P)
    n2 = lambda w: w[0] * w[0] + w[1] * w[1]
    if n2(u) > n2(v):
        u, v = v, u
    while True:
        m = (u[0] * v[0] + u[1] * v[1] + n2(u) // 2) // n2(u)
        v = (v[0] - m * u[0], v[1] - m * u[1])
        if n2(v) >= n2(u):
            break
        u, v = v, u
    for span in range(1, 65):
        for i in range(-span, span + 1):
            for j in range(-span, span + 1):
                k, m = i * u[0] + j * v[0], i * u[1] + j * v[1]
                if 0 < k < bound and 0 <= m < bound:
                    assert (k * c - m) % P == 0
                    return k, m
    raise AssertionError("no short vector with both signs right")


COORDS = "XYZT"
_PARTNER = {"X": "Y", "Y": "X", "Z": "T", "T": "Z"}


def high_limb9_rep(pt, which):
    """pt's coordinates (a projective rescaling of the same point) as four representatives below 2^256 such that the ten-limb
    form of coordinate `which` has limb 9 = 2^26 - 1 (it is 2p - k) while its partner's limb 9 is 0 (it is below 2^230)"""
    co = dict(X=pt.X, Y=pt.Y, Z=pt.Z, T=pt.T)
    partner = _PARTNER[which]
    if co[which] == 0:  # nothing to scale: 0 = 2p as it stands
        rep = dict(co)
        rep[which] = 2 * P
    else:
        c = (-co[partner]) * pow(co[which], -1, P) % P
        k, m = _short_vector(c, 1 << 200)
        lam = (-k) * pow(co[which], -1, P) % P
        rep = {n: co[n] * lam % P for n in COORDS}
        assert rep[which] == P - k and rep[partner] == m
        rep[which] = 2 * P - k
    assert fe10_split(rep[which])[9] == (1 << 26) - 1 and fe10_split(rep[partner])[9] == 0
    assert rep["X"] * rep["Y"] % P == rep["Z"] * rep["T"] % P
    return [rep[n] for n in COORDS]


def base_points():
    """a few valid points: multiples of the basepoint and two sums that leave Z != 1"""
    B = PG.basepoint()
    return [B, 2 * B, 7 * B + 3 * B, (Q - 1) * B, 0x1234567 * B + B]


def edge_points():
    """(label, [X, Y, Z, T] representatives, Pt): the identity as (2p, 1, 1, 0) and (p, 1, 1, 0), then every base point with each
    coordinate in turn at the top of its range"""
    out = [("id-2p", [2 * P, 1, 1, 0], PG.Pt.identity()), ("id-p", [P, 1, 1, 0], PG.Pt.identity()),
           ("id-T2p", [0, 1, 1, 2 * P], PG.Pt.identity()), ("id-all", [2 * P, 2 * P + 1, P + 1, 2 * P], PG.Pt.identity())]
    for n, pt in enumerate(base_points()):
        for which in COORDS:
            out.append((f"pt{n}-{which}", high_limb9_rep(pt, which), pt))
    return out


def plain_points():
    """(label, representatives, Pt) with canonical coordinates, and with p added where it fits"""
    out = []
    for n, pt in enumerate(base_points()):
        out.append((f"pt{n}", [pt.X, pt.Y, pt.Z, pt.T], pt))
        out.append((f"pt{n}+p", [pt.X + P, pt.Y + P, pt.Z + P, pt.T + P], pt))
    return out


def point_words(rep):
    return [w for x in rep for w in limbs(x)]


def niels_words(pt):
    zi = pow(pt.Z, -1, P)
    x, y = pt.X * zi % P, pt.Y * zi % P
    return point_words([(y + x) % P, (y - x) % P, 2 * PG.D * x * y % P])


def cached_words(rep):
    X, Y, Z, T = rep
    return point_words([(Y + X) % P, (Y - X) % P, Z % P, 2 * PG.D * T % P])


def top_rep(v):
    """the largest representative of v below 2^256: v + 2p for v < 38, else v + p (bit 255 set: limb 9 of the ten-limb form is
    2^25 or more, and 2^26 - 1 for the first kind and for -k with a small k)"""
    v %= P
    return v + 2 * P if v + 2 * P < B256 else v + P


def niels_words_top(pt):
    """the affine table entry of pt with every element at its largest representative (table entries are weakly reduced)"""
    zi = pow(pt.Z, -1, P)
    x, y = pt.X * zi % P, pt.Y * zi % P
    return point_words([top_rep(y + x), top_rep(y - x), top_rep(2 * PG.D * x * y)])


def cached_top_cases():
    """(label, words of (Y+X, Y-X, Z, 2dT), Pt): cached entries of projective rescalings chosen so that Y+X = -k for a small k,
    written as 2p - k (limb 9 = 2^26 - 1), the other three elements at their largest representatives"""
    out = []
    for n, pt in enumerate([PG.Pt.identity()] + base_points()):
        for k in (1, 5, 1 << 200):
            lam = (-k) * pow(pt.Y + pt.X, -1, P) % P
            X, Y, Z, T = (c * lam % P for c in (pt.X, pt.Y, pt.Z, pt.T))
            entry = [top_rep(Y + X), top_rep(Y - X), top_rep(Z), top_rep(2 * PG.D * T)]
            assert entry[0] == 2 * P - k and fe10_split(entry[0])[9] == (1 << 26) - 1
            out.append((f"cached{n}-k{k.bit_length()}", point_words(entry), pt))
    return out


def affine(pt):
    zi = pow(pt.Z, -1, P)
    return pt.X * zi % P, pt.Y * zi % P


def affine_of_words(ws):
    """(x, y) of an extended point given as 32 words, and whether X Y == Z T"""
    X, Y, Z, T = (from_limbs(ws[8 * i:8 * i + 8]) for i in range(4))
    zi = pow(Z, -1, P)
    return (X * zi % P, Y * zi % P), (X * Y - Z * T) % P == 0
