"""Chosen scalars for the signed-digit recoding of the multi-window table walks (vpin_amd/csrc/msm.hip) and the recoders
themselves restated in plain Python integers.  Nothing here depends on the code under test: tests/test_digit_vectors.py
checks on the CPU that every vector is what its name says and that the set separates the carry rule of carry_into from its
plausible mistakes; tests/test_gpu_msm_digits.py and tests/test_gpu_msm_strip.py run the vectors through the kernels.

A scalar s of F_q is first folded (fq_fold_sign: s -> q - s when bit 251 or 252 is set, the sign of every digit flipped), then
cut into W = ceil(254 / c) windows of c bits.  A window value v = digit + carry above half = 2^(c-1) becomes the negative
digit v - 2^c with a carry into the next window; exactly half stays positive.  Two forms exist on the device:
    recode_walk   the sequential loop of table_mul_acc, either accumulator (one lane walks all windows),
    recode_lanes  table_mul_acc_range: eight lanes of wpg = ceil(W / 8) windows each, the carry into a lane's first window
                  rebuilt by carry_into -- the nearest lower digit that is not exactly half decides."""
from collections import namedtuple

Q = 2**252 + 27742317777372353535851937790883648493
FOLD = 1 << 251          # fq_fold_sign folds from here on: the top limb is at least 0x08000000
LANES = 8
WIDTHS = range(6, 15)    # every window width gens_build_once can choose (fit: 6 bits at the least, VPIN_GENS_CMAX 14 at the most)


def windows(c):
    return (254 + c - 1) // c


def lane_windows(W):
    return (W + LANES - 1) // LANES


def fold(s):
    """fq_fold_sign: (folded scalar, flip)"""
    return (Q - s, True) if s >= FOLD else (s, False)


def scalar_digit(s, w, c):
    """digit w of c bits as scalar_digit reads it: two 32-bit limbs, nothing above limb 7"""
    off = w * c
    word, sh = off >> 5, off & 31
    lo = (s >> (32 * word)) & 0xFFFFFFFF if word < 8 else 0
    hi = (s >> (32 * (word + 1))) & 0xFFFFFFFF if word + 1 < 8 else 0
    return (((hi << 32) | lo) >> sh) & ((1 << c) - 1)


def recode_walk(s, c, W):
    """table_mul_acc: (W signed digits, the carry the top window leaves)"""
    s, flip = fold(s)
    mask, half = (1 << c) - 1, 1 << (c - 1)
    carry, out = 0, []
    for _ in range(W):
        v = (s & mask) + carry
        s >>= c
        neg = v > half
        mag = (mask + 1) - v if neg else v
        carry = 1 if neg else 0
        out.append(-mag if neg != flip else mag)
    return out, carry


def carry_into(s, w0, c):
    """the carry into window w0 of an already folded scalar"""
    half = 1 << (c - 1)
    for w in range(w0 - 1, -1, -1):
        d = scalar_digit(s, w, c)
        if d != half:
            return 1 if d > half else 0
    return 0


# the three plausible mistakes (tests/test_digit_vectors.py: the vector set tells each of them from carry_into at every lane boundary)
def carry_nearest_only(s, w0, c):
    """looks at the digit below only; a digit of exactly half then never carries"""
    return 1 if w0 > 0 and scalar_digit(s, w0 - 1, c) > (1 << (c - 1)) else 0


def carry_half_carries(s, w0, c):
    """>= for >: the digit below decides, and exactly half counts as a carry"""
    return 1 if w0 > 0 and scalar_digit(s, w0 - 1, c) >= (1 << (c - 1)) else 0


def carry_run_to_zero_carries(s, w0, c):
    """a run of half digits that reaches window 0 taken for a carry"""
    half = 1 << (c - 1)
    for w in range(w0 - 1, -1, -1):
        d = scalar_digit(s, w, c)
        if d != half:
            return 1 if d > half else 0
    return 1 if w0 > 0 else 0


WRONG_CARRY_RULES = (carry_nearest_only, carry_half_carries, carry_run_to_zero_carries)


def recode_lanes(s, c, W, rule=carry_into):
    """table_mul_acc_range over the eight lanes of msm_wide_kernel / bullet_step_kernel / single_base_mul_kernel:
    (W signed digits, the carry the last window leaves)"""
    s, flip = fold(s)
    full, half = 1 << c, 1 << (c - 1)
    wpg = lane_windows(W)
    out, carry = [], 0
    for lane in range(LANES):
        w0, w1 = lane * wpg, min(lane * wpg + wpg, W)
        if w0 >= w1:
            continue
        carry = rule(s, w0, c)
        for w in range(w0, w1):
            v = scalar_digit(s, w, c) + carry
            neg = v > half
            mag = full - v if neg else v
            carry = 1 if neg else 0
            out.append(-mag if neg != flip else mag)
    return out, carry


def lane_boundaries(c, W):
    """first windows of the lanes 1.. whose windows below lie under bit 251 (c * b <= 250): there any digit pattern is a scalar"""
    wpg = lane_windows(W)
    return [b for b in range(wpg, W, wpg) if c * b <= 250]


# name: says what the vector is; s: the scalar; flip: whether fq_fold_sign folds it; folded: the scalar after the fold;
# digits: {window: digit} of the folded scalar, every window not named being zero (None where the name promises no digits);
# boundary: the lane boundary the vector was built for (None: none)
Vec = namedtuple("Vec", "name s flip folded digits boundary")


def _from_digits(digits, c):
    return sum(d << (c * w) for w, d in digits.items())


def edge_scalars(c, W):
    """the named vectors for a table of W windows of c bits, duplicates of value removed (the first name stays)"""
    half, mask = 1 << (c - 1), (1 << c) - 1
    wpg = lane_windows(W)
    nfull = 251 // c   # windows that lie wholly below bit 251
    built = []         # (name, digits, boundary)

    def add(name, digits, boundary=None):
        digits = {w: d for w, d in digits.items() if d}
        built.append((name, digits, boundary))

    add("1", {0: 1})
    add("half", {0: half})
    add("half+1", {0: half + 1})
    add("2^c-1", {0: mask})
    add("2^c", {1: 1})
    add("every digit below bit 251 = half", {w: half for w in range(nfull)})
    add("every digit below bit 251 = half+1", {w: half + 1 for w in range(nfull)})
    top, rest = divmod(250, c)
    ones = {w: mask for w in range(top)}
    ones[top] = (1 << rest) - 1
    add("2^250-1", ones)
    for b in lane_boundaries(c, W):
        for k in sorted({1, 2, wpg}):
            lo = b - k   # the run of half digits covers windows lo .. b-1
            if lo < 1:
                continue
            run = {w: half for w in range(lo, b)}
            for below, word in ((half + 1, "carry in"), (half - 1, "no carry in")):
                d = dict(run)
                d[lo - 1] = below
                d[b] = 1   # c * b <= 250: it always fits
                add(f"b={b}: run of {k} half below the boundary, {word} from window {lo - 1}, 1 in window {b}", d, b)
        run0 = {w: half for w in range(b)}
        add(f"b={b}: half from window 0 up to the boundary, nothing below", run0, b)
        run0 = dict(run0)
        run0[b] = 1
        add(f"b={b}: half from window 0 up to the boundary, nothing below, 1 in window {b}", run0, b)

    out = []
    for name, digits, boundary in built:
        v = _from_digits(digits, c)
        assert 0 < v < FOLD, name
        out.append(Vec(name, v, False, v, digits, boundary))
    # the fold: the values around the threshold and the only folded values that reach bit 251
    for name, s in (("(q-1)/2", (Q - 1) // 2), ("(q+1)/2", (Q + 1) // 2), ("2^251-1", FOLD - 1), ("2^251", FOLD), ("2^251+1", FOLD + 1),
                    ("q-2^251", Q - FOLD), ("q-2^251+1", Q - FOLD + 1), ("q-1", Q - 1)):
        flip = s >= FOLD
        out.append(Vec(name, s, flip, Q - s if flip else s, None, None))
    # the same digits behind the fold, every sign flipped
    for v in list(out):
        s = Q - v.s
        flip = s >= FOLD
        out.append(Vec(f"q - [{v.name}]", s, flip, Q - s if flip else s, v.digits if flip else None, v.boundary if flip else None))
    seen, uniq = set(), []
    for v in out:
        if v.s not in seen:
            seen.add(v.s)
            uniq.append(v)
    return uniq


def values(c, W):
    return [v.s for v in edge_scalars(c, W)]
