"""Python model of the reference client's exponential ElGamal on E2 (src/LeNet/Client.py: key generation :19-41, encrypt
:121-132, decrypt and bsgs :182-243) on gadgets_model's e2_add / e2_mul, with the randomness explicit.  The baby-step table is
the reference's dict {(x, y) of j * G: j} for 0 <= j < m with j = 0 the identity (keyed None here), and the walk is its two
lock-step walks M - i (m G) and -M - i (m G).  It is checked against recorded runs of the reference's own client:
tests/golden/layer_pins.json (tests/golden/make_layer_pins.py), compared in tests/test_layer_pins.py."""
import gadgets_model as GM

Q = GM.Q
ORDER = GM.E2_ORDER
G = (GM.E2_GX, GM.E2_GY)


def neg(P):
    return None if P is None else (P[0], (Q - P[1]) % Q)


def mul(k, P=G):
    """k * P for any integer k (a negative k multiplies the negated point, as the reference's encrypt does)"""
    return GM.e2_mul(-k, neg(P)) if k < 0 else GM.e2_mul(k, P)


def keygen(sk):
    return mul(sk)


def encrypt(H, msg, r):
    """(c1, c2) = (r G, msg G + r H)"""
    return mul(r), GM.e2_add(mul(int(msg)), mul(r, H))


def baby_steps(m):
    table, P = {None: 0}, None
    for j in range(1, m):
        P = GM.e2_add(P, G)
        table[P] = j
    return table


def bsgs(table, m, M, max_giant):
    """the v with M = v G and |v| <= max_giant * m + m - 1, or None"""
    step = neg(mul(m))
    pos, ngt = M, neg(M)
    for i in range(max_giant + 1):
        if pos in table:
            return i * m + table[pos]
        if ngt in table:
            return -(i * m + table[ngt])
        pos, ngt = GM.e2_add(pos, step), GM.e2_add(ngt, step)
    return None


def decrypt(table, m, sk, c1, c2, max_giant):
    return bsgs(table, m, GM.e2_add(c2, neg(mul(sk, c1))), max_giant)


def splitmix_scalars(seed, count, lo=1, hi=ORDER):
    """count integers in [lo, hi) from four SplitMix64 words each"""
    out, st = [], seed
    for _ in range(count):
        v = 0
        for _ in range(4):
            st, z = GM.splitmix64(st)
            v = (v << 64) | z
        out.append(lo + v % (hi - lo))
    return out
