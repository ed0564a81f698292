"""e2_dev.h on the GPU through tests/devarith/devarith.hip: Jacobian triples with Z != 1 through every branch of the complete
additions, the Fermat and block inversions, the block tree and the scalar products, exact against gadgets_model.py's affine
integer group law."""
import random

import pytest

import devarith_lib as D
import gadgets_model as GM
import limb_vectors as V

pytestmark = pytest.mark.gpu
Q, R, RINV = V.Q, V.R, V.RINV
mont = lambda x: x * R % Q
A = V.limbs(mont(GM.E2_A))
PTS = GM.synthetic_points(0xE2, 12)
ZS = [1, 2, Q - 1, 0x123456789ABCDEF, 2**252 - 1, R]


def neg(p):
    return None if p is None else (p[0], (-p[1]) % Q)


def jac(p, z):
    """affine point (or None) as Montgomery-form Jacobian words with the given Z"""
    if p is None:
        return V.limbs(mont(z)) + V.limbs(mont(z + 1)) + V.limbs(0)  # any X, Y with Z = 0
    return V.limbs(mont(p[0] * z * z)) + V.limbs(mont(p[1] * z * z * z)) + V.limbs(mont(z))


def aff(p):
    return V.limbs(mont(p[0])) + V.limbs(mont(p[1]))


def to_affine(o):
    X, Y, Z = (V.from_limbs(o[8 * i:8 * i + 8]) * RINV % Q for i in range(3))
    assert all(V.from_limbs(o[8 * i:8 * i + 8]) < Q for i in range(3)), "a coordinate is not canonical"
    if Z == 0:
        return None
    zi = pow(Z, -1, Q)
    return X * zi * zi % Q, Y * zi * zi * zi % Q


def test_e2_dbl():
    cases = [(p, z) for p in PTS[:6] for z in ZS] + [(None, 5)]
    out = D.run("e2_dbl", [jac(p, z) + A for p, z in cases], 24)
    assert [to_affine(o) for o in out] == [GM.e2_add(p, p) for p, z in cases]


def add_cases():
    P0, P1, P2 = PTS[0], PTS[1], PTS[2]
    cases = []
    for z1 in ZS:
        for z2 in ZS[1:4]:
            cases += [(None, z1, P1, z2), (P0, z1, None, z2), (None, z1, None, z2),   # identity on either side
                      (P0, z1, P0, z2), (P0, z1, neg(P0), z2),                        # P + P and P + (-P), different Z
                      (P0, z1, P1, z2), (P2, z1, P1, z2), (GM.e2_add(P0, P0), z1, P0, z2)]
    return cases


def test_e2_add_every_branch():
    cases = add_cases()
    out = D.run("e2_add", [jac(p, z1) + jac(q, z2) + A for p, z1, q, z2 in cases], 24)
    for (p, z1, q, z2), o in zip(cases, out):
        assert to_affine(o) == GM.e2_add(p, q), (p, z1, q, z2)


def test_e2_add_mixed_every_branch():
    cases = [(p, z1, q) for p, z1, q, z2 in add_cases() if q is not None]
    out = D.run("e2_add_mixed", [jac(p, z1) + aff(q) + A for p, z1, q in cases], 24)
    for (p, z1, q), o in zip(cases, out):
        assert to_affine(o) == GM.e2_add(p, q), (p, z1, q)


def test_e2_fq_inv():
    xs = [1, 2, Q - 1, 2**252 - 1, R]
    got = D.ints(D.run("e2_fq_inv", [V.limbs(mont(x)) for x in xs], 8))
    assert got == [mont(pow(x, -1, Q)) for x in xs]


def test_e2_block_inverse():
    rng = random.Random(0xB1)
    xs = [1, Q - 1, 2, R] + [rng.randrange(1, Q) for _ in range(252)]
    got = D.ints(D.run("e2_block_inverse", [[w for x in xs for w in V.limbs(mont(x))]], 8 * 256).reshape(256, 8))
    assert got == [mont(pow(x, -1, Q)) for x in xs]


def test_e2_block_tree_with_repeats_and_cancelling_pairs():
    rng = random.Random(0xB2)
    pts = []
    for i in range(256):
        k = i % 16
        p = PTS[k % len(PTS)] if k < 12 else None
        if i % 32 >= 16:
            p = neg(p)           # lane i + 16 holds the negative of lane i: they meet at the level of width 16
        pts.append((p, rng.randrange(1, Q)))
    for i in (3, 40, 77, 200, 201, 255):
        pts[i] = (PTS[5], rng.randrange(1, Q))   # repeats that leave a sum other than the identity
    out = D.run("e2_block_tree", [[w for p, z in pts for w in jac(p, z)] + A], 24)
    total = None
    for p, z in pts:
        total = GM.e2_add(total, p)
    assert total is not None and to_affine(out[0]) == total


@pytest.mark.parametrize("nb", [128, 32])
def test_e2_mul_affine(nb):
    scalars = [1, 2, 1 << (nb - 1), (1 << nb) - 1, 0, 0x9E3779B9 if nb == 32 else 0x9E3779B97F4A7C15F39CC0605CEDC835]
    cases = [(p, s) for p in PTS[:3] for s in scalars]
    words = lambda s: ([0, 0, 0, s] if nb == 32 else V.limbs(s, 4)) + [nb]
    out = D.run("e2_mul_affine", [aff(p) + words(s) + A for p, s in cases], 24)
    for (p, s), o in zip(cases, out):
        assert to_affine(o) == GM.e2_mul(s, p), (p, hex(s))


def test_e2_mul_affine256():
    scalars = [1, 2, 1 << 255, (1 << 256) - 1, 0, GM.E2_ORDER - 1, GM.E2_ORDER, GM.E2_ORDER + 1]
    cases = [(p, s) for p in PTS[:3] for s in scalars]
    out = D.run("e2_mul_affine256", [aff(p) + V.limbs(s) + A for p, s in cases], 24)
    for (p, s), o in zip(cases, out):
        assert to_affine(o) == GM.e2_mul(s, p), (p, hex(s))
