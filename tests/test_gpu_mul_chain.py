"""GPU tests of the layer tail as a stage (vpin_e2_mul_chain: e2_scalar_mul_kernel, e2_chain_scan_kernel and one
e2_to_affine_kernel launch) against the literal affine arithmetic of tests/gadgets_model.py, byte for byte: the products
s * X and the inclusive prefixes of every chain, identities flagged and written as zeros.

The prefixes are a workgroup scan in tiles of 256 with a carried prefix, so the shapes sit at the wave boundary (63, 64, 65), at
the tile boundary (255, 256, 257) and past two tiles (600), alone and as three unequal chains side by side.  A scan adds
segment sums, not single terms: the periodic patterns make two equal segment sums meet at an internal node (the doubling
case) whatever tree the scan uses, and with the sign alternating per period two opposite ones (an identity at an internal node,
and an identity prefix in mid-chain from which the chain goes on).

The scalars are small so that the model stays fast (a model addition is one modular inversion); one chain of full 128-bit
scalars runs at K = 65.  The points are consecutive multiples of one point of large logarithm: one model addition each."""
import ctypes as C

import numpy as np
import pytest

import enc_conv_model as EM
import gadgets_model as GM
from test_gpu_enc_conv import points_of, to_arrays

pytestmark = pytest.mark.gpu

Q = GM.Q
KS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 600]


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """700 distinct points D, 2 D, 3 D, ..: shared by the tests and never changed"""
    D = EM.log_point(0x9E3779B97F4A7C15F39CC0605CEDC835)
    out, acc = [], None
    for _ in range(700):
        acc = GM.e2_add(acc, D)
        out.append(acc)
    return tuple(out)


def neg(p):
    return None if p is None else (p[0], (Q - p[1]) % Q)


_products = {}


def product(s, x):
    if x is None or s == 0:
        return None
    if (s, x) not in _products:
        _products[s, x] = GM.e2_mul(s, x)
    return _products[s, x]


def model(scalars, points, P, K):
    """the left-to-right loop of the layers: T_k = s_k * X_k, acc_k = acc_{k-1} + T_k"""
    T = [product(s, x) for s, x in zip(scalars, points)]
    acc = []
    for p in range(P):
        a = None
        for k in range(K):
            a = GM.e2_add(a, T[p * K + k])
            acc.append(a)
    return T, acc


def check(ctx, scalars, points, P, K):
    x, y, inf = to_arrays(points)
    (tx, ty, ti), (ax, ay, ai) = ctx.e2_mul_chain(scalars, x, y, inf, P, K)
    T, acc = model(scalars, points, P, K)
    assert points_of(tx, ty, ti) == T, "products s * X"
    got = points_of(ax, ay, ai)
    bad = [i for i in range(P * K) if got[i] != acc[i]]
    assert not bad, f"prefixes differ first at chain {bad[0] // K}, term {bad[0] % K} ({len(bad)} of {P * K})"
    return T, acc


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_shapes(ctx, pool, K, P):
    """every chain its own points and scalars 0 .. 7: s = 0 and a flagged identity under a non-zero scalar are identity terms,
    also as the first term of a chain (the prefix starts as the identity) and as the last"""
    scalars = [(5 * p + 3 * k + k // 7) % 8 for p in range(P) for k in range(K)]
    points = [pool[(211 * p + k) % 700] for p in range(P) for k in range(K)]
    for p in range(P):
        for k in (0, 5, 64, 255, 256, K - 1):
            if k < K and (k + p) % 2 == 0:
                points[p * K + k] = None
                scalars[p * K + k] = 3
    if P == 3:  # the three chains do not start alike: chain 1 opens with s = 0, chain 2 with an ordinary term
        scalars[K], scalars[2 * K], points[2 * K] = 0, 6, pool[699]
    T, acc = check(ctx, scalars, points, P, K)
    assert T[0] is None and acc[0] is None


@pytest.mark.parametrize("K", [65, 300])
def test_all_identity_chain(ctx, pool, K):
    """chain 0: every term an identity (s = 0 and flagged points alternate), so every prefix is; chain 1 beside it is ordinary"""
    scalars = [0 if k % 2 else 4 for k in range(K)] + [1 + k % 5 for k in range(K)]
    points = [pool[k] if k % 2 else None for k in range(K)] + [pool[100 + k] for k in range(K)]
    T, acc = check(ctx, scalars, points, 2, K)
    assert all(a is None for a in acc[:K]) and all(a is not None for a in acc[K:])


PERIODS = [1, 2, 4, 8, 16, 32, 64, 128]


@pytest.mark.parametrize("K", [256, 600])
def test_periodic_terms_double_at_internal_nodes(ctx, pool, K):
    """chain i has X_k = X_{k mod m} and equal scalars for m = 2^i: two neighbouring aligned segments of m terms have equal sums,
    so some node of any scan tree adds a point to itself"""
    P = len(PERIODS)
    scalars = [3] * (P * K)
    points = [pool[17 * i + k % m] for i, m in enumerate(PERIODS) for k in range(K)]
    check(ctx, scalars, points, P, K)


@pytest.mark.parametrize("K", [256, 600])
def test_alternating_periods_cancel_in_mid_chain(ctx, pool, K):
    """the same with the sign of y alternating per block of m: neighbouring segment sums are opposite, an internal node gives the
    identity, and the prefixes at k = 2m - 1, 4m - 1, .. are the identity, from which the chain goes on"""
    P = len(PERIODS)
    scalars = [3] * (P * K)
    points = []
    for i, m in enumerate(PERIODS):
        for k in range(K):
            pt = pool[300 + 17 * i + k % m]
            points.append(neg(pt) if (k // m) % 2 else pt)
    T, acc = check(ctx, scalars, points, P, K)
    for i, m in enumerate(PERIODS):
        for k in range(2 * m - 1, K, 2 * m):
            assert acc[i * K + k] is None
        assert acc[i * K + m - 1] is not None and (2 * m >= K or acc[i * K + 2 * m] == T[i * K])


def test_two_terms_equal_and_opposite(ctx, pool):
    """K = 2: T_1 = T_0 (the addition is a doubling) and T_1 = -T_0 (the prefix is the identity); the products differ from the
    points, so equal products come from different scalars over different points too (2 * (3 D) = 3 * (2 D))"""
    D, D2, D3 = pool[0], pool[1], pool[2]
    scalars = [5, 5, 5, 5, 2, 3, 2, 3]
    points = [D, D, D, neg(D), D3, D2, D3, neg(D2)]
    T, acc = check(ctx, scalars, points, 4, 2)
    assert acc[1] == GM.e2_mul(10, D) and acc[3] is None and acc[5] == GM.e2_mul(12, D) and acc[7] is None


def test_full_width_scalars(ctx, pool):
    """one chain of K = 65 under 128-bit scalars (top bit set in the first, all ones in the second)"""
    K, st, scalars = 65, 0xC4A1, []
    for _ in range(K):
        st, a = GM.splitmix64(st)
        st, b = GM.splitmix64(st)
        scalars.append((a << 64) | b)
    scalars[0] |= 1 << 127
    scalars[1] = 2**128 - 1
    check(ctx, scalars, list(pool[400:400 + K]), 1, K)


def test_rejections(ctx, pool):
    """VPIN_EINVAL as for vpin_e2_msm: a null argument, a zero dimension, a coordinate not below q, a point off the curve"""
    import vpin_amd
    L = vpin_amd.lib()
    pts = list(pool[:6])

    def rejected(points=pts, P=2, K=3, raw=None):
        x, y, inf = raw if raw is not None else to_arrays(points)
        with pytest.raises(vpin_amd.VpinError) as ei:
            ctx.e2_mul_chain([1] * (P * K), x, y, inf, P, K)
        return ei.value.code, str(ei.value)

    off = list(pts)
    off[4] = (pts[4][0], (pts[4][1] + 1) % Q)
    code, msg = rejected(off)
    assert code == -1 and "not on the curve" in msg
    x, y, inf = to_arrays(pts)
    x[5] = np.frombuffer(Q.to_bytes(32, "little"), np.uint8)
    code, msg = rejected(raw=(x, y, inf))
    assert code == -1 and "not below q" in msg
    buf = np.zeros(6 * 32, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    args = [ctx.h, p, p, p, p, 2, 3] + [p] * 6
    for i in [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12]:
        assert L.vpin_e2_mul_chain(*[None if j == i else v for j, v in enumerate(args)]) == -1, f"argument {i} null"
    assert b"null argument" in L.vpin_last_error()
    for P, K in ((0, 3), (2, 0), (2**20, 2**11)):
        assert L.vpin_e2_mul_chain(ctx.h, p, p, p, p, P, K, *[p] * 6) == -1, (P, K)
    # the same inputs unspoilt are accepted
    check(ctx, [1, 2, 3, 4, 5, 6], pts, 2, 3)
