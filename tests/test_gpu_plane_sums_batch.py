"""GPU tests of the batched channel sums (vpin_e2_plane_sums_batch, e2_plane_sums_batch_kernel): `groups` sets of planes under one
table in one call.  Every group is compared with two references: vpin_e2_plane_sums on that group's planes alone, byte for byte,
and tests/lenet_model.py on discrete logarithms.  Shapes: a single pixel, one lane short of a wave (7 x 9), exactly a wave
(8 x 8), one lane over (5 x 13) and one pixel past a 256-lane workgroup (1 x 257); tables of one plane per row, of all planes and
with overlapping rows.  The cases of the complete addition are planted in a group between two plain ones, so that a wrong group
stride shows; every refusal comes before a launch."""
import ctypes as C

import numpy as np
import pytest

import enc_conv_model as EM
import gadgets_model as GM
import lenet_model as LM
from test_gpu_enc_conv import points_of, to_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def check(ctx, groups_logs, H, W, connect):
    """groups_logs[g][j]: the H * W logs of plane j of group g -> the batched call's output, checked against both references"""
    groups, n_in, n_out = len(groups_logs), len(groups_logs[0]), len(connect)
    x, y, inf = to_arrays(LM.logs_to_points([k for g in groups_logs for p in g for k in p]))
    ox, oy, oi = ctx.e2_plane_sums_batch(x, y, inf, groups, n_in, H, W, connect)
    assert ox.shape == (groups, n_out, H, W, 32) and oi.shape == (groups, n_out, H, W)
    per = n_in * H * W
    for g in range(groups):
        sx, sy, si = ctx.e2_plane_sums(x[g * per:(g + 1) * per], y[g * per:(g + 1) * per], inf[g * per:(g + 1) * per], n_in, H, W, connect)
        assert np.array_equal(ox[g], sx) and np.array_equal(oy[g], sy) and np.array_equal(oi[g], si), "group %d against the single call" % g
        want = LM.logs_to_points([k for p in LM.plane_sums(EM.LOGS, groups_logs[g], connect) for k in p])
        assert points_of(ox[g], oy[g], oi[g]) == want, "group %d against the model" % g
    return ox, oy, oi


def plain(seed, groups, n_in, hw):
    return [[EM.synthetic_logs(seed + 16 * g + j, hw) for j in range(n_in)] for g in range(groups)]


ONE3 = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
ALL3 = [[1, 1, 1]]
OVER3 = [[1, 1, 0], [0, 1, 1], [1, 0, 1]]
ONE6 = [[0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]]
ALL6 = [[1] * 6]
OVER6 = [[1, 1, 1, 0, 0, 0], [0, 0, 1, 1, 1, 1], [1, 0, 1, 0, 1, 0]]
SHAPES = [(1, 1, [[1]], 1, 1), (1, 3, ALL3, 8, 8), (1, 6, OVER6, 7, 9), (2, 1, [[1]] * 3, 5, 13), (2, 3, ONE3, 7, 9), (2, 6, ALL6, 8, 8),
          (2, 3, OVER3, 1, 257), (5, 1, [[1]], 8, 8), (5, 3, OVER3, 5, 13), (5, 6, OVER6, 1, 1), (5, 1, [[1]], 1, 257), (2, 6, ONE6, 5, 13)]


@pytest.mark.parametrize("groups, n_in, connect, H, W", SHAPES, ids=["g%d-in%d-out%d-%dx%d" % (s[0], s[1], len(s[2]), s[3], s[4]) for s in SHAPES])
def test_every_group_is_the_single_call_and_the_model(ctx, groups, n_in, connect, H, W):
    ox, _, _ = check(ctx, plain(0x5B00 + 256 * groups + n_in, groups, n_in, H * W), H, W, connect)
    if groups > 1:
        assert not np.array_equal(ox[0], ox[1]), "the groups hold different planes"


def test_planted_cases_of_the_complete_addition_in_the_middle_group(ctx):
    """group 1 of three, per pixel of its 3 x 2 planes: the same point in two planes (the doubling), P and -P (a flagged identity),
    an identity input pixel (skipped), the identity in every connected plane (the output is flagged), P + P + (-P), an ordinary
    sum; groups 0 and 2 are plain and come out as their own sums"""
    a = EM.synthetic_logs(0x5C0, 6)
    b = [a[0], EM.ORDER - a[1], 0, 0, a[4], EM.synthetic_logs(0x5C1, 6)[5]]
    c = EM.synthetic_logs(0x5C2, 6)
    c[3] = 0
    c[4] = EM.ORDER - a[4]
    groups = plain(0x5D0, 1, 3, 6) + [[a, b, c]] + plain(0x5E0, 1, 3, 6)
    connect = [[1, 1, 0], [1, 1, 1], [0, 1, 1]]
    ox, oy, oi = check(ctx, groups, 3, 2, connect)
    got = [points_of(ox[1][o], oy[1][o], oi[1][o]) for o in range(3)]
    assert got[0][0] == EM.log_point(2 * a[0]), "the doubling"
    assert got[0][1] is None and [int(v) for v in oi[1][0].reshape(-1)] == [0, 1, 0, 0, 0, 0], "P + (-P) is flagged, its neighbours are not"
    assert got[0][2] == EM.log_point(a[2]), "an identity pixel adds nothing"
    assert got[2][3] is None and int(oi[1][2].reshape(-1)[3]) == 1, "a row whose connected pixels are all the identity"
    assert not ox[1][2].reshape(-1, 32)[3].any() and not oy[1][2].reshape(-1, 32)[3].any(), "a flagged output is written as zeros"
    assert got[1][4] == EM.log_point(a[4]), "P + P + (-P)"
    assert not oi[0].any() and not oi[2].any(), "the plain groups have no flagged output"


def test_refusals_come_before_any_launch(ctx):
    import vpin_amd
    from vpin_amd import capi

    def einval(fn, match):
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            fn()
        assert e.value.code == -1

    pts = LM.logs_to_points(EM.synthetic_logs(0x5F0, 16))
    x, y, inf = to_arrays(pts)
    ox, oy, oi = ctx.e2_plane_sums_batch(x, y, inf, 2, 2, 2, 2, [[1, 1]])
    assert points_of(ox, oy, oi) == [GM.e2_add(pts[8 * g + i], pts[8 * g + 4 + i]) for g in range(2) for i in range(4)]
    einval(lambda: ctx.e2_plane_sums_batch(x, y, inf, 2, 2, 2, 2, [[1, 1], [0, 0]]), "vpin_e2_plane_sums_batch: a row of the connection table selects no plane")
    # one point of the second group off the curve, one coordinate not below q: the whole call fails and names itself
    bad = y.copy()
    bad[13, 0] ^= 1
    einval(lambda: ctx.e2_plane_sums_batch(x, bad, inf, 2, 2, 2, 2, [[1, 1]]), "vpin_e2_plane_sums_batch: a pixel is not on the curve")
    big = x.copy()
    big[9] = np.frombuffer(GM.Q.to_bytes(32, "little"), np.uint8)
    einval(lambda: ctx.e2_plane_sums_batch(big, y, inf, 2, 2, 2, 2, [[1, 1]]), "vpin_e2_plane_sums_batch: a coordinate is not below q")
    # dimensions, through the C ABI itself: (groups, n_in, H, W, n_out); nothing is read before they are refused
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    con = np.ones((1, 2), np.uint8)
    out = [np.zeros((8, 32), np.uint8), np.zeros((8, 32), np.uint8), np.zeros(8, np.uint8)]
    call = lambda d: L.vpin_e2_plane_sums_batch(ctx.h, p(x), p(y), p(inf), d[0], d[1], d[2], d[3], p(con), d[4], *[p(a) for a in out])
    for i in range(5):
        dims = [2, 2, 2, 2, 1]
        dims[i] = 0
        assert call(dims) == -1 and b"vpin_e2_plane_sums_batch: a dimension is zero" in L.vpin_last_error()
    for dims in ((65536, 2, 2, 2, 1), (2, 65536, 2, 2, 1), (2, 2, 2, 2, 65536), (2, 2, (1 << 24) + 1, 2, 1), (2, 2, 2, (1 << 24) + 1, 1),
                 (4, 2, 1 << 14, 1 << 14, 1),      # 4 * 2 * 2^28 = 2^31 points in
                 (4, 1, 1 << 14, 1 << 14, 2),      # .. and out
                 (65535, 65535, 1 << 24, 1 << 24, 65535)):  # a product past 2^64
        assert call(dims) == -1 and b"vpin_e2_plane_sums_batch: a dimension is out of range" in L.vpin_last_error(), dims
    args = [ctx.h, p(x), p(y), p(inf), 2, 2, 2, 2, p(con), 1] + [p(a) for a in out]
    for i in (0, 1, 2, 3, 8, 10, 11, 12):
        rc = L.vpin_e2_plane_sums_batch(*[None if j == i else v for j, v in enumerate(args)])
        assert rc == -1 and b"vpin_e2_plane_sums_batch: null argument" in L.vpin_last_error()
