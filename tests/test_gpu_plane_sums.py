"""GPU tests of the channel sums (vpin_e2_plane_sums, e2_plane_sum_kernel) against tests/lenet_model.py and against what the
reference's secondConv handed to its convolution (tests/golden/inference_pins.json): the 3-row and the 16-row connection table,
a launch past one workgroup, the cases of the complete addition and every rejection.  Inputs are points of known discrete
logarithm, so every expected point is one fixed-base multiplication of the model."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import enc_conv_model as EM
import gadgets_model as GM
import lenet_model as LM
from test_gpu_enc_conv import points_of, to_arrays

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "inference_pins.json")) as f:
    PINS = json.load(f)
SK = PINS["sk"]


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def run(ctx, planes_logs, H, W, connect):
    """planes of logs through the kernel -> per output plane the list of (x, y) / None"""
    pts = LM.logs_to_points([k for p in planes_logs for k in p])
    x, y, inf = to_arrays(pts)
    ox, oy, oi = ctx.e2_plane_sums(x, y, inf, len(planes_logs), H, W, connect)
    assert ox.shape == (len(connect), H, W, 32) and oi.shape == (len(connect), H, W)
    return [points_of(ox[o], oy[o], oi[o]) for o in range(len(connect))]


def expect(planes_logs, connect):
    return [LM.logs_to_points(p) for p in LM.plane_sums(EM.LOGS, planes_logs, connect)]


def digest(planes):
    raw = b"".join(b"\0" * 64 if p is None else p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big") for pl in planes for p in pl)
    return dict(n=sum(len(pl) for pl in planes), sha256=hashlib.sha256(raw).hexdigest())


@pytest.mark.parametrize("which", [0, 1])
def test_second_conv_tables_against_the_reference_run(ctx, which):
    """6 planes of 6 x 6 under the reference's table, 3 rows and all 16: the sums its secondConv computed"""
    case, inp = PINS["second_conv"][which], PINS["second_conv_input"]
    c1 = [[r % EM.ORDER for r in rs] for rs in inp["r"]]
    c2 = [[(m + r * SK) % EM.ORDER for m, r in zip(ms, rs)] for ms, rs in zip(inp["messages"], inp["r"])]
    got1, got2 = run(ctx, c1, 6, 6, case["connect"]), run(ctx, c2, 6, 6, case["connect"])
    assert got1 == expect(c1, case["connect"]) and got2 == expect(c2, case["connect"])
    assert digest([p for pair in zip(got1, got2) for p in pair]) == case["sums"]


def logs(seed, n):
    return EM.synthetic_logs(seed, n)


def test_300_lanes_and_a_single_plane_row(ctx):
    """3 outputs x 100 pixels: a partial second workgroup; the row that selects one plane returns it unchanged"""
    planes = [logs(0x100 + j, 100) for j in range(4)]
    connect = [[1, 0, 1, 1], [0, 0, 1, 0], [1, 1, 1, 1]]
    got = run(ctx, planes, 10, 10, connect)
    assert got == expect(planes, connect)
    assert got[1] == LM.logs_to_points(planes[2])


def test_complete_addition_cases(ctx):
    """per pixel of a 3 x 2 plane: the same point in two planes (the doubling), P and -P (a flagged identity, the other pixels
    right), an identity input pixel, the identity in every plane, P + P + (-P), and an ordinary sum"""
    a = logs(0x200, 6)
    b = [a[0], EM.ORDER - a[1], 0, 0, a[4], logs(0x201, 6)[5]]
    c = logs(0x202, 6)
    c[3] = 0
    c[4] = EM.ORDER - a[4]
    x, y, inf = to_arrays(LM.logs_to_points(a + b + c))
    assert list(inf) == [0] * 8 + [1, 1] + [0] * 5 + [1] + [0, 0]
    connect = [[1, 1, 0], [1, 1, 1], [0, 1, 1]]
    ox, oy, oi = ctx.e2_plane_sums(x, y, inf, 3, 3, 2, connect)
    got = [points_of(ox[o], oy[o], oi[o]) for o in range(3)]
    assert got == expect([a, b, c], connect)
    assert got[0][0] == EM.log_point(2 * a[0]) and got[0][1] is None and got[0][2] == EM.log_point(a[2])
    assert got[2][3] is None and int(oi[2].reshape(-1)[3]) == 1 and got[1][4] == EM.log_point(a[4])
    assert [int(v) for v in oi[0].reshape(-1)] == [0, 1, 0, 0, 0, 0]


def test_rejections(ctx):
    import vpin_amd
    from vpin_amd import capi

    def einval(fn, match):
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            fn()
        assert e.value.code == -1

    pts = LM.logs_to_points(logs(0x300, 8))
    x, y, inf = to_arrays(pts)
    ok = ctx.e2_plane_sums(x, y, inf, 2, 2, 2, [[1, 1]])
    assert points_of(*ok) == [GM.e2_add(pts[i], pts[4 + i]) for i in range(4)]
    einval(lambda: ctx.e2_plane_sums(x, y, inf, 2, 2, 2, [[1, 1], [0, 0]]), "selects no plane")
    bad = y.copy()
    bad[5, 0] ^= 1
    einval(lambda: ctx.e2_plane_sums(x, bad, inf, 2, 2, 2, [[1, 1]]), "not on the curve")
    big = x.copy()
    big[3] = np.frombuffer(GM.Q.to_bytes(32, "little"), np.uint8)
    einval(lambda: ctx.e2_plane_sums(big, y, inf, 2, 2, 2, [[1, 1]]), "below q")
    # a zero dimension and a null argument, through the C ABI itself
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    con = np.ones((1, 2), np.uint8)
    out = [np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)]
    for dims in ((0, 2, 2, 1), (2, 0, 2, 1), (2, 2, 0, 1), (2, 2, 2, 0)):
        rc = L.vpin_e2_plane_sums(ctx.h, p(x), p(y), p(inf), dims[0], dims[1], dims[2], p(con), dims[3], *[p(a) for a in out])
        assert rc == -1 and b"zero" in L.vpin_last_error()
    args = [ctx.h, p(x), p(y), p(inf), 2, 2, 2, p(con), 1] + [p(a) for a in out]
    for i in (0, 1, 2, 3, 7, 9, 10, 11):
        rc = L.vpin_e2_plane_sums(*[None if j == i else v for j, v in enumerate(args)])
        assert rc == -1 and b"null argument" in L.vpin_last_error()
