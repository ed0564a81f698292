"""GPU parity of the encrypted convolution layer (vpin_e2_msm, vpin_e2_conv2d, vpin_enc_conv2d) with the Python model
tests/enc_conv_model.py: output ciphertext, the two operation lists of the random-linear-combination check and its left side,
byte for byte; the rejections; and one layer through to two verified SNARKs.

Only the first test uses the literal model (a scalar multiplication of the model costs 10-17 ms).  The others feed the GPU
pixels k_p * G from vpin_synthetic_points and the model the discrete logs k_p: every expected point is then one multiplication
of G (enc_conv_model.log_point)."""
import numpy as np
import pytest

import enc_conv_model as EM
import gadgets_model as GM

pytestmark = pytest.mark.gpu

Q = GM.Q
CONV3 = [1, 0, 1, 2, 0, 2, 1, 0, 1]
KEYS = [bytes((31 * p + 7 * i + 3) % 256 for i in range(32)) for p in range(4)]
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def to_arrays(points):
    """list of (x, y) / None -> x (n, 32), y (n, 32), inf (n) uint8"""
    x = b"".join((0 if p is None else p[0]).to_bytes(32, "little") for p in points)
    y = b"".join((0 if p is None else p[1]).to_bytes(32, "little") for p in points)
    inf = np.array([p is None for p in points], dtype=np.uint8)
    return (np.frombuffer(x, np.uint8).reshape(-1, 32).copy(), np.frombuffer(y, np.uint8).reshape(-1, 32).copy(), inf)


def point_at(x, y, inf=None, i=0):
    """entry i of flat point arrays as the model's (x, y) / None"""
    x, y = x.reshape(-1, 32), y.reshape(-1, 32)
    if inf is not None and inf.reshape(-1)[i]:
        assert not x[i].any() and not y[i].any(), "an identity is written as zeros"
        return None
    return int.from_bytes(bytes(x[i]), "little"), int.from_bytes(bytes(y[i]), "little")


def points_of(x, y, inf=None):
    return [point_at(x, y, inf, i) for i in range(x.reshape(-1, 32).shape[0])]


def assert_lists(tr, mults, adds, left, conv=lambda p: p):
    """the trace's two operation lists and left sides against the model's (conv maps a model element to a point)"""
    w, mx, my = tr.mults()
    assert tr.n_mult == len(mults) and tr.n_add == len(adds)
    assert w == [m[0] for m in mults]
    assert points_of(mx, my) == [conv(m[1]) for m in mults], "multiplication operands B'[k]"
    px, py, rx, ry, rz = tr.adds()
    assert points_of(px, py) == [conv(a[0]) for a in adds], "addition accumulators"
    assert points_of(rx, ry, rz) == [conv(a[1]) for a in adds], "addition operands T_k (rz = 1 and zeros for the identity)"
    lx, ly, li = tr.left()
    assert points_of(lx, ly, li) == [conv(v) for v in left], "left sides"


def test_literal_parity_two_planes(ctx):
    """5 x 4 (a row / column swap shows), zero taps (identity terms), pad 1, two planes with their own keys, prf_bytes 16"""
    P, H, W = 2, 5, 4
    logs = EM.synthetic_logs(0x5650494E, P * H * W)
    planes = [[EM.log_point(k) for k in logs[p * H * W:(p + 1) * H * W]] for p in range(P)]
    x, y, inf = to_arrays(planes[0] + planes[1])
    tr = ctx.enc_conv2d(x, y, inf, P, H, W, CONV3, 3, 3, 1, 1, KEYS[:2], 16)
    exp = EM.layer(EM.POINTS, planes, H, W, CONV3, 3, 3, 1, 1, KEYS[:2], 16)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (2, 5, 4, 18, 16)
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == exp["out"][0] + exp["out"][1]
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"])
    assert sum(int(v) for v in tr.adds()[4]) == 6  # three zero taps per plane
    # the plane entry point computes the same outputs
    cx, cy, ci = ctx.e2_conv2d(x[:H * W], y[:H * W], inf[:H * W], H, W, CONV3, 3, 3, 1, 1)
    assert np.array_equal(cx, ox[0]) and np.array_equal(cy, oy[0]) and np.array_equal(ci, oi[0])
    tr.free()


def run_log_layer(ctx, seed, P, H, W, filt, fh, fw, pad, stride, prf_bytes):
    from vpin_amd import gadgets as G
    n = P * H * W
    x, y = G.synthetic_points(seed, n)
    logs = EM.synthetic_logs(seed, n)
    tr = ctx.enc_conv2d(x, y, None, P, H, W, filt, fh, fw, pad, stride, KEYS[:P], prf_bytes)
    exp = EM.layer(EM.LOGS, [logs[p * H * W:(p + 1) * H * W] for p in range(P)], H, W, filt, fh, fw, pad, stride, KEYS[:P], prf_bytes)
    return tr, exp


def test_geometry_and_wide_weights(ctx):
    """6 x 5, 2 x 2 filter, pad 0, stride 2 (the last column is never read); weights 2^16 - 1 and a 100-bit value; prf_bytes 13"""
    filt = [1, 2**16 - 1, (1 << 99) | 0x1E3779B97F4A7C15F39CC0605, 3]
    assert filt[2].bit_length() == 100
    tr, exp = run_log_layer(ctx, 0xC0FFEE, 1, 6, 5, filt, 2, 2, 0, 2, 13)
    assert (tr.oh, tr.ow, tr.n_mult, tr.n_add) == (3, 2, 4, 3)
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == [EM.log_point(k) for k in exp["out"][0]]
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], EM.log_point)
    tr.free()


def test_degenerate_points(ctx):
    """(a) every pixel the same point: 1*P + 1*P takes the doubling branch; (b) P, -P and flagged identities: some outputs are
    the identity.  Outputs and left sides of both planes against the literal model."""
    H = W = 3
    Pt, Rt, St = EM.log_point(5), EM.log_point(77), EM.log_point(123456789)
    neg = lambda p: (p[0], (Q - p[1]) % Q)
    plane_a = [Pt] * 9
    plane_b = [Pt, neg(Pt), Rt,
               None, None, St,
               Rt, neg(Rt), Pt]
    x, y, inf = to_arrays(plane_a + plane_b)
    filt = [1, 1, 1, 1]
    tr = ctx.enc_conv2d(x, y, inf, 2, H, W, filt, 2, 2, 0, 1, KEYS[:2], 16)
    exp = EM.layer(EM.POINTS, [plane_a, plane_b], H, W, filt, 2, 2, 0, 1, KEYS[:2], 16)
    assert exp["out"][0] == [EM.log_point(20)] * 4 and exp["out"][1][0] is None  # P - P + 0 + 0
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == exp["out"][0] + exp["out"][1]
    lx, ly, li = tr.left()
    assert points_of(lx, ly, li) == exp["left"]
    tr.free()


@pytest.mark.parametrize("P,H,W,f", [(2, 9, 8, 3), (1, 67, 61, 5)])
def test_across_waves_and_workgroups(ctx, P, H, W, f):
    """72 outputs per plane (one more than a wave) and 3835 (fifteen workgroups of the RLC, a second-launch reduction)"""
    filt = [(5 * k + 1) % 7 for k in range(f * f)]
    assert filt[0] != 0 and 0 in filt
    tr, exp = run_log_layer(ctx, 0xABCD + H, P, H, W, filt, f, f, 1, 1, 16)
    oh, ow = EM.out_dims(H, W, f, f, 1, 1)
    assert (tr.oh, tr.ow) == (oh, ow) and oh * ow in (72, 3835)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], EM.log_point)  # every B'[k] is a multiplication operand
    ox, oy, oi = tr.output()
    rng = np.random.default_rng(H)
    corners = [0, ow - 1, (oh - 1) * ow, oh * ow - 1]
    rest = [int(v) for v in rng.choice(np.setdiff1d(np.arange(oh * ow), corners), 60, replace=False)]
    for p in range(P):
        for t in (corners + rest if p == P - 1 else corners):
            assert point_at(ox[p], oy[p], oi[p], t) == EM.log_point(exp["out"][p][t]), f"output {t} of plane {p}"
    tr.free()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4099])
def test_e2_msm(ctx, n):
    from vpin_amd import gadgets as G
    x, y = G.synthetic_points(0xE2 + n, n)
    logs = EM.synthetic_logs(0xE2 + n, n)
    inf = np.zeros(n, dtype=np.uint8)
    st, scalars = n, []
    for _ in range(n):
        st, a = GM.splitmix64(st)
        st, b = GM.splitmix64(st)
        scalars.append((a << 64) | b)
    if n >= 2:  # a repeated point (equal scalars too: the tree meets P + P), and with three or more terms an identity
        x[1], y[1], logs[1], scalars[1] = x[0], y[0], logs[0], scalars[0]
    if n >= 3:
        inf[2], logs[2] = 1, 0
    exp = sum(s * k for s, k in zip(scalars, logs)) % EM.ORDER
    assert ctx.e2_msm(scalars, x, y, inf) == EM.log_point(exp)


def test_e2_msm_cancels_to_the_identity(ctx):
    Pt = EM.log_point(9)
    x, y, inf = to_arrays([Pt, (Pt[0], Q - Pt[1])])
    assert ctx.e2_msm([12345, 12345], x, y, inf) is None


def test_rejections(ctx):
    import vpin_amd
    H = W = 3
    logs = EM.synthetic_logs(99, H * W)
    pts = [EM.log_point(k) for k in logs]
    keys, filt = KEYS[:1], [1, 2, 3, 4]

    def rejected(points, filt=filt, prf_bytes=16, raw=None):
        x, y, inf = raw if raw is not None else to_arrays(points)
        with pytest.raises(vpin_amd.VpinError) as ei:  # enc_conv2d itself asserts that no handle came back
            ctx.enc_conv2d(x, y, inf, 1, H, W, filt, 2, 2, 0, 1, keys, prf_bytes)
        return ei.value.code, str(ei.value)

    off = list(pts)
    off[4] = (pts[4][0], (pts[4][1] + 1) % Q)
    code, msg = rejected(off)
    assert code == -1 and "not on the curve" in msg
    x, y, inf = to_arrays(pts)
    x[7] = np.frombuffer(Q.to_bytes(32, "little"), np.uint8)
    code, msg = rejected(None, raw=(x, y, inf))
    assert code == -1 and "not below q" in msg
    code, msg = rejected(pts, prf_bytes=17)
    assert code == -1 and "prf_bytes" in msg
    code, msg = rejected(pts, filt=[0, 2, 3, 4])
    assert code == -5 and "accumulator is the identity" in msg
    code, msg = rejected([None] * 9)
    assert code == -5 and "B'[k] is the identity" in msg
    # the same inputs unspoilt are accepted
    tr = ctx.enc_conv2d(*to_arrays(pts), 1, H, W, filt, 2, 2, 0, 1, keys, 16)
    assert (tr.n_mult, tr.n_add) == (4, 3)
    tr.free()


def test_layer_through_to_two_proofs(ctx):
    """one c1 and one c2 plane of 32 x 32 under the 3 x 3 filter: the 3_32 configuration's 18 + 16 operations, proven"""
    import vpin_amd
    tr, exp = run_log_layer(ctx, 0x5650494E + 1, 2, 32, 32, CONV3, 3, 3, 1, 1, 16)
    assert (tr.oh, tr.ow, tr.n_mult, tr.n_add) == (32, 32, 18, 16)
    assert vpin_amd.gadget_shape("mult", tr.n_mult)[:2] == (2**16, 2**16)
    assert vpin_amd.gadget_shape("add", tr.n_add)[0] == 2**8
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], EM.log_point)
    gm, ga = tr.instances()
    w, mx, my = tr.mults()
    direct = [ctx.gadget_point_mult_dev(w, mx, my), ctx.gadget_point_add_dev(*tr.adds())]
    for g, d, nc_unpadded in ((gm, direct[0], 62352), (ga, direct[1], 160)):
        assert g.num_cons_unpadded == nc_unpadded and g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        ref = d.snark_prove(SEED_C, SEED_P)
        assert got["proof"] == ref["proof"] and got["comm"] == ref["comm"]
        g.free()
        d.free()
    tr.free()
