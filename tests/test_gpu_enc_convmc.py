"""GPU parity of the trained convolution layer (vpin_enc_conv2d_mc, vpin_e2_conv2d_mc) with the Python model
tests/convmc_model.py: output ciphertext, the two operation lists of the check and its left sides, byte for byte; the cases of
the complete addition across channels; the existing one-filter layer and the plane sums as special cases; the rejections; and one
layer through to two verified SNARKs.

Only the first test uses the literal model.  The others feed the GPU pixels k_p * G from vpin_synthetic_points (negated or flagged
where a case needs it) and the model the discrete logs; expected points come from one batched conversion (lenet_model.logs_to_points)."""
import numpy as np
import pytest

import convmc_model as CM
import enc_conv_model as EM
import gadgets_model as GM
import lenet_model as LM
from test_gpu_enc_conv import assert_lists, points_of, to_arrays

pytestmark = pytest.mark.gpu

Q = GM.Q
KEYS = [bytes((37 * p + 11 * i + 5) % 256 for i in range(32)) for p in range(8)]
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))
# a negative weight, a zero that is not the first term of a chain, a value >= 2^16
W_2x2x2 = [[[3, -5, 0, 70001], [-2, 1, 65536, -7]], [[-1, 0, 4, 9], [6, -66000, 0, 2]]]


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def test_literal_parity(ctx):
    """groups 2, C 2, n_out 2, 4 x 4, f 2, pad 0, stride 1, prf_bytes 16, against the model on affine points"""
    G_, C, n_out, H, W = 2, 2, 2, 4, 4
    logs = EM.synthetic_logs(0x4D43, G_ * C * H * W)
    planes = [[EM.log_point(k) for k in logs[p * H * W:(p + 1) * H * W]] for p in range(G_ * C)]
    x, y, inf = to_arrays([p for plane in planes for p in plane])
    tr = ctx.enc_conv2d_mc(x, y, inf, G_, C, n_out, H, W, W_2x2x2, None, 2, 2, 0, 1, KEYS[:4], 16)
    exp = CM.layer(CM.POINTS, planes, C, n_out, H, W, W_2x2x2, None, 2, 2, 0, 1, KEYS[:4], 16)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (4, 3, 3, 32, 28)
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == [p for plane in exp["out"] for p in plane]
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"])
    assert tr.mults()[0][:8] == [3, 5, 0, 70001, 2, 1, 65536, 7] and sum(int(v) for v in tr.adds()[4]) == 2 * 3  # the zero weights
    bx, by, bi = ctx.e2_conv2d_mc(x, y, inf, G_, C, n_out, H, W, W_2x2x2, None, 2, 2, 0, 1)
    assert np.array_equal(bx.reshape(ox.shape), ox) and np.array_equal(by.reshape(oy.shape), oy) and np.array_equal(bi.reshape(oi.shape), oi)
    tr.free()


def pixels(seed, n_planes, H, W):
    """n_planes planes of synthetic points with their discrete logs"""
    from vpin_amd import gadgets as G
    n = n_planes * H * W
    x, y = G.synthetic_points(seed, n)
    logs = EM.synthetic_logs(seed, n)
    return x.reshape(n_planes, H * W, 32).copy(), y.reshape(n_planes, H * W, 32).copy(), np.zeros((n_planes, H * W), np.uint8), \
        [logs[p * H * W:(p + 1) * H * W] for p in range(n_planes)]


def negated(y):
    """q - y on canonical little-endian bytes"""
    out = np.zeros_like(y)
    for i, row in enumerate(y.reshape(-1, 32)):
        out.reshape(-1, 32)[i] = np.frombuffer((Q - int.from_bytes(bytes(row), "little")).to_bytes(32, "little"), np.uint8)
    return out


def check_log_layer(ctx, x, y, inf, logs, G_, C, n_out, H, W, weights, connect, f, pad, stride, prf_bytes=16):
    """the layer on the GPU against the model on logarithms: output, lists, left sides.  Returns (trace, model result)"""
    keys = KEYS[:G_ * n_out]
    tr = ctx.enc_conv2d_mc(x, y, inf, G_, C, n_out, H, W, weights, connect, f, f, pad, stride, keys, prf_bytes)
    exp = CM.layer(CM.LOGS, logs, C, n_out, H, W, weights, connect, f, f, pad, stride, keys, prf_bytes)
    oh, ow = EM.out_dims(H, W, f, f, pad, stride)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (G_ * n_out, oh, ow) + CM.trace_counts(G_, C, n_out, connect, f, f)
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == LM.logs_to_points([v for plane in exp["out"] for v in plane]), "output ciphertext"
    flat = [m[1] for m in exp["mults"]] + [a[0] for a in exp["adds"]] + [a[1] for a in exp["adds"]] + exp["left"]
    table = dict(zip(flat, LM.logs_to_points(flat)))
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], table.__getitem__)
    return tr, exp


def test_pad_stride_and_a_rectangular_plane(ctx):
    """pad 1, stride 2, 5 x 4, f 3: a row / column swap shows; the padding is the identity inside the windows"""
    x, y, inf, logs = pixels(0xA1, 4, 5, 4)
    weights = [[CM._signed(0x10 + 2 * o + c, 9, 1 << 17) for c in range(2)] for o in range(2)]
    weights[1][0][4] = 0
    tr, _ = check_log_layer(ctx, x, y, inf, logs, 2, 2, 2, 5, 4, weights, None, 3, 1, 2)
    assert (tr.oh, tr.ow) == (3, 2)
    tr.free()


TABLE = [[1, 1, 0], [0, 1, 1], [1, 1, 1]]
FILT = [2, 0, 1, 3]


def test_connection_table_and_the_plane_sum_route(ctx):
    """an unconnected pair shrinks the trace; garbage in its weights changes nothing; and with W[o][c] = filter where connected the
    output is vpin_e2_plane_sums followed by vpin_e2_conv2d"""
    G_, C, H, W = 2, 3, 4, 5
    x, y, inf, logs = pixels(0xA2, G_ * C, H, W)
    w_a = [[[w if on else 977 for w in FILT] for on in row] for row in TABLE]
    w_b = [[[w if on else -(1 << 30) for w in FILT] for on in row] for row in TABLE]
    tr, _ = check_log_layer(ctx, x, y, inf, logs, G_, C, 3, H, W, w_a, TABLE, 2, 0, 1)
    assert (tr.n_mult, tr.n_add) == (2 * 4 * 7, 2 * 4 * 7 - 6) and tr.n_mult < 2 * 4 * 9
    other = ctx.enc_conv2d_mc(x, y, inf, G_, C, 3, H, W, w_b, TABLE, 2, 2, 0, 1, KEYS[:6], 16)
    for u, v in zip(list(tr.output()) + list(tr.adds()) + list(tr.mults()[1:]) + list(tr.left()),
                    list(other.output()) + list(other.adds()) + list(other.mults()[1:]) + list(other.left())):
        assert np.array_equal(u, v)
    assert tr.mults()[0] == other.mults()[0]
    ox, oy, oi = tr.output()
    for g in range(G_):
        sx, sy, si = ctx.e2_plane_sums(x[g * C:(g + 1) * C], y[g * C:(g + 1) * C], inf[g * C:(g + 1) * C], C, H, W, TABLE)
        for o in range(3):
            cx, cy, ci = ctx.e2_conv2d(sx[o], sy[o], si[o], H, W, FILT, 2, 2, 0, 1)
            assert np.array_equal(cx, ox[g * 3 + o]) and np.array_equal(cy, oy[g * 3 + o]) and np.array_equal(ci, oi[g * 3 + o])
    other.free()
    tr.free()


def test_equal_channels_double_in_the_tree(ctx):
    """C 3 with channel 1 = channel 0 under equal weights: the slots' partial sums are the same point"""
    x, y, inf, logs = pixels(0xA3, 3, 4, 4)
    x[1], y[1], logs[1] = x[0], y[0], list(logs[0])
    f0 = [5, -3, 2, 1]
    tr, exp = check_log_layer(ctx, x, y, inf, logs, 1, 3, 1, 4, 4, [[f0, f0, [1, 0, -2, 4]]], None, 2, 0, 1)
    tr.free()


def test_opposite_channels_cancel_to_the_flagged_identity(ctx):
    """C 2 with channel 1 = -channel 0 under equal weights: every output is the flagged identity (the bare stage returns the
    flags) and so is the left side.  The chain T(0,0) .. T(0,3), -T(0,0) .. cancels term by term; the filter's last weight is 0,
    so the accumulator is the identity BEFORE the last step and the layer ends in VPIN_ESHAPE under the accumulator rule.  (With a
    non-zero last weight the identity appears only after the last step, where it is compared, not judged.)"""
    import vpin_amd
    x, y, inf, logs = pixels(0xA4, 2, 4, 4)
    x[1], y[1], logs[1] = x[0], negated(y[0]).reshape(y[0].shape), [(-k) % EM.ORDER for k in logs[0]]
    f0 = [4, -9, 6, 0]
    ox, oy, oi = ctx.e2_conv2d_mc(x, y, inf, 1, 2, 1, 4, 4, [[f0, f0]], None, 2, 2, 0, 1)
    assert oi.all() and not ox.any() and not oy.any()
    with pytest.raises(CM.ShapeError, match="accumulator"):
        CM.layer(CM.LOGS, logs, 2, 1, 4, 4, [[f0, f0]], None, 2, 2, 0, 1, KEYS[:1], 16)
    with pytest.raises(vpin_amd.VpinError, match="accumulator is the identity") as e:
        ctx.enc_conv2d_mc(x, y, inf, 1, 2, 1, 4, 4, [[f0, f0]], None, 2, 2, 0, 1, KEYS[:1], 16)
    assert e.value.code == -5
    # the non-zero last weight: both sides are the identity, the check holds, the left side is flagged
    f1 = [4, -9, 6, 2]
    tr, exp = check_log_layer(ctx, x, y, inf, logs, 1, 2, 1, 4, 4, [[f1, f1]], None, 2, 0, 1)
    assert exp["left"] == [0] and tr.left()[2].all() and tr.output()[2].all()
    tr.free()


def test_identity_pixels_and_padding_inside_a_window(ctx):
    x, y, inf, logs = pixels(0xA5, 4, 4, 3)
    for p, i in ((0, 0), (0, 5), (1, 4), (3, 11), (3, 10)):
        inf[p, i], logs[p][i] = 1, 0
    weights = [[CM._signed(0x20 + 2 * o + c, 4) for c in range(2)] for o in range(2)]
    tr, exp = check_log_layer(ctx, x, y, inf, logs, 2, 2, 2, 4, 3, weights, None, 2, 1, 1, prf_bytes=13)
    tr.free()


@pytest.mark.parametrize("C,n_out,H,f,outputs", [(2, 1, 10, 2, 81), (5, 2, 6, 2, 25), (2, 1, 18, 2, 289), (3, 2, 2, 2, 1), (17, 1, 3, 2, 4)])
def test_pixel_block_edge_and_uneven_channel_split(ctx, C, n_out, H, f, outputs):
    """10 x 10, f 2, C 2: 81 outputs, the edge of a 64-pixel block falls inside the plane.  C 5: five slots of 51 pixels, 255
    lanes, the split does not divide the workgroup.  289 outputs: a sum of the check takes two workgroups and the second launch
    adds them; 1 output: 256 sums share a workgroup.  C 17: slot 0 walks two channels"""
    x, y, inf, logs = pixels(0xA6 + C, C, H, H)
    weights = [[CM._signed(0x30 + C * o + c, f * f) for c in range(C)] for o in range(n_out)]
    tr, _ = check_log_layer(ctx, x, y, inf, logs, 1, C, n_out, H, H, weights, None, f, 0, 1)
    assert tr.oh * tr.ow == outputs
    tr.free()


def test_degenerate_case_is_the_existing_layer(ctx):
    """groups = P, C = 1, n_out = 1 against vpin_enc_conv2d on the same planes and keys: the trace byte for byte"""
    P, H, W = 3, 6, 5
    x, y, inf, _ = pixels(0xA7, P, H, W)
    filt = [1, 0, 1, 2, 0, 2, 1, 0, 65537]
    old = ctx.enc_conv2d(x, y, inf, P, H, W, filt, 3, 3, 1, 1, KEYS[:P], 14)
    new = ctx.enc_conv2d_mc(x, y, inf, P, 1, 1, H, W, [[filt]], None, 3, 3, 1, 1, KEYS[:P], 14)
    assert (old.P, old.oh, old.ow, old.n_mult, old.n_add) == (new.P, new.oh, new.ow, new.n_mult, new.n_add) == (3, 6, 5, 27, 24)
    assert old.mults()[0] == new.mults()[0]
    for u, v in zip(list(old.output()) + list(old.adds()) + list(old.mults()[1:]) + list(old.left()),
                    list(new.output()) + list(new.adds()) + list(new.mults()[1:]) + list(new.left())):
        assert np.array_equal(u, v)
    old.free()
    new.free()


def test_rejections(ctx):
    import ctypes

    import vpin_amd
    from vpin_amd import capi
    H = W = 3
    x, y, inf, logs = pixels(0xA8, 2, H, W)
    good = [[[1, 2, 3, 4], [5, -6, 7, 8]]]

    def rejected(x=x, y=y, inf=inf, G_=1, C=2, n_out=1, weights=good, connect=None, f=2, prf_bytes=16, keys=KEYS[:1]):
        with pytest.raises(vpin_amd.VpinError) as ei:  # enc_conv2d_mc itself asserts that no handle came back
            ctx.enc_conv2d_mc(x, y, inf, G_, C, n_out, H, W, weights, connect, f, f, 0, 1, keys, prf_bytes)
        return ei.value.code, str(ei.value)

    off = y.copy()
    off[0, 4, 0] ^= 1
    code, msg = rejected(y=off)
    assert code == -1 and "not on the curve" in msg
    big = x.copy()
    big[1, 7] = np.frombuffer(Q.to_bytes(32, "little"), np.uint8)
    code, msg = rejected(x=big)
    assert code == -1 and "not below q" in msg
    code, msg = rejected(prf_bytes=0)
    assert code == -1 and "prf_bytes" in msg
    code, msg = rejected(f=4, weights=[[[1] * 16, [1] * 16]])
    assert code == -1 and "does not fit" in msg
    code, msg = rejected(connect=[[0, 0]])
    assert code == -1 and "selects no channel" in msg
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    w32, k = np.array(good, dtype=np.int32), np.frombuffer(KEYS[0], np.uint8).copy()
    h = ctypes.c_void_p()
    xs, ys, fs = ctx._points(x, y, inf)
    for G_, C, n_out in ((0, 2, 1), (1, 0, 1), (1, 2, 0)):  # the binding's own shape assertions stand in the way: the C ABI itself
        rc = capi.lib().vpin_enc_conv2d_mc(ctx.h, p(xs), p(ys), p(fs), G_, C, n_out, H, W, p(w32), None, 2, 2, 0, 1, p(k), 16, ctypes.byref(h))
        assert rc == -1 and not h.value and b"zero" in capi.lib().vpin_last_error()
    for Hh, f, stride in ((0, 2, 1), (3, 0, 1), (3, 2, 0)):  # a zero dimension, as vpin_enc_conv2d answers it
        rc = capi.lib().vpin_enc_conv2d_mc(ctx.h, p(xs), p(ys), p(fs), 1, 2, 1, Hh, W, p(w32), None, f, f, 0, stride, p(k), 16, ctypes.byref(h))
        assert rc == -1 and not h.value and b"a dimension is zero" in capi.lib().vpin_last_error()
    rc = capi.lib().vpin_enc_conv2d_mc(ctx.h, p(xs), p(ys), p(fs), 1, 2, 1, H, W, None, None, 2, 2, 0, 1, p(k), 16, ctypes.byref(h))
    assert rc == -1 and not h.value and b"null argument" in capi.lib().vpin_last_error()
    ob = np.zeros(4 * 32, np.uint8)
    rc = capi.lib().vpin_e2_conv2d_mc(ctx.h, p(xs), p(ys), p(fs), 1, 2, 0, H, W, p(w32), None, 2, 2, 0, 1, p(ob), p(ob), p(ob))
    assert rc == -1 and b"zero" in capi.lib().vpin_last_error()
    code, msg = rejected(weights=[[[0, 2, 3, 4], [5, -6, 7, 8]]])
    assert code == -5 and "accumulator is the identity" in msg
    none = inf.copy()
    none[1, :] = 1
    code, msg = rejected(inf=none)
    assert code == -5 and "B'[c][k] is the identity" in msg
    tr = ctx.enc_conv2d_mc(x, y, inf, 1, 2, 1, H, W, good, None, 2, 2, 0, 1, KEYS[:1], 16)  # the same inputs unspoilt are accepted
    assert (tr.n_mult, tr.n_add) == (8, 7)
    tr.free()


def test_layer_through_to_two_proofs(ctx):
    """groups 2, C 2, n_out 2, 4 x 4, f 2: the 32 + 28 operations through the unchanged prover and verifier"""
    x, y, inf, logs = pixels(0xA9, 4, 4, 4)
    tr, _ = check_log_layer(ctx, x, y, inf, logs, 2, 2, 2, 4, 4, W_2x2x2, None, 2, 0, 1)
    gm, ga = tr.instances()
    for g in (gm, ga):
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        g.free()
    tr.free()
