"""GPU parity of the encrypted fully connected layer (vpin_enc_fc) and of the encrypted average pooling (vpin_enc_avgpool2d) with
the Python model tests/enc_fc_model.py: output ciphertext, the operation lists and the left sides byte for byte; degenerate
points; the rejections; and each layer through to verified SNARKs.

As in test_gpu_enc_conv.py only the small cases use the literal model.  The others feed the GPU points k * G from
vpin_synthetic_points and the model the discrete logs k; an expected point is then one multiplication of G
(enc_fc_model.base_point, a fixed-base form of log_point: the larger lists hold about a thousand points)."""
import numpy as np
import pytest

import enc_fc_model as FM
import gadgets_model as GM
from test_gpu_enc_conv import KEYS, SEED_C, SEED_P, assert_lists, point_at, points_of, to_arrays

pytestmark = pytest.mark.gpu

Q = GM.Q


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def neg(p):
    return p[0], (Q - p[1]) % Q


def flat(rows):
    return [v for r in rows for v in r]


def fc_points(ctx, rows, K, W, N, biases, keys, prf_bytes):
    """the layer over literal points: rows and biases as the model takes them"""
    x, y, inf = to_arrays(flat(rows))
    bx, by, binf = to_arrays(flat(biases))
    return ctx.enc_fc(x, y, inf, len(rows), K, W, N, bx, by, binf, keys, prf_bytes)


def assert_output(tr, out, conv=lambda p: p):
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == [conv(v) for v in flat(out)], "outputs (an identity flagged and written as zeros)"


# ---- the fully connected layer --------------------------------------------------------------------------------------

def test_fc_literal_parity(ctx):
    """P = 2, K = 3, N = 2; a zero weight and a 17-bit one; non-identity biases; the 13-byte PRF; one key per row"""
    P, K, N = 2, 3, 2
    W = [[3, 0], [0x1ABCD, 7], [2, 5]]
    assert W[1][0].bit_length() == 17
    pts = [FM.log_point(k) for k in FM.synthetic_logs(0xFC01, P * (K + N))]
    rows = [pts[p * K:(p + 1) * K] for p in range(P)]
    biases = [pts[P * K + p * N:P * K + (p + 1) * N] for p in range(P)]
    assert KEYS[0] != KEYS[1]
    tr = fc_points(ctx, rows, K, W, N, biases, KEYS[:2], 13)
    exp = FM.fc(FM.POINTS, rows, K, W, N, biases, KEYS[:2], 13)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (2, 1, 2, 6, 8)
    assert_output(tr, exp["out"])
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"])
    assert not tr.adds()[4].any()
    tr.free()


def run_log_fc(ctx, seed, P, K, W, N, prf_bytes):
    from vpin_amd import gadgets as G
    n = P * (K + N)
    x, y = G.synthetic_points(seed, n)
    logs = FM.synthetic_logs(seed, n)
    tr = ctx.enc_fc(x[:P * K], y[:P * K], None, P, K, W, N, x[P * K:], y[P * K:], None, KEYS[:P], prf_bytes)
    exp = FM.fc(FM.LOGS, [logs[p * K:(p + 1) * K] for p in range(P)], K, W, N,
                [logs[P * K + p * N:P * K + (p + 1) * N] for p in range(P)], KEYS[:P], prf_bytes)
    return tr, exp


@pytest.mark.parametrize("P,K,N", [(2, 1, 1), (2, 65, 3), (1, 257, 2), (1, 5, 70)])
def test_fc_shapes(ctx, P, K, N):
    """no chain additions; one term past a wave; a second block of k (the reduce launch sees two partials); N past a wave for
    the left sum.  W is not square and its entries are distinct, so a k / j swap shows; they stay below 2^13, so with the
    13-byte PRF a folded weight stays below 2^(104 + 13 + 7)."""
    W = [[1 + 7 * (k * N + j) for j in range(N)] for k in range(K)]
    tr, exp = run_log_fc(ctx, 0xFC00 + K, P, K, W, N, 13)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (P, 1, N, P * K, P * (N + K - 1))
    assert_output(tr, exp["out"], FM.base_point)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], FM.base_point)
    tr.free()


def test_fc_degenerate_points(ctx):
    """X[0] == X[1] under equal weights (the tree and the chain meet P + P); X[2] = -X[3] under equal weights in column 0 only
    (a partial sum cancels, C[0] survives); a bias flagged as the identity (rz = 1); a bias equal to -C[1] (the output is the
    identity); a weight row of zeros (s_4 = 0, T_4 is the identity, rz = 1)"""
    K, N = 5, 2
    A, B, D = FM.log_point(5), FM.log_point(77), FM.log_point(123456789)
    X = [A, A, B, neg(B), D]
    W = [[3, 6], [3, 6], [4, 2], [4, 5], [0, 0]]
    C1 = FM.POINTS.add(FM.POINTS.mul(12, A), FM.POINTS.mul(3, neg(B)))
    bias = [None, neg(C1)]
    tr = fc_points(ctx, [X], K, W, N, [bias], KEYS[:1], 13)
    exp = FM.fc(FM.POINTS, [X], K, W, N, [bias], KEYS[:1], 13)
    assert exp["out"][0] == [FM.log_point(30), None]  # C[0] = 6 A
    assert exp["mults"][4][0] == 0 and exp["adds"][-1][1] is None
    assert_output(tr, exp["out"])
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"])
    assert [int(v) for v in tr.adds()[4]] == [1, 0, 0, 0, 0, 1]
    tr.free()


def test_fc_rejections(ctx):
    import vpin_amd
    P, K, N = 1, 3, 2
    pts = [FM.log_point(k) for k in FM.synthetic_logs(0xFC02, K + N)]
    X, bias, W = pts[:K], pts[K:], [[1, 2], [3, 4], [5, 6]]

    def rejected(X=X, bias=bias, W=W, N=N, prf_bytes=13):
        with pytest.raises(vpin_amd.VpinError) as ei:  # enc_fc itself asserts that no handle came back
            fc_points(ctx, [X], K, W, N, [bias], KEYS[:1], prf_bytes)
        return ei.value.code, str(ei.value)

    code, msg = rejected(X=[X[0], None, X[2]])
    assert code == -5 and "X[k] is the identity" in msg
    code, msg = rejected(W=[[1, 0], [3, 0], [5, 0]])
    assert code == -5 and "C[j] is the identity" in msg
    code, msg = rejected(W=[[0xFFFFFFFF] * 2] * 3, prf_bytes=16)
    assert code == -5 and "128 bits" in msg
    code, msg = rejected(bias=[bias[0], (bias[1][0], (bias[1][1] + 1) % Q)])
    assert code == -1 and "bias point is not on the curve" in msg
    code, msg = rejected(prf_bytes=0)
    assert code == -1 and "prf_bytes" in msg
    code, msg = rejected(bias=[], W=[[], [], []], N=0)
    assert code == -1
    # the same inputs unspoilt are accepted
    tr = fc_points(ctx, [X], K, W, N, [bias], KEYS[:1], 13)
    assert (tr.n_mult, tr.n_add) == (3, 4)
    tr.free()


def prove_and_compare(ctx, pairs):
    """pairs: (instance from the trace, instance from the gadget entry point called directly on the list)"""
    for g, d in pairs:
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        ref = d.snark_prove(SEED_C, SEED_P)
        assert got["proof"] == ref["proof"] and got["comm"] == ref["comm"]
        g.free()
        d.free()


def test_fc_through_to_two_proofs(ctx):
    P, K, N = 2, 4, 3
    W = [[1 + 7 * (k * N + j) for j in range(N)] for k in range(K)]
    tr, exp = run_log_fc(ctx, 0xFC03, P, K, W, N, 13)
    assert (tr.n_mult, tr.n_add) == (8, 12)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], FM.base_point)
    gm, ga = tr.instances()
    w, mx, my = tr.mults()
    prove_and_compare(ctx, [(gm, ctx.gadget_point_mult_dev(w, mx, my)), (ga, ctx.gadget_point_add_dev(*tr.adds()))])
    tr.free()


# ---- the average pooling --------------------------------------------------------------------------------------------

def test_pool_literal_parity(ctx):
    P, H, W = 2, 4, 6
    pts = [FM.log_point(k) for k in FM.synthetic_logs(0x9002, P * H * W)]
    planes = [pts[p * H * W:(p + 1) * H * W] for p in range(P)]
    tr = ctx.enc_avgpool2d(*to_arrays(pts), P, H, W, 2, 2, 256)
    exp = FM.avgpool(FM.POINTS, planes, H, W, 2, 2, 256)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (2, 2, 3, 0, 36)
    assert_output(tr, exp["out"])
    assert_lists(tr, [], exp["adds"], [])
    tr.free()


def run_log_pool(ctx, seed, P, H, W, k, stride, scale):
    from vpin_amd import gadgets as G
    n = P * H * W
    x, y = G.synthetic_points(seed, n)
    logs = FM.synthetic_logs(seed, n)
    tr = ctx.enc_avgpool2d(x, y, None, P, H, W, k, stride, scale)
    exp = FM.avgpool(FM.LOGS, [logs[p * H * W:(p + 1) * H * W] for p in range(P)], H, W, k, stride, scale)
    return tr, exp, (x, y)


@pytest.mark.parametrize("P,H,W,k,stride", [(2, 5, 5, 2, 2), (1, 5, 4, 3, 1)])
def test_pool_shapes(ctx, P, H, W, k, stride):
    """the last row and column are never read; overlapping windows"""
    tr, exp, _ = run_log_pool(ctx, 0x9000 + H * W, P, H, W, k, stride, 256)
    oh, ow = FM.pool_dims(H, W, k, stride)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (P, oh, ow, 0, P * oh * ow * (k * k - 1))
    assert_output(tr, exp["out"], FM.base_point)
    assert_lists(tr, [], exp["adds"], [], FM.base_point)
    tr.free()


def test_pool_past_one_workgroup(ctx):
    """one plane of 34 x 34: 289 outputs.  The corners and 40 sampled outputs with their three additions as points; the
    second operands of the WHOLE list are input points and are compared with the input bytes"""
    H = W = 34
    tr, exp, (x, y) = run_log_pool(ctx, 0x9003, 1, H, W, 2, 2, 256)
    assert (tr.oh, tr.ow, tr.n_add) == (17, 17, 867)
    ox, oy, oi = tr.output()
    px, py, rx, ry, rz = tr.adds()
    rng = np.random.default_rng(34)
    corners = [0, 16, 16 * 17, 288]
    rest = [int(v) for v in rng.choice(np.setdiff1d(np.arange(289), corners), 40, replace=False)]
    for t in corners + rest:
        assert point_at(ox, oy, oi, t) == FM.base_point(exp["out"][0][t]), f"output {t}"
        for m in range(3):
            acc, e = exp["adds"][3 * t + m]
            assert point_at(px, py, None, 3 * t + m) == FM.base_point(acc), f"accumulator {m} of output {t}"
            assert point_at(rx, ry, rz, 3 * t + m) == FM.base_point(e), f"operand {m} of output {t}"
    src = np.array([(2 * (t // 17) + m // 2) * W + 2 * (t % 17) + m % 2 for t in range(289) for m in (1, 2, 3)])
    assert np.array_equal(rx, x[src]) and np.array_equal(ry, y[src]) and not rz.any()
    tr.free()


def test_pool_outputs_equal_the_constant_filter_convolution(ctx):
    from vpin_amd import gadgets as G
    H, W, k, stride, scale = 7, 6, 3, 2, 341
    x, y = G.synthetic_points(0x9004, H * W)
    tr = ctx.enc_avgpool2d(x, y, None, 1, H, W, k, stride, scale)
    cx, cy, ci = ctx.e2_conv2d(x, y, None, H, W, [scale] * (k * k), k, k, 0, stride)
    ox, oy, oi = tr.output()
    assert cx.shape == (3, 2, 32) and np.array_equal(ox[0], cx) and np.array_equal(oy[0], cy) and np.array_equal(oi[0], ci)
    tr.free()


def test_pool_degenerate_points(ctx):
    """one plane of 2 x 8 under k = 2, stride 2: four windows e_0 e_1 / e_2 e_3.  Window 0: an identity at e_2 (rz = 1).
    Window 1: e_3 = -(e_0 + e_1 + e_2), the LAST sum cancels: the output is the identity.  Windows 2, 3: ordinary.
    A sum that cancels one step earlier (e_2 = -(e_0 + e_1), e_3 an identity) leaves an identity accumulator before e_3: by the
    layer's rule that is VPIN_ESHAPE like the other two rejected windows, not an identity output."""
    import vpin_amd
    A, B, D, E = (FM.log_point(k) for k in (5, 77, 123456789, 4242))
    add = FM.POINTS.add
    row0 = [A, B, A, B, D, E, E, A]
    row1 = [None, D, D, neg(add(add(A, B), D)), A, B, D, D]
    plane = row0 + row1
    tr = ctx.enc_avgpool2d(*to_arrays(plane), 1, 2, 8, 2, 2, 256)
    exp = FM.avgpool(FM.POINTS, [plane], 2, 8, 2, 2, 256)
    assert exp["out"][0][1] is None and exp["adds"][1][1] is None
    assert_output(tr, exp["out"])
    assert_lists(tr, [], exp["adds"], [])
    assert [int(v) for v in tr.adds()[4]] == [0, 1, 0] + [0] * 9
    tr.free()

    def rejected(window):
        with pytest.raises(vpin_amd.VpinError) as ei:
            ctx.enc_avgpool2d(*to_arrays(window), 1, 2, 2, 2, 2, 256)
        assert ei.value.code == -5 and "accumulator is the identity" in str(ei.value)

    rejected([None, A, B, D])                       # e_0 is the identity
    rejected([A, neg(A), B, D])                     # e_1 = -e_0: an identity accumulator before e_2
    rejected([A, B, neg(add(A, B)), None])          # e_2 = -(e_0 + e_1): an identity accumulator before e_3, whatever e_3 is
    tr = ctx.enc_avgpool2d(*to_arrays([A, B, D, E]), 1, 2, 2, 2, 2, 256)  # the same call unspoilt
    assert tr.n_add == 3
    tr.free()


def test_pool_trace_shape(ctx):
    """k = 1 has nothing to add; no pooling trace has multiplications or a left side"""
    tr, exp, _ = run_log_pool(ctx, 0x9005, 1, 3, 2, 1, 1, 256)
    assert (tr.oh, tr.ow, tr.n_mult, tr.n_add) == (3, 2, 0, 0)
    assert tr.instances() == (None, None)
    w, mx, my = tr.mults()
    assert w == [] and mx.shape == (0, 32) and my.shape == (0, 32)
    assert [a.shape for a in tr.left()] == [(0, 32), (0, 32), (0,)]
    assert [a.shape[0] for a in tr.adds()] == [0] * 5
    assert_output(tr, exp["out"], FM.base_point)
    tr.free()


def test_pool_through_to_a_proof(ctx):
    tr, exp, _ = run_log_pool(ctx, 0x9006, 1, 4, 4, 2, 2, 256)
    assert (tr.n_mult, tr.n_add) == (0, 12)
    assert_lists(tr, [], exp["adds"], [], FM.base_point)
    gm, ga = tr.instances()
    assert gm is None
    prove_and_compare(ctx, [(ga, ctx.gadget_point_add_dev(*tr.adds()))])
    tr.free()
