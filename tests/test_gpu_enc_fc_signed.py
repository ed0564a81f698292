"""GPU parity of the fully connected layer over signed weights (vpin_enc_fc_signed) with the Python model tests/fcs_model.py:
output ciphertext, the operation lists and the left sides byte for byte; byte equality with vpin_enc_fc on non-negative weights;
the degenerate points the signs make reachable; the rejections; and the layer through to two verified SNARKs.

As in test_gpu_enc_fc.py only the small cases use the literal model; the shapes feed the GPU points k * G from
vpin_synthetic_points and the model the discrete logs k (enc_fc_model.base_point turns an expected logarithm into a point)."""
import numpy as np
import pytest

import enc_fc_model as FM
import fcs_model as TM
import gadgets_model as GM
from test_gpu_enc_conv import KEYS, assert_lists, to_arrays
from test_gpu_enc_fc import assert_output, flat, neg, prove_and_compare

pytestmark = pytest.mark.gpu

Q = GM.Q


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def fcs_points(ctx, rows, K, W, N, biases, keys, prf_bytes):
    """the layer over literal points: rows and biases as the model takes them"""
    x, y, inf = to_arrays(flat(rows))
    bx, by, binf = to_arrays(flat(biases))
    return ctx.enc_fc_signed(x, y, inf, len(rows), K, W, N, bx, by, binf, keys, prf_bytes)


@pytest.mark.parametrize("W,prf_bytes", [([[3, 0], [-0x1ABCD, 7], [-2, -5]], 13), ([[3, 0], [-(1 << 31), 7], [-2, -5]], 8)])
def test_fcs_literal_parity(ctx, W, prf_bytes):
    """P = 2, K = 3, N = 2: s_0 = 3 r_0 > 0, s_1 < 0 (r_0 has prf_bytes bytes and a weight of 17 or 32 bits against 7 r_1), s_2 < 0;
    the second case holds INT32_MIN, whose magnitude 2^31 exists only unsigned, with an 8-byte PRF so that the fold fits"""
    P, K, N = 2, 3, 2
    pts = [FM.log_point(k) for k in FM.synthetic_logs(0xF501, P * (K + N))]
    rows = [pts[p * K:(p + 1) * K] for p in range(P)]
    biases = [pts[P * K + p * N:P * K + (p + 1) * N] for p in range(P)]
    tr = fcs_points(ctx, rows, K, W, N, biases, KEYS[:2], prf_bytes)
    exp = TM.fc_signed(TM.POINTS, rows, K, W, N, biases, KEYS[:2], prf_bytes)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (2, 1, 2, 6, 8)
    assert_output(tr, exp["out"])
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"])
    assert [m[1] for m in exp["mults"][:3]] == [rows[0][0], neg(rows[0][1]), neg(rows[0][2])], "the sign goes into the point"
    tr.free()


def signed_matrix(K, N):
    """distinct entries of alternating sign, the first one negative; below 2^13 in magnitude for the shapes used here"""
    return [[(1 + 7 * (k * N + j)) * (1 if (k * N + j) % 2 else -1) for j in range(N)] for k in range(K)]


def run_log_fcs(ctx, seed, P, K, W, N, prf_bytes):
    from vpin_amd import gadgets as G
    n = P * (K + N)
    x, y = G.synthetic_points(seed, n)
    logs = FM.synthetic_logs(seed, n)
    tr = ctx.enc_fc_signed(x[:P * K], y[:P * K], None, P, K, W, N, x[P * K:], y[P * K:], None, KEYS[:P], prf_bytes)
    exp = TM.fc_signed(TM.LOGS, [logs[p * K:(p + 1) * K] for p in range(P)], K, W, N,
                       [logs[P * K + p * N:P * K + (p + 1) * N] for p in range(P)], KEYS[:P], prf_bytes)
    return tr, exp


@pytest.mark.parametrize("P,K,N", [(2, 1, 1), (2, 65, 3), (1, 257, 2), (1, 5, 70)])
def test_fcs_shapes(ctx, P, K, N):
    """test_gpu_enc_fc.py's shapes: no chain additions (and the one weight negative); one term past a wave; a second block of k;
    N past a wave for the left sum"""
    tr, exp = run_log_fcs(ctx, 0xF500 + K, P, K, signed_matrix(K, N), N, 13)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (P, 1, N, P * K, P * (N + K - 1))
    assert_output(tr, exp["out"], FM.base_point)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], FM.base_point)
    tr.free()


def test_fcs_on_non_negative_weights_is_vpin_enc_fc_byte_for_byte(ctx):
    from vpin_amd import gadgets as G
    P, K, N = 2, 65, 3
    W = [[1 + 7 * (k * N + j) for j in range(N)] for k in range(K)]
    x, y = G.synthetic_points(0xF541, P * (K + N))
    args = (x[:P * K], y[:P * K], None, P, K, W, N, x[P * K:], y[P * K:], None, KEYS[:P], 13)
    old, new = ctx.enc_fc(*args), ctx.enc_fc_signed(*args)
    assert (old.P, old.oh, old.ow, old.n_mult, old.n_add) == (new.P, new.oh, new.ow, new.n_mult, new.n_add)
    assert old.mults()[0] == new.mults()[0]
    for u, v in zip(list(old.output()) + list(old.adds()) + list(old.mults()[1:]) + list(old.left()),
                    list(new.output()) + list(new.adds()) + list(new.mults()[1:]) + list(new.left())):
        assert np.array_equal(u, v)
    old.free()
    new.free()


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (0, 2, 1, 3, 4)])
def test_fcs_degenerate_points(ctx, order):
    """K = 5, N = 2.  X[0] = X[1] under (3, -3) in column 0 only: a partial sum cancels, C[0] survives.  X[2] = -X[3] under
    (4, -4): both terms are 4 X[2], a doubling.  A weight row of zeros (s_4 = 0, T_4 the identity, rz = 1).  A bias equal to
    -C[1]: that output is the identity.  The second order (rows 1 and 2 swapped) puts the equal and the opposite terms into lanes
    k and k + 2, which the workgroup's tree adds to each other directly"""
    K, N = 5, 2
    A, B, D = FM.log_point(5), FM.log_point(77), FM.log_point(123456789)
    X = [[A, A, B, neg(B), D][i] for i in order]
    W = [[[3, 6], [-3, 6], [4, 2], [-4, 5], [0, 0]][i] for i in order]
    C1 = FM.POINTS.add(FM.POINTS.mul(12, A), FM.POINTS.mul(3, neg(B)))  # 6 A + 6 A + 2 B - 5 B
    bias = [B, neg(C1)]
    tr = fcs_points(ctx, [X], K, W, N, [bias], KEYS[:1], 13)
    exp = TM.fc_signed(TM.POINTS, [X], K, W, N, [bias], KEYS[:1], 13)
    assert exp["out"][0] == [FM.POINTS.add(FM.log_point(8 * 77), B), None]  # C[0] = 8 B
    assert exp["mults"][4][0] == 0 and exp["adds"][-1][1] is None
    assert_output(tr, exp["out"])
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"])
    assert [int(v) for v in tr.adds()[4]] == [0, 0, 0, 0, 0, 1]
    tr.free()


def test_fcs_rejections(ctx):
    import vpin_amd
    K, N = 3, 2
    pts = [FM.log_point(k) for k in FM.synthetic_logs(0xF502, K + N)]
    X, bias, W = pts[:K], pts[K:], [[1, -2], [3, 4], [-5, 6]]

    def rejected(X=X, bias=bias, W=W, prf_bytes=13):
        with pytest.raises(vpin_amd.VpinError) as ei:
            fcs_points(ctx, [X], K, W, N, [bias], KEYS[:1], prf_bytes)
        return ei.value.code, str(ei.value)

    code, msg = rejected(X=[X[0], X[0], X[2]], W=[[3, 1], [-3, 1], [0, 1]])  # a cancelling column, by plain inputs
    assert code == -5 and "C[j] is the identity" in msg and "vpin_enc_fc_signed" in msg
    code, msg = rejected(X=[X[0], None, X[2]])
    assert code == -5 and "X[k] is the identity" in msg
    code, msg = rejected(W=[[-(1 << 31)] * 2] * 3, prf_bytes=16)
    assert code == -5 and "128 bits" in msg
    code, msg = rejected(bias=[bias[0], (bias[1][0], (bias[1][1] + 1) % Q)])
    assert code == -1 and "bias point is not on the curve" in msg
    code, msg = rejected(prf_bytes=0)
    assert code == -1 and "prf_bytes" in msg
    tr = fcs_points(ctx, [X], K, W, N, [bias], KEYS[:1], 13)  # the same inputs unspoilt are accepted
    assert (tr.n_mult, tr.n_add) == (3, 4)
    tr.free()


def test_fcs_through_to_two_proofs(ctx):
    P, K, N = 2, 5, 2
    tr, exp = run_log_fcs(ctx, 0xF503, P, K, signed_matrix(K, N), N, 13)
    assert (tr.n_mult, tr.n_add) == (10, 12)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], FM.base_point)
    gm, ga = tr.instances()
    w, mx, my = tr.mults()
    prove_and_compare(ctx, [(gm, ctx.gadget_point_mult_dev(w, mx, my)), (ga, ctx.gadget_point_add_dev(*tr.adds()))])
    tr.free()
