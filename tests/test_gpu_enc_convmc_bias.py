"""GPU parity of the trained convolution with a bias per output channel (vpin_enc_conv2d_mc_bias) with the Python model
tests/fcs_model.py: output ciphertext, both lists and the left sides byte for byte; the unbiased layer's lists inside it; the
cases of the complete addition on a bias; the rejections; and one layer through to two verified SNARKs.

The GPU is fed pixels and biases k * G from vpin_synthetic_points (negated or flagged where a case needs it) and the model the
discrete logs; expected points come from one batched conversion (lenet_model.logs_to_points)."""
import numpy as np
import pytest

import convmc_model as CM
import enc_conv_model as EM
import fcs_model as TM
import gadgets_model as GM
import lenet_model as LM
from test_gpu_enc_conv import assert_lists, points_of, to_arrays
from test_gpu_enc_convmc import KEYS, SEED_C, SEED_P, W_2x2x2, negated, pixels

pytestmark = pytest.mark.gpu

Q = GM.Q


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def check_log_layer(ctx, x, y, inf, logs, bias_logs, G_, C, n_out, H, W, weights, connect, f, prf_bytes=16):
    """the layer on the GPU against the model on logarithms (pad 0, stride 1); a bias logarithm 0 is the flagged identity.
    Returns (trace, model result)"""
    keys = KEYS[:G_ * n_out]
    bx, by, binf = to_arrays(LM.logs_to_points(bias_logs))
    tr = ctx.enc_conv2d_mc_bias(x, y, inf, G_, C, n_out, H, W, weights, connect, f, f, 0, 1, bx, by, binf, keys, prf_bytes)
    exp = TM.layer_bias(TM.LOGS, logs, C, n_out, H, W, weights, connect, f, f, 0, 1, bias_logs, keys, prf_bytes)
    oh, ow = EM.out_dims(H, W, f, f, 0, 1)
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (G_ * n_out, oh, ow) + TM.bias_trace_counts(G_, C, n_out, connect, f, f, oh, ow)
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == LM.logs_to_points([v for plane in exp["out"] for v in plane]), "output ciphertext"
    flat = [m[1] for m in exp["mults"]] + [a[0] for a in exp["adds"]] + [a[1] for a in exp["adds"]] + exp["left"]
    table = dict(zip(flat, LM.logs_to_points(flat)))
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], table.__getitem__)
    return tr, exp


@pytest.mark.parametrize("table", [None, [[1, 0], [1, 1]]])
def test_parity_and_the_unbiased_layers_lists(ctx, table):
    """groups 2, C 2, n_out 2, 4 x 4, f 2, with and without a connection table.  The multiplication list, the left sides and the
    chain additions are vpin_enc_conv2d_mc's on the same inputs and keys (under the table the pairs' chains differ in length)"""
    x, y, inf, logs = pixels(0xB1, 4, 4, 4)
    bias_logs = EM.synthetic_logs(0xB10, 4)
    tr, _ = check_log_layer(ctx, x, y, inf, logs, bias_logs, 2, 2, 2, 4, 4, W_2x2x2, table, 2)
    base = ctx.enc_conv2d_mc(x, y, inf, 2, 2, 2, 4, 4, W_2x2x2, table, 2, 2, 0, 1, KEYS[:4], 16)
    assert tr.mults()[0] == base.mults()[0]
    for u, v in zip(list(tr.mults()[1:]) + list(tr.left()), list(base.mults()[1:]) + list(base.left())):
        assert np.array_equal(u, v)
    rows, pos = [], 0
    for q in range(4):  # per pair 9 bias additions, then its chain of 4 * (connected channels) - 1
        n = 4 * (2 if table is None else sum(table[q % 2])) - 1
        rows += list(range(pos + 9, pos + 9 + n))
        pos += 9 + n
    assert pos == tr.n_add and len(rows) == base.n_add
    for u, v in zip(tr.adds(), base.adds()):
        assert np.array_equal(u[np.array(rows)], v)
    base.free()
    tr.free()


def test_degenerate_biases(ctx):
    """groups 2, n_out 2: plane 0 under an identity bias (rz = 1, out = C), plane 1 under -C[1][4] (that output is the flagged
    identity), plane 2 under C[2][0] (the addition is a doubling), plane 3 under an ordinary point"""
    x, y, inf, logs = pixels(0xB2, 4, 4, 4)
    conv = CM.conv2d_mc(CM.LOGS, logs, 2, 2, 4, 4, W_2x2x2, None, 2, 2, 0, 1)
    bias_logs = [0, (-conv[1][4]) % EM.ORDER, conv[2][0], 987654321]
    tr, exp = check_log_layer(ctx, x, y, inf, logs, bias_logs, 2, 2, 2, 4, 4, W_2x2x2, None, 2)
    assert exp["out"][1][4] == 0 and exp["out"][2][0] == 2 * conv[2][0] % EM.ORDER and exp["out"][0] == conv[0]
    oi, rz = tr.output()[2].reshape(4, 9), tr.adds()[4].reshape(4, -1)
    assert [int(v) for v in np.flatnonzero(oi)] == [9 + 4], "one flagged output"
    assert rz[0, :9].all() and not rz[1:, :9].any()
    tr.free()


def test_outputs_past_one_workgroup(ctx):
    """a 9 x 9 output plane: 81 outputs, two blocks of the bias kernel's 64 lanes, the second one short"""
    x, y, inf, logs = pixels(0xB3, 2, 10, 10)
    weights = [[CM._signed(0xB30 + c, 4) for c in range(2)]]
    tr, _ = check_log_layer(ctx, x, y, inf, logs, EM.synthetic_logs(0xB31, 1), 1, 2, 1, 10, 10, weights, None, 2)
    assert tr.oh * tr.ow == 81 and tr.n_add == 81 + 7
    tr.free()


def test_rejections(ctx):
    import vpin_amd
    x, y, inf, logs = pixels(0xB4, 2, 3, 3)
    good = [[[1, 2, 3, 4], [5, -6, 7, 8]]]
    bx, by, binf = to_arrays(LM.logs_to_points([424242]))

    def rejected(x=x, y=y, weights=good, by=by):
        with pytest.raises(vpin_amd.VpinError) as ei:
            ctx.enc_conv2d_mc_bias(x, y, inf, 1, 2, 1, 3, 3, weights, None, 2, 2, 0, 1, bx, by, binf, KEYS[:1], 16)
        return ei.value.code, str(ei.value)

    xo, yo = x.copy(), y.copy()  # channel 1 = -channel 0 under equal weights: every C[t] is the identity
    xo[1], yo[1] = x[0], negated(y[0]).reshape(y[0].shape)
    code, msg = rejected(x=xo, y=yo, weights=[[[4, -9, 6, 2]] * 2])
    assert code == -5 and "C[t] is the identity" in msg and "vpin_enc_conv2d_mc_bias" in msg
    off = by.copy()
    off[0, 0] ^= 1
    code, msg = rejected(by=off)
    assert code == -1 and "bias point is not on the curve" in msg
    code, msg = rejected(weights=[[[0, 2, 3, 4], [5, -6, 7, 8]]])  # what vpin_enc_conv2d_mc rejects, the same way
    assert code == -5 and "accumulator is the identity" in msg
    tr = ctx.enc_conv2d_mc_bias(x, y, inf, 1, 2, 1, 3, 3, good, None, 2, 2, 0, 1, bx, by, binf, KEYS[:1], 16)  # unspoilt
    assert (tr.n_mult, tr.n_add) == (8, 7 + 4)
    tr.free()


def test_layer_through_to_two_proofs(ctx):
    """groups 2, C 2, n_out 2, 4 x 4, f 2: the 32 multiplications and 28 + 36 additions through the unchanged prover and verifier"""
    x, y, inf, logs = pixels(0xB5, 4, 4, 4)
    tr, _ = check_log_layer(ctx, x, y, inf, logs, EM.synthetic_logs(0xB50, 4), 2, 2, 2, 4, 4, W_2x2x2, None, 2)
    assert (tr.n_mult, tr.n_add) == (32, 64)
    gm, ga = tr.instances()
    for g in (gm, ga):
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        g.free()
    tr.free()
