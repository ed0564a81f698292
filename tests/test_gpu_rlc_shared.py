"""The layers' random-linear-combination sums through the shared-scalar bucket walk (e2_msm_shared.hip): vpin_enc_conv2d,
vpin_enc_conv2d_mc and vpin_enc_conv2d_mc_bias on both sides of the selection rule, every case against the Python models byte for
byte (output, both lists, left sides; the helpers of the existing GPU test modules), and vpin_ctx_rlc_shared_sums moving by
exactly the number of sums the rule, restated here, sends to the walk -- and by zero on the other side."""
import pytest

import convmc_model as CM
import enc_conv_model as EM
from test_gpu_enc_conv import KEYS as CONV_KEYS
from test_gpu_enc_conv import assert_lists, points_of, run_log_layer, to_arrays
from test_gpu_enc_convmc import KEYS, check_log_layer, pixels
from test_gpu_enc_convmc_bias import check_log_layer as check_bias_layer

pytestmark = pytest.mark.gpu

MIN_SUMS_PER_VECTOR, MIN_TERMS = 17, 9  # e2_rlc_shared_wins


def walk_takes(sums_per_vector, n_terms, prf_bytes):
    return sums_per_vector >= MIN_SUMS_PER_VECTOR and n_terms >= MIN_TERMS and 8 * prf_bytes >= 3


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def mc_expected_sums(G_, C, n_out, connect, f, H, W, pad, stride, prf_bytes):
    """the sums of the trained layer's check: per pair the chain padded to the longest row of the table, and the left side"""
    k_max = max(len(r) for r in CM.connected(connect, n_out, C)) * f * f
    oh, ow = EM.out_dims(H, W, f, f, pad, stride)
    return G_ * n_out * (k_max + 1) if walk_takes(k_max + 1, oh * ow, prf_bytes) else 0


# (groups, C, n_out, H, W, f, pad, stride, table, prf_bytes, the walk takes it)
MC_CASES = {
    "walk_19_sums_9_terms": (2, 2, 2, 5, 5, 3, 0, 1, None, 16, True),
    "old_9_sums": (2, 2, 2, 5, 5, 2, 0, 1, None, 16, False),               # 2 * 4 + 1 sums a vector: below the rule
    "old_4_terms": (1, 2, 2, 4, 4, 3, 0, 1, None, 16, False),              # 19 sums a vector of 4 terms: below the rule
    "walk_unequal_chains": (1, 3, 2, 5, 5, 3, 0, 1, [[1, 1, 1], [1, 0, 1]], 13, True),  # chains of 27 and 18: padded descriptors
    "walk_groups_4_pad_stride": (4, 2, 2, 7, 6, 3, 1, 2, None, 16, True),  # B = 2; windows reach into the padding
    "walk_one_byte_scalars": (1, 2, 1, 5, 5, 3, 0, 1, None, 1, True),      # scalar_bits 8: three windows
}


@pytest.mark.parametrize("name", sorted(MC_CASES))
def test_trained_layer_on_both_sides_of_the_rule(ctx, name):
    G_, C, n_out, H, W, f, pad, stride, table, prf_bytes, walk = MC_CASES[name]
    x, y, inf, logs = pixels(0xD0 + len(name), G_ * C, H, W)
    weights = [[CM._signed(0x40 + C * o + c, f * f, 1 << 17) for c in range(C)] for o in range(n_out)]
    assert any(w < 0 for o in weights for c in o for w in c)
    before = ctx.rlc_shared_sums()
    tr, _ = check_log_layer(ctx, x, y, inf, logs, G_, C, n_out, H, W, weights, table, f, pad, stride, prf_bytes)
    took = ctx.rlc_shared_sums() - before
    assert took == mc_expected_sums(G_, C, n_out, table, f, H, W, pad, stride, prf_bytes) and (took > 0) == walk
    tr.free()


@pytest.mark.parametrize("f,walk", [(3, True), (2, False)])
def test_trained_layer_with_a_bias(ctx, f, walk):
    G_, C, n_out, H, W = 2, 2, 2, 5, 5
    x, y, inf, logs = pixels(0xE0 + f, G_ * C, H, W)
    for p, i in ((0, 3), (3, 24)):  # flagged pixels inside the windows
        inf[p, i], logs[p][i] = 1, 0
    weights = [[CM._signed(0x50 + C * o + c, f * f) for c in range(C)] for o in range(n_out)]
    before = ctx.rlc_shared_sums()
    tr, _ = check_bias_layer(ctx, x, y, inf, logs, EM.synthetic_logs(0xE00, G_ * n_out), G_, C, n_out, H, W, weights, None, f)
    took = ctx.rlc_shared_sums() - before
    assert took == mc_expected_sums(G_, C, n_out, None, f, H, W, 0, 1, 16) and (took > 0) == walk
    tr.free()


@pytest.mark.parametrize("P,H,W,f,pad,stride,prf_bytes,walk", [(2, 7, 7, 4, 0, 1, 16, True), (3, 9, 8, 4, 1, 2, 13, True), (2, 7, 7, 3, 0, 1, 16, False),
                                                               (1, 5, 5, 4, 0, 1, 16, False)])
def test_one_filter_layer_on_both_sides_of_the_rule(ctx, P, H, W, f, pad, stride, prf_bytes, walk):
    """f 4: 17 sums a plane; 7 x 7 gives 16 terms, 9 x 8 under pad 1 / stride 2 gives 4 x 4 with windows in the padding; f 3: ten
    sums a plane and 5 x 5 under f 4: four terms, both below the rule"""
    filt = [(7 * k + 1) % 11 for k in range(f * f)]
    assert filt[0] and 0 in filt
    oh, ow = EM.out_dims(H, W, f, f, pad, stride)
    assert walk == walk_takes(f * f + 1, oh * ow, prf_bytes)
    before = ctx.rlc_shared_sums()
    tr, exp = run_log_layer(ctx, 0xF00 + H + f, P, H, W, filt, f, f, pad, stride, prf_bytes)
    assert ctx.rlc_shared_sums() - before == (P * (f * f + 1) if walk else 0)
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == [EM.log_point(k) for plane in exp["out"] for k in plane]
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], EM.log_point)
    tr.free()


def test_a_layer_that_must_refuse_still_refuses(ctx):
    """an identity B'[k] on shapes the walk takes: the same code and text as before (tests/test_gpu_enc_convmc.py, test_gpu_enc_conv.py)"""
    import vpin_amd
    G_, C, n_out, H, W, f = 1, 2, 1, 5, 5, 3
    x, y, inf, _ = pixels(0xC7, G_ * C, H, W)
    inf[1, :] = 1
    weights = [[CM._signed(0x60 + c, f * f) for c in range(C)]]
    before = ctx.rlc_shared_sums()
    with pytest.raises(vpin_amd.VpinError, match=r"vpin_enc_conv2d_mc: a multiplication operand B'\[c\]\[k\] is the identity") as e:
        ctx.enc_conv2d_mc(x, y, inf, G_, C, n_out, H, W, weights, None, f, f, 0, 1, KEYS[:1], 16)
    assert e.value.code == -5 and ctx.rlc_shared_sums() - before == 19
    px, py, pinf = to_arrays([None] * 49)
    with pytest.raises(vpin_amd.VpinError, match=r"vpin_enc_conv2d: a multiplication operand B'\[k\] is the identity") as e:
        ctx.enc_conv2d(px, py, pinf, 1, 7, 7, list(range(1, 17)), 4, 4, 0, 1, CONV_KEYS[:1], 16)
    assert e.value.code == -5 and ctx.rlc_shared_sums() - before == 19 + 17
