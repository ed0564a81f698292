"""The model of the trained convolution layer (tests/convmc_model.py) without a GPU: anchored to the reference's recorded
convolution runs (tests/golden/layer_pins.json) in the degenerate case C = n_out = 1, against lenet_model's plane sums followed by
the one-filter convolution, the sign rule against the point-mult gadget model, decryption against the plaintext convolution, the
declared symbols, vpin_net_cfg_counts for the new layer kind, and the magnitudes of the network tests/test_gpu_net_convmc.py runs."""
import numpy as np
import pytest

import convmc_model as CM
import enc_conv_model as EM
import gadgets_model as GM
import lenet_model as LM
import net_model as NM
import oracle_lib as O
from test_layer_pins import CONV_NAMES, case, keys_of, lists_of, pts

KEYS = [bytes((29 * p + 5 * i + 1) % 256 for i in range(32)) for p in range(8)]


@pytest.mark.parametrize("name", CONV_NAMES[1:])
def test_degenerate_case_reproduces_the_references_recorded_run(name):
    """C = 1, n_out = 1, groups = P, the recorded non-negative filter: outputs, both lists and left sides byte for byte (the two
    runs of the convolution service: pad 1, and stride 2; the literal model needs 16 s for the third, LeNet's 7 x 6)"""
    c = case("conv", name)
    mults, adds = lists_of(c)
    planes = [pts(p) for p in c["input"]]
    assert all(w >= 0 for w in c["filter"])
    got = CM.layer(CM.POINTS, planes, 1, 1, c["H"], c["W"], [[list(c["filter"])]], None, c["fh"], c["fw"], c["pad"], c["stride"], keys_of(c),
                   c["prf_bytes"])
    assert got["out"] == [pts(o) for o in c["output"]], "output ciphertext"
    assert got["mults"] == mults, "multiplication list"
    assert got["adds"] == adds, "addition list (None where the reference added the identity)"
    assert got["left"] == pts(c["left"]), "left sides"
    assert CM.trace_counts(len(planes), 1, 1, None, c["fh"], c["fw"]) == (len(mults), len(adds))


TABLE = [[1, 1, 0], [0, 1, 1], [1, 1, 1]]
FILT = [2, 0, 1, 3]


def test_table_times_filter_is_plane_sums_then_the_one_filter():
    """W[o][c] = connect[o][c] * filter: the outputs are lenet_model's plane sums through enc_conv_model's convolution"""
    H, W, C = 4, 5, 3
    logs = EM.synthetic_logs(0x3C3, 2 * C * H * W)
    planes = [logs[p * H * W:(p + 1) * H * W] for p in range(2 * C)]
    weights = [[[on * w for w in FILT] for on in row] for row in TABLE]
    garbage = [[[w if on else 977 for w in FILT] for on in row] for row in TABLE]
    want = []
    for g in range(2):
        for s in LM.plane_sums(EM.LOGS, planes[g * C:(g + 1) * C], TABLE):
            want.append(EM.conv2d(EM.LOGS, s, H, W, FILT, 2, 2, 0, 1))
    assert CM.conv2d_mc(CM.LOGS, planes, C, 3, H, W, weights, None, 2, 2, 0, 1) == want  # zeros where unconnected
    assert CM.conv2d_mc(CM.LOGS, planes, C, 3, H, W, garbage, TABLE, 2, 2, 0, 1) == want  # the table: those weights are not read
    res = CM.layer(CM.LOGS, planes, C, 3, H, W, garbage, TABLE, 2, 2, 0, 1, KEYS[:6], 16)
    assert res["out"] == want
    assert (len(res["mults"]), len(res["adds"])) == CM.trace_counts(2, C, 3, TABLE, 2, 2) == (2 * 4 * 7, 2 * 4 * 7 - 6)


def test_negative_weight_records_the_negated_point_and_satisfies_the_gadget():
    H = W = 3
    logs = EM.synthetic_logs(0x51, H * W)
    weights = [[[3, -5, 0, 2]]]
    res = CM.layer(CM.LOGS, [logs], 1, 1, H, W, weights, None, 2, 2, 0, 1, KEYS[:1], 16)
    lit = CM.layer(CM.POINTS, [[EM.log_point(k) for k in logs]], 1, 1, H, W, weights, None, 2, 2, 0, 1, KEYS[:1], 16)
    assert [(w, EM.log_point(s)) for w, s in res["mults"]] == lit["mults"] and [w for w, _ in res["mults"]] == [3, 5, 0, 2]
    assert [(EM.log_point(a), EM.log_point(t)) for a, t in res["adds"]] == lit["adds"] and lit["adds"][1][1] is None  # the zero weight
    w, S = lit["mults"][1]
    r = [EM.prf(KEYS[0], t, 16) for t in range(4)]
    Bp = EM.log_point(sum(r[t] * logs[(t // 2) * W + t % 2 + 1] for t in range(4)))  # tap 1: the column to the right
    assert w == 5 and S == (Bp[0], GM.Q - Bp[1]), "(|w|, -B') with -B' = (x, q - y)"
    g = GM.build_point_mult([(w, S[0], S[1])])
    assert O.is_sat(GM.instance_new(g)) == 1
    n = 128
    assert (g["vars_input"][10 * n + 6], g["vars_input"][10 * n + 7]) == lit["adds"][0][1] == GM.e2_mul(5, S)  # the gadget's product is T_1
    assert lit["adds"][0][1] == EM.log_point(-5 * sum(r[t] * logs[(t // 2) * W + t % 2 + 1] for t in range(4)))


def test_output_decrypts_to_the_plaintext_convolution():
    """pad 1, stride 2, 5 x 4, f 3, a table: both ciphertext halves through the model, then c2 - sk * c1"""
    C, n_out, H, W, f, sk = 2, 3, 5, 4, 3, 0x1F2E3D4C5B6A7988
    msgs = [(7 * i * i + 3 * i) % 41 - 20 for i in range(C * H * W)]
    rs = EM.synthetic_logs(0x77, C * H * W)
    c1, c2 = NM.log_encrypt(sk, msgs, rs)
    table = [[1, 0], [1, 1], [0, 1]]
    weights = [[CM._signed(0x900 + 2 * o + c, f * f, 1 << 17) for c in range(C)] for o in range(n_out)]
    assert min(min(w) for r in weights for w in r) < 0 and max(max(w) for r in weights for w in r) >= 1 << 16
    planes = [c[p * H * W:(p + 1) * H * W] for c in (c1, c2) for p in range(C)]
    res = CM.layer(CM.LOGS, planes, C, n_out, H, W, weights, table, f, f, 1, 2, KEYS[:6], 13)
    half = len(res["out"]) // 2
    got = []
    for a, b in zip(res["out"][:half], res["out"][half:]):
        v = [(y - sk * x) % EM.ORDER for x, y in zip(a, b)]
        got.append([x - EM.ORDER if x > EM.ORDER // 2 else x for x in v])
    want = CM.plain_conv2d_mc(np.array(msgs, dtype=object).reshape(C, H, W), weights, table, f, f, 1, 2)
    assert EM.out_dims(H, W, f, f, 1, 2) == (3, 2) and got == [[int(v) for v in p.reshape(-1)] for p in want]
    assert any(v < 0 for p in got for v in p)


def test_model_rejections():
    logs = EM.synthetic_logs(5, 2 * 9)
    planes = [logs[:9], logs[9:]]
    w = [[[1, 2, 3, 4], [5, 6, 7, 8]]]
    with pytest.raises(CM.ShapeError, match="accumulator"):  # a zero first weight
        CM.layer(CM.LOGS, planes, 2, 1, 3, 3, [[[0, 2, 3, 4], [5, 6, 7, 8]]], None, 2, 2, 0, 1, KEYS[:1], 16)
    with pytest.raises(CM.ShapeError, match="B'"):  # an all-identity connected channel
        CM.layer(CM.LOGS, [logs[:9], [0] * 9], 2, 1, 3, 3, w, None, 2, 2, 0, 1, KEYS[:1], 16)
    with pytest.raises(ValueError):
        CM.layer(CM.LOGS, planes, 2, 1, 3, 3, w, [[0, 0]], 2, 2, 0, 1, KEYS[:1], 16)
    # a spoilt output: the two sides differ (VPIN_EVERIFY has no way in from outside on the device)
    real = CM.conv2d_mc
    try:
        def spoilt(*a):
            out = real(*a)
            out[0][0] = (out[0][0] + 1) % EM.ORDER
            return out
        CM.conv2d_mc = spoilt
        with pytest.raises(CM.VerifyError):
            CM.layer(CM.LOGS, planes, 2, 1, 3, 3, w, None, 2, 2, 0, 1, KEYS[:1], 16)
    finally:
        CM.conv2d_mc = real


def test_symbols_are_declared_and_exported():
    import vpin_amd
    from vpin_amd import capi, net
    names = ["vpin_enc_conv2d_mc", "vpin_e2_conv2d_mc"]
    assert all(n in capi.declared_symbols() for n in names) and all(n in capi.exported_symbols() for n in names)
    assert capi.lib().vpin_abi_version() >= 3 and net.CONVMC == 3
    assert [f[0] for f in capi.NetLayer._fields_][-3:] == ["n_out", "w_mc", "connect"]
    assert hasattr(vpin_amd.Context, "enc_conv2d_mc") and hasattr(vpin_amd.Context, "e2_conv2d_mc")
    assert hasattr(net.Config, "convmc")


device_config = CM.device_config


def test_net_cfg_counts_count_the_trained_convolution():
    """vpin_net_cfg_counts needs no GPU"""
    import vpin_amd
    cfg = CM.lenet_shaped_config()
    want = CM.net_counts(cfg)
    assert want["layers"] == [(36, 32), (0, 192), (32, 26), (54, 60), (8, 12)] and want["prf_keys"] == 4 + 6 + 2 + 2
    assert want["per_round"] == [128, 32, 27, 4, 3] and want["bias_r"] == 7
    got = device_config(cfg, [1 << 14] * 5).counts()
    assert got == dict(want, rounds=5)
    bad = dict(cfg, layers=[dict(l) for l in cfg["layers"]])
    bad["layers"][2]["connect"] = [[1, 0], [0, 0], [0, 1]]
    no_row, no_out = device_config(bad, [1 << 14] * 5), device_config(cfg, [1 << 14] * 5)
    no_out.layers[2].n_out = 0
    for dev, match in ((no_row, "selects no channel"), (no_out, "zero")):
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            dev.counts()
        assert e.value.code == -1


def test_network_magnitudes_stay_below_2_to_30():
    """the condition on tests/test_gpu_net_convmc.py's inputs: with max_giant = 2^14 over 2^16 baby steps every round's walk is short"""
    cfg = CM.lenet_shaped_config()
    image = CM.lenet_shaped_image()
    assert image.shape == (10, 10)
    vs, acts = CM.net_plaintext(cfg, image)
    mags = [max(abs(v) for v in r) for r in vs]
    print("largest |v| per round:", mags)
    assert len(vs) == 5 and all(m < 1 << 30 for m in mags)
    assert all(abs(w) < 16 for l in cfg["layers"] if l["kind"] == "convmc" for o in l["w"] for c in o for w in c)
    assert any(w < 0 for o in cfg["layers"][0]["w"] for c in o for w in c) and any(w < 0 for o in cfg["layers"][2]["w"] for c in o for w in c)
    assert any(v < 0 for v in vs[0]) and any(v > 0 for v in acts[-1]), "signed values reach the client and the result is not all zero"
    assert all(any(v != 0 for v in a) for a in acts), "no round zeroes the network"
