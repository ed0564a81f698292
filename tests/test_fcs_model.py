"""The models of the signed fully connected layer and of the biased trained convolution (tests/fcs_model.py) without a GPU:
anchored to enc_fc_model.fc (which tests/test_layer_pins.py pins to the reference's recorded runs) on non-negative weights and to
convmc_model.layer without a bias, the sign rule and a bias addition against the gadget models, the rejections, the declared
symbols, vpin_net_cfg_counts for VPIN_NET_FCS and a biased CONVMC, and the magnitudes of the network tests/test_gpu_net_trained.py runs."""
import pytest

import convmc_model as CM
import enc_conv_model as EM
import enc_fc_model as FM
import fcs_model as TM
import gadgets_model as GM
import net_model as NM
import oracle_lib as O

KEYS = [bytes((31 * p + 7 * i + 3) % 256 for i in range(32)) for p in range(8)]


def rows_of(seed, P, K, N):
    logs = EM.synthetic_logs(seed, P * (K + N))
    return [logs[p * K:(p + 1) * K] for p in range(P)], [logs[P * K + p * N:P * K + (p + 1) * N] for p in range(P)]


def test_non_negative_weights_give_the_unsigned_layer():
    P, K, N = 2, 5, 3
    W = [[1 + 7 * (k * N + j) for j in range(N)] for k in range(K)]
    W[2] = [0, 0, 0]
    rows, biases = rows_of(0x5F1, P, K, N)
    assert TM.fc_signed(TM.LOGS, rows, K, W, N, biases, KEYS[:P], 13) == FM.fc(FM.LOGS, rows, K, W, N, biases, KEYS[:P], 13)


def test_signed_layer_decrypts_to_the_plaintext_product():
    K, N, sk = 6, 3, 0x1F2E3D4C5B6A7988
    W = [CM._signed(0x600 + k, N, 1 << 17) for k in range(K)]
    assert min(min(r) for r in W) < 0 < max(max(r) for r in W)
    msgs, bias = [(5 * i * i + i) % 37 - 18 for i in range(K)], [100, -2000, 0]
    c1, c2 = NM.log_encrypt(sk, msgs, EM.synthetic_logs(0x601, K))
    b1, b2 = NM.log_encrypt(sk, bias, EM.synthetic_logs(0x602, N))
    res = TM.fc_signed(TM.LOGS, [c1, c2], K, W, N, [b1, b2], KEYS[:2], 13)
    v = [(y - sk * x) % EM.ORDER for x, y in zip(*res["out"])]
    assert [x - EM.ORDER if x > EM.ORDER // 2 else x for x in v] == [sum(msgs[k] * W[k][j] for k in range(K)) + bias[j] for j in range(N)]


def test_negative_folded_weight_records_the_negated_point_and_satisfies_the_gadgets():
    """P = 1, K = 3, N = 2 on points: s_1 < 0 records (|s_1|, (x, q - y)); the multiplication and the first bias addition through the
    gadget models"""
    K, N = 3, 2
    W = [[3, 0], [-0x1ABCD, 7], [-2, -5]]
    logs = EM.synthetic_logs(0x5F2, K + N)
    X, bias = [EM.log_point(k) for k in logs[:K]], [EM.log_point(k) for k in logs[K:]]
    lit = TM.fc_signed(TM.POINTS, [X], K, W, N, [bias], KEYS[:1], 13)
    res = TM.fc_signed(TM.LOGS, [logs[:K]], K, W, N, [logs[K:]], KEYS[:1], 13)
    assert [(w, EM.log_point(s)) for w, s in res["mults"]] == lit["mults"]
    assert [(EM.log_point(a), EM.log_point(t)) for a, t in res["adds"]] == lit["adds"]
    r = [EM.prf(KEYS[0], j, 13) for j in range(N)]
    s = [sum(r[j] * W[k][j] for j in range(N)) for k in range(K)]
    assert s[0] > 0 > s[2] and s[1] < 0, "the 13-byte r_0 times 0x1ABCD outweighs 7 r_1"
    assert lit["mults"][0] == (s[0], X[0]) and lit["mults"][1] == (-s[1], (X[1][0], GM.Q - X[1][1])) and lit["mults"][2][0] == -s[2]
    w, S = lit["mults"][1]
    g = GM.build_point_mult([(w, S[0], S[1])])
    assert O.is_sat(GM.instance_new(g)) == 1
    assert lit["adds"][N][1] == GM.e2_mul(w, S) == EM.log_point(s[1] * logs[1]), "T_1 = |s_1| * (-X[1]) = s_1 * X[1]"
    (c0, b0) = lit["adds"][0]
    assert b0 == bias[0] and lit["out"][0][0] == GM.e2_add(c0, b0)
    assert O.is_sat(GM.instance_new(GM.build_point_add([(c0[0], c0[1], b0[0], b0[1], 0)]))) == 1


def test_signed_model_rejections():
    K, N = 3, 2
    rows, biases = rows_of(0x5F3, 1, K, N)
    X = rows[0]
    good = [[1, -2], [3, 4], [-5, 6]]
    run = lambda X=X, W=good, prf_bytes=13: TM.fc_signed(TM.LOGS, [X], K, W, N, biases, KEYS[:1], prf_bytes)
    with pytest.raises(TM.ShapeError, match=r"C\[0\] is the identity"):  # reachable by plain inputs: X[0] = X[1] under w, -w
        run(X=[X[0], X[0], X[2]], W=[[3, 1], [-3, 1], [0, 1]])
    with pytest.raises(TM.ShapeError, match=r"X\[1\] is the identity"):
        run(X=[X[0], 0, X[2]])
    with pytest.raises(TM.ShapeError, match="128 bits"):  # neg_k alone leaves 128 bits
        run(W=[[-(1 << 31)] * 2] * 3, prf_bytes=16)
    with pytest.raises(TM.ShapeError, match="accumulator"):  # s_0 = 0: T_0 is the identity before T_1
        run(W=[[0, 0], [3, 4], [-5, 6]])
    real = TM.neg
    try:  # a negation that does nothing: C and the chain disagree about the signs, the two sides differ
        TM.neg = lambda grp, v: v
        with pytest.raises(TM.VerifyError):
            run()
    finally:
        TM.neg = real
    assert len(run()["adds"]) == N + K - 1


def test_bias_layer_is_the_unbiased_layer_plus_its_additions():
    G_, C, n_out, H, W = 2, 2, 2, 4, 4
    weights = [[[3, -5, 0, 70001], [-2, 1, 65536, -7]], [[-1, 0, 4, 9], [6, -66000, 0, 2]]]
    logs = EM.synthetic_logs(0x5F4, G_ * C * H * W + G_ * n_out)
    planes = [logs[p * H * W:(p + 1) * H * W] for p in range(G_ * C)]
    biases = logs[G_ * C * H * W:]
    biases[1] = 0  # an identity bias
    for table in (None, [[1, 0], [1, 1]]):
        base = CM.layer(CM.LOGS, planes, C, n_out, H, W, weights, table, 2, 2, 0, 1, KEYS[:4], 16)
        res = TM.layer_bias(TM.LOGS, planes, C, n_out, H, W, weights, table, 2, 2, 0, 1, biases, KEYS[:4], 16)
        assert res["mults"] == base["mults"] and res["left"] == base["left"]
        assert res["out"] == [[(v + biases[q]) % EM.ORDER for v in plane] for q, plane in enumerate(base["out"])]
        assert (len(res["mults"]), len(res["adds"])) == TM.bias_trace_counts(G_, C, n_out, table, 2, 2, 3, 3)
        want, pos = [], 0
        for q in range(G_ * n_out):  # per pair: its 9 bias additions, then its chain of 4 * (connected channels) - 1
            n = 4 * (C if table is None else sum(table[q % n_out])) - 1
            want += [(v, biases[q]) for v in base["out"][q]] + base["adds"][pos:pos + n]
            pos += n
        assert res["adds"] == want and pos == len(base["adds"])
    with pytest.raises(TM.ShapeError, match=r"C\[\d+\] of plane 0 is the identity"):  # channels P and -P under equal weights
        opposite = [planes[0], [(-k) % EM.ORDER for k in planes[0]]]
        TM.layer_bias(TM.LOGS, opposite, 2, 1, H, W, [[[4, -9, 6, 2]] * 2], None, 2, 2, 0, 1, biases[:1], KEYS[:1], 16)


def test_symbols_are_declared_and_exported():
    import vpin_amd
    from vpin_amd import capi, net
    names = ["vpin_enc_fc_signed", "vpin_enc_conv2d_mc_bias"]
    assert all(n in capi.declared_symbols() for n in names) and all(n in capi.exported_symbols() for n in names)
    assert capi.lib().vpin_abi_version() >= 4 and net.FCS == 4
    assert hasattr(vpin_amd.Context, "enc_fc_signed") and hasattr(vpin_amd.Context, "enc_conv2d_mc_bias")
    assert hasattr(net.Config, "fcs") and hasattr(net, "lenet5_config")


def test_net_cfg_counts_count_the_signed_layer_and_the_bias():
    """vpin_net_cfg_counts needs no GPU"""
    cfg = TM.trained_config()
    want = TM.net_counts(cfg)
    plain = CM.net_counts(CM.lenet_shaped_config())
    assert want["layers"] == [(36, 32 + 2 * 2 * 64), (0, 192), (32, 26 + 2 * 3 * 9), (54, 60), (8, 12)]
    assert want["bias_r"] == plain["bias_r"] + 2 + 3 and want["prf_keys"] == plain["prf_keys"] and want["per_round"] == plain["per_round"]
    assert TM.device_config(cfg, [1 << 14] * 5).counts() == dict(want, rounds=5)
    unbiased = dict(cfg, layers=[{k: v for k, v in l.items() if k != "bias" or l["kind"] != "convmc"} for l in cfg["layers"]])
    assert TM.device_config(unbiased, [1 << 14] * 5).counts() == dict(plain, rounds=5), "bias = NULL: the counts of the unbiased network"


def test_lenet5_config_counts_at_full_size():
    want = TM.net_counts(TM.lenet5_model_config())
    assert want["layers"][0] == (2 * 6 * 25, 2 * 6 * 25 - 12 + 9408) and want["layers"][4] == (800, 2 * (120 + 399))
    assert want["per_round"] == [4704, 1176, 1600, 400, 120, 84, 10] and want["bias_r"] == 6 + 16 + 120 + 84 + 10
    dev = TM.lenet5_device_config([1] * 7)
    from vpin_amd import net
    assert [l.kind for l in dev.layers] == [net.CONVMC, net.POOL, net.CONVMC, net.POOL, net.FCS, net.FCS, net.FCS]
    assert dev.counts() == dict(want, rounds=7)


def test_network_magnitudes_stay_below_2_to_30():
    """the condition on tests/test_gpu_net_trained.py's inputs: with max_giant = 2^14 over 2^16 baby steps every round's walk is short"""
    cfg = TM.trained_config()
    vs, acts = TM.net_plaintext(cfg, TM.trained_image())
    mags = [max(abs(v) for v in r) for r in vs]
    print("largest |v| per round:", mags)
    assert len(vs) == 5 and all(m < 1 << 30 for m in mags)
    assert all(any(w < 0 for row in l["w"] for w in row) for l in cfg["layers"][3:]), "the fully connected weights are signed"
    assert any(v < 0 for v in vs[0]) and any(v < 0 for v in vs[-1]) and all(any(v != 0 for v in a) for a in acts), "signed values reach the client; no round zeroes the network"
    keys = [NM.net_key(300 + i) for i in range(14)]
    assert all(TM.folded_fit_signed(l["w"], l["N"], keys[10 + 2 * j + i], cfg["prf_bytes"]) for j, l in enumerate(cfg["layers"][3:]) for i in range(2))
