"""The model of the encrypted convolution layer (tests/enc_conv_model.py) without a GPU: the PRF's known answer from Python's
hmac, and the literal (points) and discrete-log forms of the model agreeing on a tiny layer."""
import enc_conv_model as EM

KAT_KEY = bytes(range(32))
KAT_HEX = "43c875c1027e0bb60b3c5e055d7245be"


def test_prf_known_answer():
    assert EM.prf(KAT_KEY, 7, 16) == int(KAT_HEX, 16)
    assert EM.prf(KAT_KEY, 7, 13) == int(KAT_HEX[:26], 16)


def test_literal_and_discrete_log_models_agree():
    H, W, fh, fw, pad, stride = 3, 2, 2, 2, 1, 1
    filt = [3, 0, 1, 2]
    logs = EM.synthetic_logs(0x1234, H * W)
    logs[3] = 0  # an identity pixel
    keys = [bytes((7 * i + 1) % 256 for i in range(32))]
    rl = EM.layer(EM.LOGS, [logs], H, W, filt, fh, fw, pad, stride, keys, 13)
    rp = EM.layer(EM.POINTS, [[EM.log_point(k) for k in logs]], H, W, filt, fh, fw, pad, stride, keys, 13)
    assert EM.out_dims(H, W, fh, fw, pad, stride) == (4, 3) and len(rl["out"][0]) == 12
    assert [EM.log_point(k) for k in rl["out"][0]] == rp["out"][0]
    assert EM.log_point(rl["left"][0]) == rp["left"][0]
    assert [(w, EM.log_point(b)) for w, b in rl["mults"]] == rp["mults"]
    assert [(EM.log_point(a), EM.log_point(t)) for a, t in rl["adds"]] == rp["adds"]
    assert len(rp["mults"]) == 4 and len(rp["adds"]) == 3 and rp["adds"][0][1] is None  # the zero tap: T_1 is the identity
