"""The model of the encrypted fully connected and average-pooling layers (tests/enc_fc_model.py) without a GPU: its literal
(points) and discrete-log forms agree, the operation counts are LeNet's (labels L2, L4, L6, L7), the 128-bit rule of the folded
weights, and the two entry points of the library: exported, and VPIN_EINVAL for a NULL context."""
import ctypes as C

import pytest

import enc_fc_model as FM

KEYS = [bytes((13 * p + 5 * i + 1) % 256 for i in range(32)) for p in range(2)]


def test_literal_and_discrete_log_models_agree_fc():
    P, K, N = 1, 3, 2
    W = [[3, 0], [1, 70000], [2, 5]]
    logs = FM.synthetic_logs(0xFC, K + N)
    rl = FM.fc(FM.LOGS, [logs[:K]], K, W, N, [logs[K:]], KEYS[:1], 13)
    pts = [FM.log_point(k) for k in logs]
    rp = FM.fc(FM.POINTS, [pts[:K]], K, W, N, [pts[K:]], KEYS[:1], 13)
    assert [FM.log_point(k) for k in rl["out"][0]] == rp["out"][0]
    assert FM.log_point(rl["left"][0]) == rp["left"][0]
    assert [(s, FM.log_point(x)) for s, x in rl["mults"]] == rp["mults"]
    assert [(FM.log_point(a), FM.log_point(b)) for a, b in rl["adds"]] == rp["adds"]
    assert len(rp["mults"]) == P * K and len(rp["adds"]) == P * (N + K - 1)
    assert rp["adds"][0][1] == pts[K] and rp["mults"][1][1] == pts[1]  # (C[0], bias[0]) first; X[1] is the second operand


def test_literal_and_discrete_log_models_agree_pool():
    H = W = 4
    logs = FM.synthetic_logs(0x9001, H * W)
    logs[5] = 0  # an identity at e_3 of the first window
    rl = FM.avgpool(FM.LOGS, [logs], H, W, 2, 2, 256)
    rp = FM.avgpool(FM.POINTS, [[FM.log_point(k) for k in logs]], H, W, 2, 2, 256)
    assert [FM.log_point(k) for k in rl["out"][0]] == rp["out"][0] and len(rp["out"][0]) == 4
    assert [(FM.log_point(a), FM.log_point(b)) for a, b in rl["adds"]] == rp["adds"]
    assert len(rp["adds"]) == 12 and rp["adds"][2][1] is None


def test_fixed_base_points_are_log_points():
    for k in (0, 1, 15, 16, 0xFC, FM.ORDER - 1, FM.ORDER + 5, FM.synthetic_logs(3, 1)[0] << 130):
        assert FM.base_point(k) == FM.log_point(k)


@pytest.mark.parametrize("P,K,N,n_mult,n_add", [(2, 120, 84, 240, 406), (2, 84, 10, 168, 186)])
def test_fc_counts_are_lenets(P, K, N, n_mult, n_add):
    logs = FM.synthetic_logs(K * N, P * (K + N))
    W = [[(7 * k + 3 * j + 1) % 251 for j in range(N)] for k in range(K)]
    r = FM.fc(FM.LOGS, [logs[p * K:(p + 1) * K] for p in range(P)], K, W, N,
              [logs[P * K + p * N:P * K + (p + 1) * N] for p in range(P)], KEYS, 13)  # 16 PRF bytes would leave 128 bits
    assert (len(r["mults"]), len(r["adds"])) == (n_mult, n_add)
    assert [len(o) for o in r["out"]] == [N] * P and len(r["left"]) == P


@pytest.mark.parametrize("P,H,W,n_add", [(12, 28, 28, 7056), (32, 10, 10, 2400)])
def test_pool_counts_are_lenets(P, H, W, n_add):
    logs = FM.synthetic_logs(H, P * H * W)
    r = FM.avgpool(FM.LOGS, [logs[p * H * W:(p + 1) * H * W] for p in range(P)], H, W, 2, 2, 256)
    assert len(r["adds"]) == n_add and [len(o) for o in r["out"]] == [(H // 2) * (W // 2)] * P


def test_folded_weights_of_the_13_byte_prf_fit():
    """84 terms below 2^104 * 2^14: below 2^125"""
    K, N = 2, 84
    logs = FM.synthetic_logs(13, K + N)
    W = [[2**14 - 1 - (k + j) for j in range(N)] for k in range(K)]
    r = FM.fc(FM.LOGS, [logs[:K]], K, W, N, [logs[K:]], KEYS[:1], 13)
    assert all(s < 2**125 for s, _ in r["mults"]) and max(s for s, _ in r["mults"]) >= 2**110


def test_folded_weights_past_128_bits_are_a_shape_error():
    K, N = 2, 2
    logs = FM.synthetic_logs(16, K + N)
    with pytest.raises(FM.ShapeError, match="128 bits"):
        FM.fc(FM.LOGS, [logs[:K]], K, [[0xFFFFFFFF] * N] * K, N, [logs[K:]], KEYS[:1], 16)


def test_library_exports_the_two_layers():
    import vpin_amd
    L = vpin_amd.lib()
    assert hasattr(L, "vpin_enc_fc") and hasattr(L, "vpin_enc_avgpool2d")
    assert {"vpin_enc_fc", "vpin_enc_avgpool2d"} <= set(vpin_amd.declared_symbols())


def test_null_context_is_einval():
    import vpin_amd
    L = vpin_amd.lib()
    buf = (C.c_uint8 * 64)()
    b = C.cast(buf, C.c_void_p)
    h = C.c_void_p(1)
    assert L.vpin_enc_fc(None, b, b, b, 1, 1, b, 1, b, b, b, b, 16, C.byref(h)) == -1
    assert not h.value and b"null" in L.vpin_last_error()
    h = C.c_void_p(1)
    assert L.vpin_enc_avgpool2d(None, b, b, b, 1, 1, 1, 1, 1, b, C.byref(h)) == -1
    assert not h.value and b"null" in L.vpin_last_error()
