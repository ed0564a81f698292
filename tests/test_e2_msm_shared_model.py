"""The model of vpin_e2_msm_shared (tests/e2_msm_shared_model.py) against the layers' models: the random-linear-combination
sums of vpin_enc_conv2d and vpin_enc_conv2d_mc are instances of the one formula.  The device's signed 3-bit recoding, restated in
the model, reconstructs every scalar at the window edges.  And the library declares and exports the new symbols (no GPU here)."""
import pytest

import convmc_model as CM
import e2_msm_shared_model as SM
import enc_conv_model as EM

KEYS = [bytes((29 * p + 13 * i + 1) % 256 for i in range(32)) for p in range(4)]
H = W = 4
F = 2


def prf_rows(keys, n_terms, prf_bytes):
    return [[EM.prf(k, t, prf_bytes) for t in range(n_terms)] for k in keys]


@pytest.mark.parametrize("pad,stride", [(0, 1), (1, 2)])
def test_the_conv_layers_sums_are_an_instance(pad, stride):
    logs = EM.synthetic_logs(0x5348, 2 * H * W)
    planes = [logs[:H * W], logs[H * W:]]
    filt = [3, 1, 4, 5]
    exp = EM.layer(EM.LOGS, planes, H, W, filt, F, F, pad, stride, KEYS[:2], 16)
    pts, off, vec, pat, base = SM.conv_instance(planes, exp["out"], H, W, F, F, pad, stride)
    sums = SM.msm_shared(EM.LOGS, prf_rows(KEYS[:2], len(exp["out"][0]), 16), pts, off, vec, pat, base)
    assert len(sums) == 2 * 5
    for p in range(2):
        assert sums[5 * p:5 * p + 4] == exp["Bp"][p]
        assert sums[5 * p + 4] == exp["left"][p]
    if pad:
        assert any(o < 0 for row in off for o in row)


def test_the_trained_layers_sums_are_an_instance():
    G_, C, n_out = 2, 2, 2
    logs = EM.synthetic_logs(0x5349, G_ * C * H * W)
    planes = [logs[p * H * W:(p + 1) * H * W] for p in range(G_ * C)]
    weights = [[[3, -5, 2, 70001], [-2, 1, 65536, -7]], [[-1, 6, 4, 9], [6, -66000, 1, 2]]]
    table = [[1, 1], [0, 1]]
    exp = CM.layer(CM.LOGS, planes, C, n_out, H, W, weights, table, F, F, 0, 1, KEYS[:4], 13)
    rows = CM.connected(table, n_out, C)
    pts, off, vec, pat, base = SM.convmc_instance(planes, exp["out"], C, n_out, rows, H, W, F, F, 0, 1)
    sums = SM.msm_shared(EM.LOGS, prf_rows(KEYS[:4], 9, 13), pts, off, vec, pat, base)
    got_S, got_left, i = [], [], 0
    for q in range(G_ * n_out):
        for c in rows[q % n_out]:
            for k in range(F * F):
                got_S.append(CM.neg(CM.LOGS, sums[i]) if weights[q % n_out][c][k] < 0 else sums[i])
                i += 1
        got_left.append(sums[i])
        i += 1
    assert i == len(sums)
    assert got_S == [m[1] for m in exp["mults"]] and got_left == exp["left"]


@pytest.mark.parametrize("scalar_bits", [8, 127, 128])
def test_the_recoding_reconstructs_the_scalar(scalar_bits):
    vals = SM.edge_values(scalar_bits)
    assert {0, 1, (1 << scalar_bits) - 1} <= set(vals)
    for k in range(0, scalar_bits, 3):  # every window edge
        assert {(1 << k) - 1, 1 << k} <= set(vals)
        assert (1 << k) + 1 in vals or k + 1 > scalar_bits
    for r in vals:
        d = SM.recode(r, scalar_bits)
        assert len(d) == SM.n_windows(scalar_bits) and all(-4 <= v <= 4 for v in d)
        assert SM.value(d) == r, hex(r)
    if scalar_bits == 128:
        d = SM.recode((1 << 128) - 1, 128)
        assert d[0] == -1 and d[-1] == 4 and not any(d[1:-1])  # 2^128 - 1 = 4 * 8^42 - 1: the carry ends in the partial top window


def test_the_number_of_windows():
    assert [SM.n_windows(b) for b in (1, 2, 3, 8, 127, 128)] == [1, 1, 2, 3, 43, 43]


def test_symbols_are_declared_and_exported():
    import vpin_amd
    from vpin_amd import build as vbuild
    vbuild.build()
    for name in ("vpin_e2_msm_shared", "vpin_ctx_rlc_shared_sums"):
        assert name in vpin_amd.declared_symbols() and name in vpin_amd.exported_symbols(), name
    assert vpin_amd.lib().vpin_abi_version() >= 11
