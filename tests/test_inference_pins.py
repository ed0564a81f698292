"""tests/lenet_model.py pinned to RUNS of the reference's own Python, and the plaintext LeNet to the reference's model files.

tests/golden/inference_pins.json is what the reference's functions (src/LeNet/Server.py secondConv, thirdConv, firstConv,
firstAvgPool; src/LeNet/Client.py relu, shifting, min_max_scaling, realNumbersToFixedPointRepresentation) computed when
tests/golden/make_inference_pins.py called them in the build container.  Its ciphertexts are stored as the (message, r) they
were encrypted from under a small key, so the model runs in LOGS mode (discrete logarithms) and every expected point is one
fixed-base multiplication; lists are compared through the SHA-256 the generator states.

The whole inferenceCNN at full size is not run under Python (its RLC sums would take on the order of 10^3 s in affine
arithmetic); its call order is pinned piecewise here, by the label counts and by the plaintext network below."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import enc_conv_model as EM
import enc_fc_model as FM
import lenet_model as LM
from vpin_amd import gadgets as VG

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "inference_pins.json")
GENERATOR = os.path.join(HERE, "golden", "make_inference_pins.py")
with open(FIXTURE) as f:
    PINS = json.load(f)
with open(os.path.join(HERE, "golden", "layer_pins.json")) as f:
    LAYER = json.load(f)

SK = PINS["sk"]
LENET_CONV = next(c for c in LAYER["conv"] if c["name"] == "conv_lenet_7x6")
FILT, F, PRF_BYTES = [int(w) for w in LENET_CONV["filter"]], LENET_CONV["fh"], LENET_CONV["prf_bytes"]
POOL_SCALE = int(next(c for c in LAYER["pool"] if c["service"] == "LeNet")["scale"])
MAGNITUDES = [19.1, 29.0, 24.5, 34.2, 30.0, 37.6, 38.4]  # log2 of the largest decrypted magnitude of R1 .. R7


def cipher_logs(msgs, rs):
    """pixel (m, r) -> the logs of (c1, c2) = (r G, (m + r sk) G)"""
    return [r % EM.ORDER for r in rs], [(m + r * SK) % EM.ORDER for m, r in zip(msgs, rs)]


def digest_points(logs):
    pts = LM.logs_to_points(logs)
    raw = b"".join(b"\0" * 64 if p is None else p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big") for p in pts)
    return dict(n=len(pts), sha256=hashlib.sha256(raw).hexdigest())


def digest_weights(ws):
    return dict(n=len(ws), sha256=hashlib.sha256(",".join(str(int(w)) for w in ws).encode()).hexdigest())


def assert_lists(case, res):
    if "mult_weights" in case:
        assert digest_weights([m[0] for m in res["mults"]]) == case["mult_weights"]
        assert digest_points([m[1] for m in res["mults"]]) == case["mult_points"]
    assert digest_points([a[0] for a in res["adds"]]) == case["add_p"]
    assert digest_points([a[1] for a in res["adds"]]) == case["add_r"]


def flat(planes):
    return [v for p in planes for v in p]


def test_fixture_is_whole():
    assert [c["n2"] for c in PINS["second_conv"]] == [3, 16] and PINS["multi_core_feature"] == 0
    assert PINS["third_conv"]["mult_points"]["n"] == 6000 and PINS["third_conv"]["add_p"]["n"] == 5760
    assert len(PINS["client"]["shifting_26"]["values"]) > 60 and len(PINS["client"]["shifting_33"]["values"]) > 100
    assert os.path.getsize(FIXTURE) < 200 * 1024 and len(PINS["reference_sha256"]) == 2


def test_generator_reproduces_the_fixture(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_layer_pins
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(make_layer_pins.REF, "src", "LeNet")):
        pytest.skip("the reference tree is not here")
    out = tmp_path / "pins.json"
    subprocess.run([sys.executable, GENERATOR, "--out", str(out)], check=True, capture_output=True)
    with open(FIXTURE, "rb") as f:
        assert out.read_bytes() == f.read()


def test_logs_to_points_is_base_point():
    logs = [0, 1, 2, 15, 16, EM.ORDER - 1, SK, 0xFEDCBA9876543210 * SK, 16**63, 16**63 - 1]
    assert LM.logs_to_points(logs) == [FM.base_point(k) if k else None for k in logs]
    assert FM.base_point(SK) == EM.log_point(SK)


@pytest.mark.parametrize("bits", [26, 33])
def test_shifting_pinned(bits):
    c = PINS["client"]["shifting_%d" % bits]
    vals = [int(v) for v in c["values"]]
    assert c["bits"] == bits and max(abs(v) for v in vals) > 2**24 and min(vals) < -2**24
    assert [LM.shifting(v, bits) for v in vals] == c["results"]
    # the fixture is not tame: a value one below a power of two rounds up into float32 and carries, so the integer shift is one
    # short there.  The generator puts five such values into either list; whatever else differs comes on top
    carries = [2**26 - 1, 2**30 - 1, -(2**30 - 1), 2**(bits + 14) - 1, -(2**(bits + 14) - 1)]
    assert all(LM.shift_int(v, bits) != c["results"][vals.index(v)] for v in carries)
    wrong = sum(LM.shift_int(v, bits) != r for v, r in zip(vals, c["results"]))
    assert wrong > len(carries), wrong


def test_shifting_is_numpy():
    """the integer model against numpy's own float32 path, on sizes the real network produces and on ties"""
    rng = np.random.default_rng(0x5EED)
    for bits, top in ((26, 41), (33, 48)):
        vals = [int(v) for e in range(1, top) for v in rng.integers(-2**e, 2**e, 40)]
        vals = [v for v in vals if abs(LM.f32_rn(v)) < 2**top]
        got = (np.array(vals, dtype=np.float64).astype(np.float32) / 2**bits * 2**16).astype(np.int32)
        assert [LM.shifting(v, bits) for v in vals] == [int(g) for g in got]
    assert LM.shifting(2**41, 26) is None and LM.shifting(-2**41, 26) == -2**31 and LM.shifting(2**41 - 1, 26) is None


def test_relu_and_preprocess_pinned():
    c = PINS["client"]["relu"]
    assert [str(LM.activate(int(v), True, 0)) for v in c["values"]] == c["results"]
    p = PINS["client"]["preprocess"]
    img = np.frombuffer(bytes.fromhex(p["image_f32_le"]), dtype="<f4").reshape(1, 1, *p["shape"])
    assert LM.min_max_scaling(img).astype("<f4").tobytes().hex() == p["scaled_f32_le"]
    assert [int(v) for v in LM.preprocess(img).reshape(-1)] == p["fixed"]


@pytest.mark.parametrize("which", [0, 1])
def test_second_conv_pinned(which):
    case, inp = PINS["second_conv"][which], PINS["second_conv_input"]
    ct = [cipher_logs(m, r) for m, r in zip(inp["messages"], inp["r"])]
    keys = [bytes.fromhex(k) for k in case["keys"]]
    sums, res = LM.summed_conv(EM.LOGS, [c[0] for c in ct], [c[1] for c in ct], 6, 6, case["connect"], FILT, F, keys, PRF_BYTES)
    assert digest_points(flat(sums)) == case["sums"]
    assert digest_points(flat(res["out"])) == case["output"]
    assert_lists(case, res)
    assert len(res["mults"]) == 2 * case["n2"] * F * F and len(res["adds"]) == 2 * case["n2"] * (F * F - 1)  # no plane addition


def test_connection_table_read_off_the_run():
    small, full = PINS["second_conv"][0]["connect"], PINS["second_conv"][1]["connect"]
    assert full[:3] == small and len(full) == 16 and len({tuple(r) for r in full}) == 16
    assert sorted(sum(r) for r in full) == [3] * 6 + [4] * 9 + [6]
    assert LM.default_config()["connect"] == full


def test_third_conv_pinned():
    case = PINS["third_conv"]
    ct = [cipher_logs(m, r) for m, r in zip(case["messages"], case["r"])]
    keys = [hashlib.sha256(("layer_pins/key/inference_pins/third_conv/%d" % i).encode()).digest() for i in range(240)]
    assert hashlib.sha256(b"".join(keys)).hexdigest() == case["keys_sha256"]
    sums, res = LM.summed_conv(EM.LOGS, [c[0] for c in ct], [c[1] for c in ct], 5, 5, [[1] * 16] * 120, FILT, F, keys, PRF_BYTES)
    assert digest_points(flat(sums[:2])) == case["sums"]
    assert digest_points(flat(res["out"][0::2])) == case["output_c1"] and digest_points(flat(res["out"][1::2])) == case["output_c2"]
    assert_lists(case, res)


def test_first_conv_and_pool_pinned():
    case = PINS["first_conv"]
    c1, c2 = cipher_logs(case["messages"], case["r"])
    res = LM.first_conv(EM.LOGS, c1, c2, 6, 6, case["kernels"], FILT, F, [bytes.fromhex(k) for k in case["keys"]], PRF_BYTES)
    assert digest_points(flat(res["out"])) == case["output"]
    assert_lists(case, res)
    case = PINS["first_pool"]
    ct = [cipher_logs(m, r) for m, r in zip(case["messages"], case["r"])]
    res = LM.avg_pool(EM.LOGS, [c[0] for c in ct], [c[1] for c in ct], 4, 4, case["k"], case["stride"], POOL_SCALE)
    assert digest_points(flat(res["out"])) == case["output"]
    assert_lists(case, res)


# ---- the plaintext network on the reference's image and weights -----------------------------------------------------

@pytest.fixture(scope="module")
def plain():
    cfg = LM.default_config()
    image, w1, b1, w2, b2 = LM.reference_model()
    return cfg, (image, w1, b1, w2, b2), LM.plaintext(cfg, image, w1.tolist(), b1.tolist(), w2.tolist(), b2.tolist())


def test_reference_weights_are_unsigned_u32(plain):
    _, (image, w1, b1, w2, b2), _ = plain
    assert w1.min() >= 0 and w2.min() >= 0 and max(int(w1.max()), int(w2.max())) == 11016
    assert image.shape == (32, 32) and 0 < image.min() and image.max() < 65536


def test_plaintext_magnitudes_per_round(plain):
    _, _, (vs, acts) = plain
    got = [round(math.log2(max(abs(v) for v in r)), 1) for r in vs]
    assert got == MAGNITUDES, got
    assert 2**35 < max(abs(v) for v in vs[5]) < 2**39 and 2**35 < max(abs(v) for v in vs[6]) < 2**39
    assert len(acts[6]) == 10 and acts[6] == [max(v, 0) for v in vs[6]]


def test_default_counts(plain):
    cfg, _, (vs, _) = plain
    c = LM.counts(cfg)
    assert (c["encryptions"], c["decryptions"], c["prf_keys"], c["bias_r"]) == (9108, 8094, 288, 94)
    assert [len(v) for v in vs] == c["per_round"]
    assert [(VG.CONFIGS[label]["n_mult"], VG.CONFIGS[label]["n_add"]) for label in VG.LENET] == c["labels"]
