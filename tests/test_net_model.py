"""The layer-list model (tests/net_model.py) against recorded runs of the reference's CNN service (tests/golden/net_pins.json,
written by tests/golden/make_net_pins.py), its counts against the BASELINE configurations A and E, and the magnitudes of every
round of A and E on the reference's image and weights against the discrete-log ranges vpin_amd.net.cnn_config sets.  No GPU."""
import math

import pytest

import enc_conv_model as EM
import lenet_model as LM
import net_model as NM


@pytest.fixture(scope="module")
def pins():
    return NM.pins()


def run_case(p, case):
    """one pinned case through the model on discrete logarithms -> (rounds, layers, label)"""
    sk = int(p["sk"], 16)
    cfg = NM.pinned_config(case, p)
    c1, c2 = NM.log_encrypt(sk, [v for row in case["image"] for v in row], [int(r, 16) for r in case["image_r"]])
    bias_r = [int(r, 16) for r in case["bias_r"]]
    biases, pos = [], 0
    for l in cfg["layers"]:
        if l["kind"] == "fc":
            biases.append(NM.log_encrypt(sk, l["bias"], bias_r[pos:pos + l["N"]]))
            pos += l["N"]
    assert pos == len(bias_r)
    rounds = []
    client = NM.log_client(sk, [int(r, 16) for r in case["client_r"]], rounds)
    layers, label = NM.infer_model(EM.LOGS, cfg, c1, c2, [bytes.fromhex(k) for k in case["keys"]], biases, client)
    assert not client.left, "the model drew less client randomness than the reference"
    return cfg, rounds, layers, label


@pytest.mark.parametrize("index", [0, 1])
def test_model_reproduces_the_pinned_runs(pins, index):
    """rounds, result and all four lists of the reference's run, exactly; the points through one batched conversion of the logs"""
    case = pins["cases"][index]
    cfg, rounds, layers, label = run_case(pins, case)
    assert [(v, a) for v, a in rounds] == [(r["v"], r["act"]) for r in case["rounds"]]
    logs = [m[1] for m in label["mults"]] + [a[0] for a in label["adds"]] + [a[1] for a in label["adds"]] + label["result"][0] + label["result"][1]
    pts = LM.logs_to_points(logs)
    want = lambda ids: [None if i is None else tuple(int(c, 16) for c in pins["points"][i]) for i in ids]
    nm, na = len(label["mults"]), len(label["adds"])
    assert [str(m[0]) for m in label["mults"]] == case["mult_weights"]
    assert pts[:nm] == want(case["mult_points"])
    assert pts[nm:nm + na] == want(case["add_p"])
    assert pts[nm + na:nm + 2 * na] == want(case["add_r"])
    n = len(case["result"][0])
    assert pts[nm + 2 * na:nm + 2 * na + n] == want(case["result"][0]) and pts[nm + 2 * na + n:] == want(case["result"][1])
    c = NM.counts(cfg)
    assert (c["n_mult"], c["n_add"]) == (nm, na) and c["layers"] == [(len(r.get("mults", [])), len(r["adds"])) for r in layers]
    assert c["prf_keys"] == len(case["keys"]) and c["bias_r"] == len(case["bias_r"])
    assert c["encryptions"] == len(case["image_r"]) + len(case["client_r"]) and c["per_round"] == [len(r["v"]) for r in case["rounds"]]


def test_the_recorded_constants_are_the_issues(pins):
    net = pins["network"]
    assert net["conv"] == dict(fh=3, fw=3, pad=1, stride=1, filter=[1, 0, 1, 2, 0, 2, 1, 0, 1]) and net["prf_bytes"] == 14
    assert [pins["networks"][v]["pool"] for v in NM.VERSIONS] == [[4, 4], [4, 4], [2, 2], [2, 2], [2, 2]]
    assert pins["rounds"] == [dict(relu=1, shift_bits=0), dict(relu=0, shift_bits=26), dict(relu=1, shift_bits=32), dict(relu=1, shift_bits=0)]
    assert [c["pool_scale"] for c in pins["cases"]] == [64, 256]


def test_counts_are_the_baseline_configurations():
    from vpin_amd import gadgets as G
    a, e = NM.counts(NM.cnn_config("A")), NM.counts(NM.cnn_config("E"))
    assert (a["n_mult"], a["n_add"]) == (178, 2144) == (18 + 2 * (64 + 16), 16 + 1920 + 158 + 50)
    assert (e["n_mult"], e["n_add"]) == (658, 2336) == (18 + 2 * (256 + 64), 16 + 1536 + 638 + 146)
    assert (a["n_mult"], a["n_add"]) == (G.CONFIGS["A"]["n_mult"], G.CONFIGS["A"]["n_add"])
    assert (e["n_mult"], e["n_add"]) == (G.CONFIGS["E"]["n_mult"], G.CONFIGS["E"]["n_add"])
    assert a["layers"] == [(18, 16), (0, 1920), (128, 158), (32, 50)] and (a["prf_keys"], a["bias_r"]) == (6, 26)
    assert a["per_round"] == [1024, 64, 16, 10] and a["encryptions"] == 1024 + 1024 + 64 + 16


@pytest.mark.parametrize("version,k,K,N1", [("B", 4, 64, 32), ("C", 2, 256, 16), ("D", 2, 256, 32)])
def test_counts_follow_the_formula(version, k, K, N1):
    c = NM.counts(NM.cnn_config(version))
    side = 32 // k
    assert K == side * side
    assert c["n_mult"] == 18 + 2 * (K + N1)
    assert c["n_add"] == 16 + 2 * side * side * (k * k - 1) + 2 * (N1 + K - 1) + 2 * (10 + N1 - 1)


def test_rejected_configurations():
    cfg = NM.cnn_config("A")
    for spoil in (lambda c: c.update(H=0), lambda c: c["layers"][1].update(k=33), lambda c: c["layers"][2].update(w=c["layers"][2]["w"][:-1]),
                  lambda c: c["layers"][0].update(fh=35)):
        bad = dict(cfg, layers=[dict(l) for l in cfg["layers"]])
        spoil(bad)
        with pytest.raises(ValueError):
            NM.counts(bad)


# largest |v| per round on the reference's image and weights, as the plaintext model computes them (DESIGN section 11 lists them)
MAGNITUDES = {"A": [520939, 446694784, 9951206259, 7095278023], "E": [520939, 521598976, 34379353992, 96970086310]}


@pytest.mark.parametrize("version", ["A", "E"])
def test_round_magnitudes_lie_inside_the_configured_ranges(version):
    from vpin_amd import net as VN
    vs, acts = NM.plaintext(NM.cnn_config(version), NM.reference_image())
    mags = [max(abs(v) for v in r) for r in vs]
    print(version, "largest |v| per round:", mags, ["2^%.1f" % math.log2(m) for m in mags])
    assert mags == MAGNITUDES[version]
    giants = VN.cnn_config(version, nb_log=24).max_giants()
    assert len(giants) == 4 and all(m < g << 24 for m, g in zip(mags, giants))
    assert all(0 <= a < 2**31 for r in acts[:-1] for a in r), "what the client encrypts again fits int32"
