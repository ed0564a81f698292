"""The Python models of the encrypted layers and of the ElGamal client pinned to RUNS of the reference's own Python.

tests/golden/layer_pins.json is what the reference's functions (src/LeNet/Server.py, src/cnn_networks/Server.py,
src/convolution/Server.py, src/LeNet/Client.py, src/Pre_computed_table/baby-step-giant-step.py) computed when
tests/golden/make_layer_pins.py called them in the build container on small inputs: ciphertexts, layer outputs, the four global
lists handed to the prover, the left side of every RLC check, PRF outputs, the pooling scale, decrypted integers.  Nobody
restated a line of the reference to produce it.

Checked here against it, without a GPU and in POINTS mode: enc_conv_model.layer, enc_fc_model.fc / avgpool and
elgamal_model.keygen / encrypt / decrypt / bsgs -- outputs, multiplication list (weights and operands), addition list
(accumulators and operands, the identity where the reference added the identity) and left sides, exactly and in the
reference's order; the fixture's own consistency; and, where the reference tree is present, that the generator reproduces the
committed file byte for byte.  The kernels are checked against the same file in tests/test_gpu_layer_pins.py.

The product deliberately rejects a few inputs the reference computes through (an identity accumulator, an identity B'[k] /
X[k] / C[j]: VPIN_ESHAPE); the fixture's inputs avoid them, and the rejections have their own tests."""
import json
import os
import subprocess
import sys

import pytest

import elgamal_model as LM
import enc_conv_model as EM
import enc_fc_model as FM
import gadgets_model as GM

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "layer_pins.json")
GENERATOR = os.path.join(HERE, "golden", "make_layer_pins.py")
with open(FIXTURE) as f:
    PINS = json.load(f)

CONV_NAMES = ["conv_lenet_7x6", "conv_service_5x4", "conv_service_6x5_stride2"]
FC_NAMES = ["fc_lenet_5x3", "fc_lenet_70x4", "fc_cnn_networks_5x3"]
POOL_NAMES = ["pool_lenet_6x6"]
M_BABY = 3_200_000


def assert_counts():
    """an emptied or truncated fixture fails every test"""
    assert [c["name"] for c in PINS["conv"]] == CONV_NAMES
    assert [c["name"] for c in PINS["fc"]] == FC_NAMES
    assert [c["name"] for c in PINS["pool"]] == POOL_NAMES
    assert [(p["service"], len(p["t"]), len(p["values"])) for p in PINS["prf"]] == \
        [("LeNet", 8, 8), ("cnn_networks", 8, 8), ("convolution", 8, 8)]
    cl = PINS["client"]
    assert len(cl["encrypt"]) == 6 and len(cl["decrypt"]["results"]) == 9 and len(cl["table_script"]) == 6
    assert sum(len(r) for r in PINS["chained"]["values"]) == 20
    assert len(PINS["reference_sha256"]) == 5 and PINS["multi_core_feature"] == 0
    assert len(PINS["points"]) >= 1000


def case(kind, name):
    assert_counts()
    return next(c for c in PINS[kind] if c["name"] == name)


def pt(i):
    """a fixture point index -> (x, y) ints, None for the identity"""
    return None if i is None else (int(PINS["points"][i][0], 16), int(PINS["points"][i][1], 16))


def pts(idx):
    return [pt(i) for i in idx]


def lists_of(c):
    """the reference's four lists as the models return them: mults [(w, point)], adds [(acc, operand)]"""
    assert len(c["mult_weights"]) == len(c["mult_points"]) and len(c["add_p"]) == len(c["add_r"])
    return ([(int(w), pt(i)) for w, i in zip(c["mult_weights"], c["mult_points"])],
            [(pt(p), pt(r)) for p, r in zip(c["add_p"], c["add_r"])])


def keys_of(c):
    return [bytes.fromhex(k) for k in c["keys"]]


# ---- the fixture itself ---------------------------------------------------------------------------------------------

def test_curve_and_every_point():
    assert_counts()
    cv = {k: int(v, 16) for k, v in PINS["curve"].items()}
    assert (cv["q"], cv["a"], cv["gx"], cv["gy"], cv["order"]) == (GM.Q, GM.E2_A, GM.E2_GX, GM.E2_GY, GM.E2_ORDER)
    seen = set()
    for x, y in map(tuple, (pt(i) for i in range(len(PINS["points"])))):
        assert 0 <= x < cv["q"] and 0 <= y < cv["q"]
        assert (y * y - (x * x * x + cv["a"] * x + cv["b"])) % cv["q"] == 0, "a recorded point is not on E2"
        seen.add((x, y))
    assert len(seen) == len(PINS["points"]), "the point table holds each point once"
    assert (cv["gy"] ** 2 - (cv["gx"] ** 3 + cv["a"] * cv["gx"] + cv["b"])) % cv["q"] == 0


def weighted_sum(terms):
    acc = None
    for w, P in terms:
        acc = GM.e2_add(acc, EM.POINTS.mul(w, P))
    return acc


@pytest.mark.parametrize("kind,name", [("conv", n) for n in CONV_NAMES] + [("fc", n) for n in FC_NAMES])
def test_recorded_left_side_is_the_sum_the_right_side_lists_imply(kind, name):
    """per plane / row: sum_k weight_k * operand_k of the multiplication list equals result_left, and the addition list's
    last accumulator plus its last operand does too"""
    c = case(kind, name)
    mults, adds = lists_of(c)
    P = len(c["left"])
    per = len(mults) // P
    per_add = len(adds) // P
    assert per * P == len(mults) and per_add * P == len(adds)
    for p in range(P):
        left = pt(c["left"][p])
        assert left is not None
        assert weighted_sum(mults[p * per:(p + 1) * per]) == left
        acc, last = adds[(p + 1) * per_add - 1]
        assert GM.e2_add(acc, last) == left


# ---- the PRF --------------------------------------------------------------------------------------------------------

def test_prf():
    assert_counts()
    assert [p["prf_bytes"] for p in PINS["prf"]] == [13, 14, 16]
    for p in PINS["prf"]:
        key = bytes.fromhex(p["key"])
        assert [EM.prf(key, t, p["prf_bytes"]) for t in p["t"]] == [int(v) for v in p["values"]], p["service"]
        assert max(p["t"]) >= 1000 and 10 in p["t"]  # counters of more than one decimal digit


# ---- the layers -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_model(name):
    c = case("conv", name)
    mults, adds = lists_of(c)
    planes = [pts(p) for p in c["input"]]
    assert len(planes) == len(c["planes"]) == len(c["keys"]) and all(len(p) == c["H"] * c["W"] for p in planes)
    got = EM.layer(EM.POINTS, planes, c["H"], c["W"], c["filter"], c["fh"], c["fw"], c["pad"], c["stride"], keys_of(c),
                   c["prf_bytes"])
    assert EM.out_dims(c["H"], c["W"], c["fh"], c["fw"], c["pad"], c["stride"]) == (c["oh"], c["ow"])
    assert got["out"] == [pts(o) for o in c["output"]], "output ciphertext"
    assert [m[0] for m in got["mults"]] == [m[0] for m in mults], "multiplication weights"
    assert [m[1] for m in got["mults"]] == [m[1] for m in mults], "multiplication operands B'[k]"
    assert [a[0] for a in got["adds"]] == [a[0] for a in adds], "addition accumulators"
    assert [a[1] for a in got["adds"]] == [a[1] for a in adds], "addition operands (None where the reference added the identity)"
    assert got["left"] == pts(c["left"]), "left sides"
    assert sum(a[1] is None for a in adds) == len(c["planes"]) * sum(w == 0 for w in c["filter"][1:])


@pytest.mark.parametrize("name", FC_NAMES)
def test_fc_model(name):
    c = case("fc", name)
    mults, adds = lists_of(c)
    rows, biases = [pts(r) for r in c["input"]], [pts(b) for b in c["bias_points"]]
    got = FM.fc(FM.POINTS, rows, c["K"], c["weights"], c["N"], biases, keys_of(c), c["prf_bytes"])
    assert got["out"] == [pts(o) for o in c["output"]], "output ciphertext"
    assert [m[0] for m in got["mults"]] == [m[0] for m in mults], "folded weights"
    assert [m[1] for m in got["mults"]] == [m[1] for m in mults], "multiplication operands X[k]"
    assert got["adds"] == adds, "the N bias additions, then the K - 1 additions of the check, per row"
    assert got["left"] == pts(c["left"]), "left sides"
    assert len(adds) == 2 * (c["N"] + c["K"] - 1) and any(0 in w for w in c["weights"]) and max(max(w) for w in c["weights"]) == 11016


@pytest.mark.parametrize("name", POOL_NAMES)
def test_pool_model(name):
    c = case("pool", name)
    assert c["scale"] == 256 == int((1 / c["k"] ** 2) * 2 ** 10)
    adds = [(pt(p), pt(r)) for p, r in zip(c["add_p"], c["add_r"])]
    got = FM.avgpool(FM.POINTS, [pts(p) for p in c["input"]], c["H"], c["W"], c["k"], c["stride"], c["scale"])
    assert FM.pool_dims(c["H"], c["W"], c["k"], c["stride"]) == (c["oh"], c["ow"])
    assert got["out"] == [pts(o) for o in c["output"]], "output ciphertext"
    assert got["adds"] == adds and len(adds) == 2 * c["oh"] * c["ow"] * (c["k"] ** 2 - 1)


# ---- the client -----------------------------------------------------------------------------------------------------

def model_table(js):
    """the model's baby-step table over the baby steps the fixture names (a subset of the full table answers alike: the first
    hit of the two walks is unique)"""
    assert js[0] == 0
    return {LM.mul(j): j for j in js}


def test_client_model_keygen_and_encrypt():
    assert_counts()
    cl = PINS["client"]
    sk, H = int(cl["sk"], 16), pt(cl["h"])
    assert LM.keygen(sk) == H
    assert [e["msg"] for e in cl["encrypt"]] == [0, 1, -1, 65535, -65536, 2**20 + 3]
    for e in cl["encrypt"]:
        assert LM.encrypt(H, e["msg"], int(e["r"], 16)) == (pt(e["c1"]), pt(e["c2"])), e["msg"]


def test_client_model_decrypt_and_bsgs():
    assert_counts()
    cl = PINS["client"]
    d, sk, m = cl["decrypt"], int(cl["sk"], 16), cl["m"]
    assert m == M_BABY
    assert d["values"] == [0, 1, -1, m - 1, m, -m, 3 * m + 17, -(2 * m + 5), 5 * m + m - 1] == d["results"]
    table = model_table(d["table_js"])
    assert None in table and table[None] == 0
    got = [LM.decrypt(table, m, sk, pt(a), pt(b), 6) for a, b in zip(d["c1"], d["c2"])]
    assert got == d["results"]
    got = [LM.decrypt(table, m, sk, pt(a), pt(b), 4) for a, b in zip(d["c1"], d["c2"])]
    assert got == d["results"][:8] + [None]
    for e in cl["table_script"]:  # the table script's own giant step
        assert LM.bsgs(table, m, pt(e["point"]), 6) == e["result"]
    assert [e["result"] for e in cl["table_script"]] == [v for v in d["values"] if v >= 0]


def test_chained_conv_output_decrypts_to_the_recorded_integers():
    """the reference's convolution output, decrypted by the model, equals what the reference's client decrypted -- which the
    generator compared with numpy's plain convolution of the plaintext image"""
    assert_counts()
    ch = PINS["chained"]
    c = case("conv", ch["conv"])
    sk = int(PINS["client"]["sk"], 16)
    table = model_table(ch["table_js"])
    want = [v for row in ch["values"] for v in row]
    assert (len(ch["values"]), len(ch["values"][0])) == (c["oh"], c["ow"]) and min(want) < 0 < max(want)
    got = [LM.decrypt(table, M_BABY, sk, pt(a), pt(b), 0) for a, b in zip(c["output"][0], c["output"][1])]
    assert got == want


# ---- the generator reproduces the committed file --------------------------------------------------------------------

def reference_root():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_layer_pins", GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.REF, gen.FILES


def test_generator_reproduces_the_fixture(tmp_path):
    assert_counts()
    root, files = reference_root()
    if not all(os.path.exists(os.path.join(root, rel)) for rel in files.values()):
        pytest.skip("the reference tree is not on this machine")
    out = tmp_path / "layer_pins.json"
    subprocess.run([sys.executable, GENERATOR, "--out", str(out)], check=True, capture_output=True, timeout=600)
    with open(FIXTURE, "rb") as f:
        assert out.read_bytes() == f.read(), "tests/golden/make_layer_pins.py no longer reproduces tests/golden/layer_pins.json"
