"""GPU tests of the layer-list inference (vpin_net_infer, vpin_net_client_*, vpin_amd.net): the two 8 x 8 runs of the reference's
CNN service recorded in tests/golden/net_pins.json with the pinned keys and r (every round's values, the result and the one
label's four lists byte for byte), the same through a Python callback, a network with a layer that has no round, the label
through the witness files and the CLI, the rejections, and the networks A and E at full size on the reference's image and
weights against the plaintext model (tests/net_model.py)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import elgamal_model as EL
import enc_conv_model as EM
import lenet_model as LM
import net_model as NM
from test_gpu_enc_conv import points_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vpin_amd", "bin", "vpin_prove")
NB = 1 << 16
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))
SK_FULL = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER
E_KEY_START = 0  # keys sha256("net/key/<i>"), i = E_KEY_START ..: net_model says every folded weight of E fits under these


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pins():
    return NM.pins()


def device_config(cfg, giants):
    """a net_model configuration as a vpin_amd.net.Config"""
    from vpin_amd import net as VN
    out = VN.Config(cfg["C"], cfg["H"], cfg["W"], cfg["prf_bytes"])
    giants = list(giants)
    for l in cfg["layers"]:
        if l["kind"] == "conv":
            out.conv([l["filter"][i * l["fw"]:(i + 1) * l["fw"]] for i in range(l["fh"])], l["pad"], l["stride"])
        elif l["kind"] == "pool":
            out.pool(l["k"], l["stride"], l["scale"])
        else:
            out.fc(l["w"], l["bias"])
        if l.get("round"):
            r = l["round"]
            out.round(r["relu"], r["shift_bits"], giants.pop(0), r["reencrypt"])
    return out


def pin_points(pins, ids):
    return [None if i is None else tuple(int(c, 16) for c in pins["points"][i]) for i in ids]


class PinnedRun:
    def __init__(self, ctx, pins, case):
        from vpin_amd import net as VN
        self.case, self.sk = case, int(pins["sk"], 16)
        self.model = NM.pinned_config(case, pins)
        # the range of every round from the pin's own magnitudes: a table of 2^16 baby steps
        self.giants = [max(abs(v) for v in r["v"]) // NB + 1 for r in case["rounds"]]
        self.cfg = device_config(self.model, self.giants)
        self.keys = [bytes.fromhex(k) for k in case["keys"]]
        self.bias_r = [int(r, 16) for r in case["bias_r"]]
        self.client_r = [int(r, 16) for r in case["client_r"]]
        self.image = [v for row in case["image"] for v in row]
        self.image_r = [int(r, 16) for r in case["image_r"]]
        self.client = VN.Client(ctx, self.sk, NB, self.giants, self.client_r)
        self.scores, self.rounds, self.trace = VN.infer(ctx, self.cfg, self.client, self.image, self.image_r, self.keys, self.bias_r)

    def free(self):
        self.trace.free()
        self.client.free()


@pytest.fixture(scope="module")
def runs(ctx, pins):
    out = [PinnedRun(ctx, pins, case) for case in pins["cases"]]
    yield out
    for r in out:
        r.free()


@pytest.mark.parametrize("index", [0, 1])
def test_pinned_runs_of_the_reference(ctx, pins, runs, index):
    run = runs[index]
    case, trace = run.case, run.trace
    c1, c2 = run.client.encrypt(np.array(run.image, dtype=np.int64), run.image_r)
    assert points_of(*c1) == pin_points(pins, case["input"][0]) and points_of(*c2) == pin_points(pins, case["input"][1])
    assert len(run.rounds) == len(case["rounds"]) == 4
    for i, (got, want) in enumerate(zip(run.rounds, case["rounds"])):
        assert [int(a) for a in got[0]] == want["v"], "round %d v" % i
        assert [int(a) for a in got[1]] == want["act"], "round %d act" % i
    assert [int(a) for a in run.scores] == case["rounds"][-1]["act"]
    r1, r2 = trace.result()
    assert points_of(*r1) == pin_points(pins, case["result"][0]) and points_of(*r2) == pin_points(pins, case["result"][1])
    label = trace.label()
    w, mx, my = label.mults()
    px, py, rx, ry, rz = label.adds()
    assert [str(v) for v in w] == case["mult_weights"]
    assert points_of(mx, my) == pin_points(pins, case["mult_points"])
    assert points_of(px, py) == pin_points(pins, case["add_p"])
    assert points_of(rx, ry, rz) == pin_points(pins, case["add_r"])
    counts = run.cfg.counts()
    assert counts == dict(NM.counts(run.model), rounds=4) and (label.n_mult, label.n_add) == (counts["n_mult"], counts["n_add"])
    # the per-layer views concatenate to the label
    assert trace.n_layers == 4
    layers = [trace.layer(i) for i in range(4)]
    assert [(t.n_mult, t.n_add) for t in layers] == counts["layers"]
    assert sum((t.mults()[0] for t in layers), []) == w
    for j, whole in enumerate((mx, my)):
        assert np.array_equal(np.concatenate([t.mults()[1 + j] for t in layers]), whole)
    for j, whole in enumerate((px, py, rx, ry, rz)):
        assert np.array_equal(np.concatenate([t.adds()[j] for t in layers]), whole)
    for u, v in zip(layers[3].output(), label.output()):
        assert np.array_equal(u, v)


def test_python_callback_gives_the_same_trace(ctx, runs):
    """the interaction as a Python callback: decrypt, activate with the model, encrypt -- three separate entry points"""
    from vpin_amd import elgamal as E
    from vpin_amd import net as VN
    run = runs[0]
    table = E.DlogTable(ctx, NB)
    queue, seen = list(run.client_r), []

    def fn(rnd, relu, reencrypt, bits, c1, c2):
        v, found = ctx.e2_decrypt(table.h, run.sk, c1, c2, run.giants[rnd])
        assert found.all()
        act = [LM.activate(int(a), relu, bits) for a in v]
        seen.append(act)
        if not reencrypt:
            return None
        return ctx.e2_encrypt(run.client.base_g, run.client.base_h, act, [queue.pop(0) for _ in act])

    c1, c2 = run.client.encrypt(np.array(run.image, dtype=np.int64), run.image_r)
    other = VN.run(ctx, run.cfg, c1, c2, run.client.base_g, run.client.base_h, run.keys, run.bias_r, VN.python_round(fn))
    tm = VN.timings(4)  # the layout: the whole, then per layer the layer and the round after it
    assert len(tm["layers"]) == len(tm["rounds"]) == 4 and all(t > 0 for t in tm["layers"] + tm["rounds"]), tm
    assert tm["total"] >= sum(tm["layers"]) + sum(tm["rounds"]), tm
    assert seen == [r["act"] for r in run.case["rounds"]] and not queue
    a, b = run.trace.label(), other.label()
    assert a.mults()[0] == b.mults()[0]
    for u, v in zip(list(a.output()) + list(a.adds()) + list(a.mults()[1:]), list(b.output()) + list(b.adds()) + list(b.mults()[1:])):
        assert np.array_equal(u, v)
    other.free()
    table.free()


# a small network whose convolution has no round: its ciphertext goes straight into the pooling
SMALL = dict(C=2, H=6, W=5, prf_bytes=13, layers=[
    dict(kind="conv", fh=2, fw=2, pad=0, stride=1, filter=[1, 2, 3, 1]),
    dict(kind="pool", k=2, stride=2, scale=3, round=dict(relu=1, shift_bits=0, reencrypt=True)),
    dict(kind="fc", N=2, w=[[1, 2], [3, 0], [0, 1], [2, 2], [5, 1], [0, 4], [1, 1], [2, 0]], bias=[-5, 40], round=dict(relu=0, shift_bits=0, reencrypt=False))])
SMALL_IMAGE = [[(5 * i * i + 3 * j + c * (i + 2 * j)) % 13 - 6 for j in range(5)] for c in range(2) for i in range(6)]
SMALL_SK = 0xABCDEF0123456789 % EL.ORDER


@pytest.fixture(scope="module")
def small(ctx):
    from vpin_amd import net as VN
    counts = NM.counts(SMALL)
    assert counts["layers"] == [(16, 12), (0, 48), (16, 18)] and counts["prf_keys"] == 6 and counts["per_round"] == [8, 2]
    msgs = [v for row in SMALL_IMAGE for v in row]
    vs, acts = NM.plaintext(SMALL, np.array(SMALL_IMAGE).reshape(2, 6, 5))
    assert any(v < 0 for v in vs[0]) and max(abs(v) for r in vs for v in r) < NB * 4
    image_r, bias_r, client_r = EL.splitmix_scalars(0x5A1, 60), EL.splitmix_scalars(0x5A2, 2), EL.splitmix_scalars(0x5A3, 8)
    keys = [NM.net_key(100 + i) for i in range(6)]
    cfg = device_config(SMALL, [4, 4])
    client = VN.Client(ctx, SMALL_SK, NB, [4, 4], client_r)
    scores, rounds, trace = VN.infer(ctx, cfg, client, msgs, image_r, keys, bias_r)
    timings = VN.timings(3)
    # the model on discrete logarithms
    c1, c2 = NM.log_encrypt(SMALL_SK, msgs, image_r)
    seen = []
    layers, label = NM.infer_model(EM.LOGS, SMALL, c1, c2, keys, [NM.log_encrypt(SMALL_SK, SMALL["layers"][2]["bias"], bias_r)],
                                   NM.log_client(SMALL_SK, client_r, seen))
    yield dict(cfg=cfg, client=client, trace=trace, rounds=rounds, scores=scores, plain=(vs, acts), layers=layers, label=label, seen=seen,
               msgs=msgs, image_r=image_r, bias_r=bias_r, keys=keys, timings=timings)
    trace.free()
    client.free()


def test_layer_without_a_round_hands_its_ciphertext_on(small):
    vs, acts = small["plain"]
    assert [([int(a) for a in v], [int(a) for a in act]) for v, act in small["rounds"]] == list(zip(vs, acts)) == [tuple(s) for s in small["seen"]]
    trace, conv = small["trace"], LM.logs_to_points
    assert trace.n_layers == 3
    tm = small["timings"]  # of the fixture's run: the convolution's round slot stays exactly 0
    assert all(t > 0 for t in tm["layers"]) and tm["rounds"][0] == 0 and tm["rounds"][1] > 0 and tm["rounds"][2] > 0, tm
    assert tm["total"] >= sum(tm["layers"]) + sum(tm["rounds"]), tm
    for i, exp in enumerate(small["layers"]):
        t = trace.layer(i)
        assert points_of(*t.output()) == conv([v for plane in exp["out"] for v in plane]), "output of layer %d" % i
    label = trace.label()
    w, mx, my = label.mults()
    px, py, rx, ry, rz = label.adds()
    exp = small["label"]
    assert (label.n_mult, label.n_add) == (32, 78) and w == [m[0] for m in exp["mults"]]
    assert points_of(mx, my) == conv([m[1] for m in exp["mults"]])
    assert points_of(px, py) == conv([a[0] for a in exp["adds"]]) and points_of(rx, ry, rz) == conv([a[1] for a in exp["adds"]])


def test_label_through_witness_files_and_the_cli(ctx, small, tmp_path):
    from vpin_amd import net as VN
    trace = small["trace"]
    VN.write_witness_files(trace, str(tmp_path), "NET")
    assert all(len(os.listdir(tmp_path / "rust_files" / "NET" / d)) == n for d, n in (("pointAdd", 5), ("pointMult", 3)))
    os.makedirs(tmp_path / "out")
    master = bytes(range(64)) + bytes((7 * i + 3) % 256 for i in range(64))  # 128 bytes: SHAKE256(master || domain) per proof
    r = subprocess.run([BIN, "NET", "--seed", master.hex(), "--write-proof", "out"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    gm, ga = trace.instances()
    for g, kind, dom in ((ga, "add", b"vPIN/point_add"), (gm, "mult", b"vPIN/point_mult")):
        assert g.is_sat()
        seed = hashlib.shake_256(master + dom).digest(128)
        got = g.snark_prove(seed[:64], seed[64:])
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        assert open(tmp_path / "out" / ("NET_%s.proof" % kind), "rb").read() == got["proof"], kind
        g.free()


def test_rejections(ctx, small):
    import vpin_amd
    from vpin_amd import net as VN
    client, cfg, keys, bias_r = small["client"], small["cfg"], small["keys"], small["bias_r"]
    c1, c2 = client.encrypt(np.array(small["msgs"], dtype=np.int64), small["image_r"])

    def fails(code, match, keys=keys, bias_r=bias_r, user=None, config=cfg):
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            VN.run(ctx, config, c1, c2, client.base_g, client.base_h, keys, bias_r, client.round_fn, user or client.user).free()
        assert e.value.code == code

    fails(-1, "number of PRF keys", keys=keys[:-1])
    fails(-1, "bias randomness", bias_r=bias_r[:-1])
    neg = dict(SMALL, layers=[dict(l) for l in SMALL["layers"]])
    neg["layers"][2]["w"] = [[1, 2], [3, 0], [0, -1]] + SMALL["layers"][2]["w"][3:]
    fails(-1, "negative", config=device_config(neg, [4, 4]))
    short = dict(SMALL, layers=[dict(l) for l in SMALL["layers"]])
    short["layers"][2]["w"] = SMALL["layers"][2]["w"][:7]
    fails(-1, "K is not the C \\* H \\* W", config=device_config(short, [4, 4]))
    with pytest.raises(vpin_amd.VpinError, match="K is not") as e:
        device_config(short, [4, 4]).counts()
    assert e.value.code == -1
    # the client of the fixture has used up its queue: round 0 is the one that encrypts, the error names it, nothing is consumed
    fails(-1, "round 0: .*randomness r is used up")
    fails(-1, "round 0: .*randomness r is used up")
    # a fresh client one r short fails the same way and then serves a run that needs no more than it has
    one_short = VN.Client(ctx, SMALL_SK, NB, [4, 4], EL.splitmix_scalars(0x5A3, 7))
    fails(-1, "round 0: .*randomness r is used up", user=one_short.user)
    tiny = dict(C=1, H=2, W=2, prf_bytes=13, layers=[dict(kind="pool", k=2, stride=2, scale=1, round=dict(relu=0, shift_bits=0, reencrypt=True))])
    t1, t2 = one_short.encrypt(np.array([1, 2, 3, 4], dtype=np.int64), EL.splitmix_scalars(0x5A4, 4))
    tr = VN.run(ctx, device_config(tiny, [4, 4]), t1, t2, None, None, [], [], one_short.round_fn, one_short.user)
    assert [int(v) for v in one_short.values(0)[0]] == [10]
    tr.free()
    one_short.free()


def full_size(ctx, version, key_start, prove):
    from vpin_amd import net as VN
    model = NM.cnn_config(version)
    image = NM.reference_image()
    vs, acts = NM.plaintext(model, image)
    cfg = VN.cnn_config(version, nb_log=24)
    counts, giants = cfg.counts(), cfg.max_giants()
    assert counts == dict(NM.counts(model), rounds=4)
    assert all(max(abs(v) for v in r) < g << 24 for r, g in zip(vs, giants))
    keys = [NM.net_key(key_start + i) for i in range(counts["prf_keys"])]
    assert all(NM.keys_fit(model, keys)), "a folded weight would not fit 128 bits under these keys: move the start index"
    client = VN.Client(ctx, SK_FULL, 1 << 24, giants, EL.splitmix_scalars(0xCA3, counts["encryptions"] - 1024))
    scores, rounds, trace = VN.infer(ctx, cfg, client, image, EL.splitmix_scalars(0xCA1, 1024), keys, EL.splitmix_scalars(0xCA2, counts["bias_r"]))
    for r in range(4):
        assert [int(a) for a in rounds[r][0]] == vs[r] and [int(a) for a in rounds[r][1]] == acts[r], "round %d" % r
    assert [int(a) for a in scores] == acts[3]
    label = trace.label()
    if prove:
        gm, ga = trace.instances()
        for g in (gm, ga):
            got = g.snark_prove(SEED_C, SEED_P)
            assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
            g.free()
    dims = (label.n_mult, label.n_add)
    trace.free()
    client.free()
    return dims


def test_cnn_a_on_the_reference_image_and_weights(ctx):
    """network A at full size, a table of 2^24 baby steps: every round and the scores are the plaintext model's, the one label has
    the 178 multiplications and 2144 additions of the BASELINE configuration A, and its two instances are proven and verified"""
    assert full_size(ctx, "A", 0, prove=True) == (178, 2144)


def test_cnn_e_on_the_reference_image_and_weights(ctx):
    """network E at full size: 658 multiplications and 2336 additions.  Its FC1 (K = 256, N = 64, row sums of the weights up to
    2^16.7 under 14-byte PRF values) overflows 128 bits for some keys; the keys start at index E_KEY_START = 0, the first start at
    which net_model says all six fit (no move was needed).  Proving E's shape is test_gpu_configs.py's"""
    assert full_size(ctx, "E", E_KEY_START, prove=False) == (658, 2336)


def test_cnn_e_key_whose_folded_weight_overflows_is_refused(ctx):
    """the first key index at which an s_k of E's FC1 leaves 128 bits, as the c1 row's key: VPIN_ESHAPE naming that layer, no trace"""
    import vpin_amd
    from vpin_amd import net as VN
    model = NM.cnn_config("E")
    fc1 = model["layers"][2]
    bad = next((i for i in range(2000) if not NM.folded_fit(fc1["w"], fc1["N"], NM.net_key(i), model["prf_bytes"])), None)
    assert bad is not None, "no overflowing key among 2000"
    cfg = VN.cnn_config("E", nb_log=16)
    counts, giants = cfg.counts(), [1 << 22] * 4
    keys = [NM.net_key(E_KEY_START + i) for i in range(6)]
    keys[2] = NM.net_key(bad)
    client = VN.Client(ctx, SK_FULL, NB, giants, EL.splitmix_scalars(0xCA3, counts["encryptions"] - 1024))
    c1, c2 = client.encrypt(NM.reference_image().reshape(-1).astype(np.int64), EL.splitmix_scalars(0xCA1, 1024))
    with pytest.raises(vpin_amd.VpinError, match=r"vpin_net_infer: layer 2 \(fc\): .*does not fit 128 bits") as e:
        VN.run(ctx, cfg, c1, c2, client.base_g, client.base_h, keys, EL.splitmix_scalars(0xCA2, counts["bias_r"]), client.round_fn, client.user)
    assert e.value.code == -5
    client.free()
