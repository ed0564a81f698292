"""GPU tests of the whole encrypted LeNet inference (vpin_lenet_infer, vpin_net_client_*, vpin_amd.lenet) on the smallest
network the architecture allows: a 32 x 32 image of small signed integers, n1 = 2, n2 = 3 (rows [1,1], [0,1], [1,0]), n3 = 4,
FC 4 -> 3 -> 2, the LeNet filter, pool scale 1 and shifts chosen so that every decrypted value stays within 2^16 * 64 (a table
of 2^16 baby steps and 64 giant steps).  The scores and every round's values are compared with the plaintext model, every
label's lists with tests/lenet_model.py run on discrete logarithms, byte for byte."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import elgamal_model as EL
import enc_conv_model as EM
import lenet_model as LM
from test_gpu_enc_conv import points_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vpin_amd", "bin", "vpin_prove")
N = EL.ORDER
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % N
NB, GIANT = 1 << 16, 64
BOUND = NB * GIANT
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))

FULL = LM.default_config()
CFG = dict(H=32, W=32, n1=2, n2=3, n3=4, connect=[[1, 1], [0, 1], [1, 0]], f=FULL["f"], filter=FULL["filter"], pool_k=2, pool_stride=2,
           pool_scale=1, rounds=[(1, 0), (0, 14), (1, 0), (0, 18), (1, 20), (1, 19), (1, 0)], N1=3, N2=2)
IMAGE = [[(7 * i * i + 3 * j + i * j) % 17 - 8 for j in range(32)] for i in range(32)]
W1 = [[1, 0, 3], [2, 1, 0], [0, 3, 1], [1, 1, 2]]
B1 = [-70000, 5, 1234]
W2 = [[1, 2], [3, 0], [0, 1]]
B2 = [-9, 100000]
PRF = 13
COUNTS = LM.counts(CFG)
KEYS = [hashlib.sha256(b"lenet/key/%d" % i).digest() for i in range(COUNTS["prf_keys"])]
IMAGE_RS = EL.splitmix_scalars(0x1E1, 1024)
BIAS_RS = EL.splitmix_scalars(0x1E2, COUNTS["bias_r"])
CLIENT_RS = EL.splitmix_scalars(0x1E3, COUNTS["encryptions"] - 1024)


@pytest.fixture(scope="module")
def plain():
    """the plaintext run; the bound is asserted before anything goes to the GPU"""
    vs, acts = LM.plaintext(CFG, IMAGE, W1, B1, W2, B2)
    assert max(abs(v) for r in vs for v in r) < BOUND
    assert any(v < 0 for v in vs[0]) and any(v < 0 for v in vs[5] + vs[6]), "ReLU cuts something"
    assert [len(v) for v in vs] == COUNTS["per_round"]
    return vs, acts


@pytest.fixture(scope="module")
def model(plain):
    """the loop on discrete logarithms: pixel (m, r) is (r, m + r sk); the client answers with the plaintext run's values"""
    _, acts = plain
    enc = lambda ms, rs: ([r % N for r in rs], [(m + r * SK) % N for m, r in zip(ms, rs)])
    c1, c2 = enc([v for row in IMAGE for v in row], IMAGE_RS)
    queue = list(CLIENT_RS)

    def client(r, relu, bits, reencrypt, p1, p2):
        if not reencrypt:
            return None, None
        a1, a2 = enc(acts[r], [queue.pop(0) for _ in acts[r]])
        per = len(p1[0])
        cut = lambda a: [a[i:i + per] for i in range(0, len(a), per)]
        return cut(a1), cut(a2)

    b1, b2 = enc(B1, BIAS_RS[:3]), enc(B2, BIAS_RS[3:])
    labels = LM.infer_model(EM.LOGS, CFG, PRF, c1, c2, KEYS, W1, b1, W2, b2, client)
    assert not queue
    return labels


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def make_cfg():
    from vpin_amd import lenet as VL
    f = CFG["f"]
    cfg = VL.Config([CFG["filter"][i * f:(i + 1) * f] for i in range(f)], CFG["connect"], W1, B1, W2, B2)
    cfg.set_pool(2, 2, 1)
    cfg.set_rounds(relu=[r[0] for r in CFG["rounds"]], shift_bits=[r[1] for r in CFG["rounds"]], max_giant=[GIANT] * 7)
    return cfg


@pytest.fixture(scope="module")
def run(ctx):
    """one inference against the ready-made client, shared by the checks"""
    from vpin_amd import lenet as VL
    cfg = make_cfg()
    client = VL.Client(ctx, SK, NB, [GIANT] * 7, CLIENT_RS)
    scores, rounds, trace = VL.infer(ctx, cfg, client, IMAGE, IMAGE_RS, KEYS, BIAS_RS)
    yield cfg, client, scores, rounds, trace
    trace.free()
    client.free()


def test_scores_and_round_values_are_the_plaintext_model(run, plain):
    _, _, scores, rounds, _ = run
    vs, acts = plain
    for r in range(7):
        assert [int(a) for a in rounds[r][0]] == vs[r], "R%d v" % (r + 1)
        assert [int(a) for a in rounds[r][1]] == acts[r], "R%d act" % (r + 1)
    assert [int(a) for a in scores] == acts[6]


def test_label_counts(run):
    cfg, _, _, _, trace = run
    c = cfg.counts()
    assert c == dict(COUNTS, labels=[tuple(l) for l in COUNTS["labels"]])
    for i, name in enumerate(("L1", "L2", "L3", "L4", "L5", "L6", "L7")):
        t = trace.label(name)
        assert (t.n_mult, t.n_add) == tuple(c["labels"][i]), name


def assert_label(t, exp):
    conv = lambda logs: LM.logs_to_points(logs)
    ox, oy, oi = t.output()
    want = exp.get("rows", exp["out"])
    assert points_of(ox, oy, oi) == conv([v for pl in want for v in pl]), "output"
    if t.n_mult:
        w, mx, my = t.mults()
        assert w == [m[0] for m in exp["mults"]]
        assert points_of(mx, my) == conv([m[1] for m in exp["mults"]])
        lx, ly, li = t.left()
        assert points_of(lx, ly, li) == conv(exp["left"])
    px, py, rx, ry, rz = t.adds()
    assert points_of(px, py) == conv([a[0] for a in exp["adds"]])
    assert points_of(rx, ry, rz) == conv([a[1] for a in exp["adds"]])


@pytest.mark.parametrize("label", [1, 2, 3, 4, 5, 6, 7])
def test_label_lists_are_the_models(run, model, label):
    assert_label(run[4].label("L%d" % label), model[label - 1])


def test_numpy_callback_gives_the_same_trace_and_scores(ctx, run, plain):
    """the interaction as a Python callback: decrypt, activate with the model, encrypt -- three separate entry points"""
    from vpin_amd import elgamal as E
    from vpin_amd import lenet as VL
    cfg, client, scores, _, trace = run
    table = E.DlogTable(ctx, NB)
    queue, seen = list(CLIENT_RS), []

    def fn(rnd, relu, reencrypt, bits, c1, c2):
        v, found = ctx.e2_decrypt(table.h, SK, c1, c2, GIANT)
        assert found.all()
        act = [LM.activate(int(a), relu, bits) for a in v]
        seen.append(act)
        if not reencrypt:
            return None
        return ctx.e2_encrypt(client.base_g, client.base_h, act, [queue.pop(0) for _ in act])

    c1, c2 = client.encrypt(np.array(IMAGE, dtype=np.int64).reshape(-1), IMAGE_RS)
    cb = VL.python_round(fn)
    other = VL.run(ctx, cfg, c1, c2, client.base_g, client.base_h, KEYS, BIAS_RS, cb)
    tm = VL.timings()  # the layout: seven labels, seven rounds, the whole
    assert len(tm["labels"]) == len(tm["rounds"]) == 7 and all(t > 0 for t in tm["labels"] + tm["rounds"]), tm
    assert tm["total"] >= sum(tm["labels"]) + sum(tm["rounds"]), tm
    assert seen[6] == [int(a) for a in scores] and seen[6] == plain[1][6]
    for name in VL.LABELS:
        a, b = trace.label(name), other.label(name)
        for u, v in zip(list(a.output()) + list(a.adds()) + list(a.mults()[1:]), list(b.output()) + list(b.adds()) + list(b.mults()[1:])):
            assert np.array_equal(u, v), name
        assert a.mults()[0] == b.mults()[0]
    for u, v in zip(tuple(trace.result()[0]) + tuple(trace.result()[1]), tuple(other.result()[0]) + tuple(other.result()[1])):
        assert np.array_equal(u, v)
    other.free()
    table.free()


def test_every_label_is_satisfied_and_the_fc_labels_prove(ctx, run):
    _, _, _, _, trace = run
    for name in ("L1", "L2", "L3", "L4", "L5", "L6", "L7"):
        gm, ga = trace.instances(name)
        assert (gm is None) == (name in ("L2", "L4")) and ga is not None
        for g in (gm, ga):
            if g is None:
                continue
            assert g.is_sat(), name
            if name in ("L6", "L7"):
                got = g.snark_prove(SEED_C, SEED_P)
                assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
            g.free()


def test_witness_files_and_the_cli_give_the_device_path_proofs(ctx, run, tmp_path):
    from vpin_amd import lenet as VL
    _, _, _, _, trace = run
    VL.write_witness_files(trace, str(tmp_path))
    assert sorted(os.listdir(tmp_path / "rust_files")) == list(VL.LABELS)
    assert all(len(os.listdir(tmp_path / "rust_files" / l / d)) == n for l in VL.LABELS for d, n in (("pointAdd", 5), ("pointMult", 3)))
    os.makedirs(tmp_path / "out")
    master = bytes(range(64)) + bytes((7 * i + 3) % 256 for i in range(64))  # 128 bytes: SHAKE256(master || domain) per proof
    r = subprocess.run([BIN, "L7", "--seed", master.hex(), "--write-proof", "out"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    gm, ga = trace.instances("L7")
    for g, kind, dom in ((ga, "add", b"vPIN/point_add"), (gm, "mult", b"vPIN/point_mult")):
        seed = hashlib.shake_256(master + dom).digest(128)
        got = g.snark_prove(seed[:64], seed[64:])
        assert open(tmp_path / "out" / ("L7_%s.proof" % kind), "rb").read() == got["proof"], kind
        g.free()


def test_tampering_fails_with_the_code_and_the_label(ctx, run):
    import vpin_amd
    from vpin_amd import lenet as VL
    cfg, client, _, _, _ = run
    c1, c2 = client.encrypt(np.array(IMAGE, dtype=np.int64).reshape(-1), IMAGE_RS)

    def fails(code, match, keys=KEYS, bias_rs=BIAS_RS, fn=None, user=None, config=cfg):
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            VL.run(ctx, config, c1, c2, client.base_g, client.base_h, keys, bias_rs, fn or client.round_fn, user).free()
        assert e.value.code == code

    fails(-1, "number of PRF keys", keys=KEYS[:-1], user=client.user)
    fails(-1, "bias randomness", bias_rs=BIAS_RS[:-1], user=client.user)
    # a queue of r one short: the last encrypting round, R6, runs dry
    short = VL.Client(ctx, SK, NB, [GIANT] * 7, CLIENT_RS[:-1])
    fails(-1, "R6: .*randomness r is used up", user=short.user)
    short.free()
    # a callback that answers R2 with an off-curve point: L3 takes that answer and rejects it
    from vpin_amd import elgamal as E
    table = E.DlogTable(ctx, NB)
    queue = list(CLIENT_RS)

    def fn(rnd, relu, reencrypt, bits, a, b):
        v, _ = ctx.e2_decrypt(table.h, SK, a, b, GIANT)
        act = [LM.activate(int(x), relu, bits) for x in v]
        o1, o2 = ctx.e2_encrypt(client.base_g, client.base_h, act, [queue.pop(0) for _ in act])
        if rnd == 1:
            o1[1][5, 0] ^= 1
        return o1, o2

    cb = VL.python_round(fn)
    fails(-1, "L3: .*not on the curve", fn=cb)
    table.free()
    # a callback that raises: the exception comes back once the driver has returned, with the round it named
    def boom(rnd, relu, reencrypt, bits, a, b):
        raise KeyError("no such client")

    cb = VL.python_round(boom)
    with pytest.raises(RuntimeError, match="R1: the round callback failed") as e:
        VL.run(ctx, cfg, c1, c2, client.base_g, client.base_h, KEYS, BIAS_RS, cb)
    assert isinstance(e.value.__cause__, KeyError) and cb.error is None
    # a negative weight
    neg = make_cfg()
    w = [row[:] for row in W2]
    w[1][1] = -1
    neg.set_arrays([CFG["filter"][i * 5:(i + 1) * 5] for i in range(5)], CFG["connect"], W1, B1, w, B2)
    fails(-1, "negative", user=client.user, config=neg)
    # a configuration whose third convolution is not 1 x 1
    bad = make_cfg()
    bad.set_pool(2, 1, 1)
    with pytest.raises(vpin_amd.VpinError, match="1 x 1|does not fit") as e:
        bad.counts()
    assert e.value.code == -1


def test_default_configuration_on_the_reference_image_and_weights(ctx):
    """the full-size network without proving: 9108 encryptions, 8094 decryptions, R6 and R7 beyond 2^35 (a table of 2^24 baby
    steps, 2^15 giant steps for those two rounds).  Scores and every round's values against the plaintext model, the label
    counts against the LENET table.  Measured on an MI355X: 0.45 s for the call, the table's build included"""
    from vpin_amd import gadgets as VG
    from vpin_amd import lenet as VL
    image, w1, b1, w2, b2 = LM.reference_model()
    vs, acts = LM.plaintext(FULL, image, w1.tolist(), b1.tolist(), w2.tolist(), b2.tolist())
    cfg = VL.default_config(w1, b1, w2, b2)
    counts = cfg.counts()
    giants = [int(cfg.c.max_giant[r]) for r in range(7)]
    assert max(abs(v) for v in vs[6]) > 2**35 and all(max(abs(v) for v in vs[r]) < (giants[r] << 24) for r in range(7))
    keys = [hashlib.sha256(b"lenet/full/%d" % i).digest() for i in range(counts["prf_keys"])]
    client = VL.Client(ctx, SK, 1 << 24, giants, EL.splitmix_scalars(0xF03, counts["encryptions"] - 1024))
    scores, rounds, trace = VL.infer(ctx, cfg, client, image, EL.splitmix_scalars(0xF01, 1024), keys, EL.splitmix_scalars(0xF02, counts["bias_r"]))
    for r in range(7):
        assert [int(a) for a in rounds[r][0]] == vs[r] and [int(a) for a in rounds[r][1]] == acts[r], "R%d" % (r + 1)
    assert [int(a) for a in scores] == acts[6]
    for i, name in enumerate(VL.LABELS):
        t = trace.label(name)
        assert (t.n_mult, t.n_add) == (VG.CONFIGS[name]["n_mult"], VG.CONFIGS[name]["n_add"]) == counts["labels"][i]
    trace.free()
    client.free()
