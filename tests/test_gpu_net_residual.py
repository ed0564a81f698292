"""GPU tests of skip connections through the inference driver (VPIN_NET_ADD, vpin_net_layer's input_from and skip_from) with the
ready-made client over a table of 2^16 baby steps.  The base network is 1 x 6 x 6: CONVMC 1 -> 2, CONVMC 2 -> 2, ADD of it and layer
0's output, pool 2, FCS 18 -> 3 (tests/residual_model.py).  Byte-exact against the model on logarithms: every round's (v, act), the
scores and the label's two lists, for the base network and its variants (the stride-2 block with the 1 x 1 projection through
input_from, ADD with VPIN_NET_FROM_INPUT, a tensor referenced twice); the label proven and verified; a batch of three and three
clients under their own keys as the images' single runs; the wire with proofs; and isolation: an image that the ADD refuses, or
that the round callback drops while a tensor is kept, leaves the kept tensors too, and the others finish as their single runs
(which a batch of those two alone is, by the batch test's rule).  The refusals are ordinary error returns."""
import numpy as np
import pytest

import lenet_model as LM
import net_isolate_model as IM
import net_model as NM
import residual_model as RM
from test_gpu_enc_conv import points_of
from test_gpu_net_batch import SEED_C, SEED_P, assert_batch_is_its_images, assert_views_are, views
from test_gpu_net_isolate import InProcess, assert_result_is, assert_slot_is_its_single_run
from test_gpu_net_multi import no_exception
from test_gpu_net_wire import Pair, both, ints

pytestmark = pytest.mark.gpu

NB = 1 << 16
GIANT = 1 << 14
OK, ESHAPE, ECOMM = 0, -5, -7
SKS = IM.TWO_ROUND_SKS
SEED32 = bytes((5 * i + 2) % 256 for i in range(32))
MASTER = bytes((7 * i + 1) % 256 for i in range(64))


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and one per client"""
    import vpin_amd
    out = [vpin_amd.Context(0) for _ in range(4)]
    yield out
    for c in reversed(out):
        c.close()


def giants(model):
    return [GIANT] * sum(1 for l in model["layers"] if l.get("round"))


def single_run(ctx, cfg, d, sk, b):
    from vpin_amd import net as VN
    client = VN.Client(ctx, sk, NB, giants(d["model"]), d["client_r"][b])
    scores, rounds, trace = VN.infer(ctx, cfg, client, d["images"][b], d["image_r"][b], d["keys"][b], d["bias_r"][b])
    client.free()
    return dict(scores=scores, rounds=rounds, trace=trace)


@pytest.fixture(scope="module")
def base(ctxs):
    """the base network over three images: the single runs under one key (a batch's images) and under a key each (the clients')"""
    from vpin_amd import elgamal as E
    d = RM.inputs(RM.base_config(), 3)
    cfg = RM.device_config(d["model"], giants(d["model"]))
    same = [single_run(ctxs[0], cfg, d, SKS[0], b) for b in range(3)]
    refs = {0: same[0], 1: single_run(ctxs[0], cfg, d, SKS[1], 1), 2: single_run(ctxs[0], cfg, d, SKS[2], 2)}
    base_g = E.BaseTable(ctxs[0])
    yield dict(d, cfg=cfg, same=same, refs=refs, sks=SKS, base_g=base_g, pubs=[E.keygen(base_g, sk) for sk in SKS])
    base_g.free()
    for r in same + [refs[1], refs[2]]:
        r["trace"].free()


def model_run(d, sk, b=0):
    """the model on discrete logarithms under the same keys and randomness -> (layers, label, rounds seen)"""
    model = d["model"]
    c1, c2 = NM.log_encrypt(sk, d["images"][b], d["image_r"][b])
    biases, pos = [], 0
    for l in model["layers"]:
        if l.get("bias") is not None:
            biases.append(NM.log_encrypt(sk, l["bias"], d["bias_r"][b][pos:pos + len(l["bias"])]))
            pos += len(l["bias"])
    seen = []
    layers, label = RM.infer_model(RM.LOGS, model, [c1], [c2], [d["keys"][b]], [biases], NM.log_client(sk, d["client_r"][b], seen))
    return layers, label, seen


def assert_run_is_the_models(d, run, sk):
    model, trace = d["model"], run["trace"]
    layers, exp, seen = model_run(d, sk)
    assert ints(run["rounds"]) == [(list(v), list(a)) for v, a in seen], "every round's (v, act)"
    vs, acts = RM.net_plaintext(model, d["images"][0])
    assert [r[0] for r in ints(run["rounds"])] == vs and [int(a) for a in run["scores"]] == acts[-1]
    counts = RM.net_counts(model)
    label = trace.label()
    assert (label.n_mult, label.n_add) == (counts["n_mult"], counts["n_add"])
    assert [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(trace.n_layers)] == counts["layers"]
    conv = LM.logs_to_points
    w, mx, my = label.mults()
    px, py, rx, ry, rz = label.adds()
    assert w == [m[0] for m in exp["mults"]] and points_of(mx, my) == conv([m[1] for m in exp["mults"]])
    assert points_of(px, py) == conv([a[0] for a in exp["adds"]]) and points_of(rx, ry, rz) == conv([a[1] for a in exp["adds"]])
    for i, l in enumerate(model["layers"]):
        if l["kind"] == "add":
            t = trace.layer(i)
            (C_, H, W), _ = RM.net_shapes(model)[i]
            assert (t.P, t.oh, t.ow, t.n_mult, t.n_add) == (2 * C_, H, W, 0, 2 * C_ * H * W)
            assert points_of(*t.output()) == conv([v for plane in layers[i]["out"] for v in plane]), "output of the ADD, layer %d" % i


def test_the_base_network_is_the_models_byte_for_byte(base):
    assert_run_is_the_models(base, base["same"][0], SKS[0])
    assert base["cfg"].counts()["layers"][2] == (0, 2 * 2 * 36)


def test_both_label_instances_are_proven_and_verified(ctxs, base):
    gm, ga = base["same"][0]["trace"].instances()
    for g in (gm, ga):
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctxs[0].snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        g.free()


@pytest.mark.parametrize("name", ["projection", "from_input", "twice"])
def test_the_variants_are_the_models_byte_for_byte(ctxs, name):
    d = RM.inputs(RM.CONFIGS[name](), 1)
    cfg = RM.device_config(d["model"], giants(d["model"]))
    run = single_run(ctxs[0], cfg, d, SKS[0], 0)
    try:
        assert_run_is_the_models(d, run, SKS[0])
    finally:
        run["trace"].free()


def test_a_batch_of_three_is_its_images_single_runs(ctxs, base):
    from vpin_amd import net as VN
    client = VN.Client(ctxs[0], SKS[0], NB, giants(base["model"]), RM.client_queue(base["model"], base["client_r"]))
    scores, rounds, trace = VN.infer_batch(ctxs[0], base["cfg"], client, base["images"], base["image_r"], base["keys"], base["bias_r"])
    client.free()
    try:
        assert scores.shape == (3, 3)
        assert_batch_is_its_images(scores, rounds, trace, base["same"])
        for b in range(3):
            assert_slot_is_its_single_run(trace, b, base["same"][b])  # the image_layer shares and the per-image label
        assert trace.layer(2).P == 3 * 4 and base["cfg"].counts(3)["layers"] == [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(5)]
    finally:
        trace.free()


def test_three_clients_under_their_own_keys(ctxs, base):
    run = InProcess(ctxs, base, giants=giants(base["model"]))
    trace = run.run(ctxs[0], "infer_multi")
    try:
        assert trace.images == 3 and all(trace.layer_images(i) == [0, 1, 2] for i in range(5))
        for b in range(3):
            assert_slot_is_its_single_run(trace, b, base["refs"][b], run)
        assert_result_is(trace, [0, 1, 2], base["refs"])
    finally:
        trace.free()
        run.free()


@pytest.mark.timeout(240)
def test_over_a_socketpair_with_proofs(ctxs, base):
    """serve / Client.run: the scores and the server's trace are the in-process run's; then the image's proofs, for the one label
    and per layer (the ADD layer has an addition record and no multiplication record): what proof_expectation says is what
    vpin_net_send_proofs sends, record for record, or the client would accept none"""
    from vpin_amd import net as VN
    ref, cfg = base["same"][0], base["cfg"]
    sched = VN.schedule(cfg)
    assert sched == [(3, 20, 72), (2, 20, 72), (3, 0, 72), (0, 0, 3)]
    expect, per_layer = VN.proof_expectation(cfg), VN.proof_expectation(cfg, per_layer=True)
    counts = RM.net_counts(base["model"])
    assert expect == [(0, 1, counts["n_mult"]), (0, 0, counts["n_add"])]
    assert per_layer == [(1, 1, 36), (1, 0, 176), (2, 1, 72), (2, 0, 68), (3, 0, 144), (4, 0, 108), (5, 1, 36), (5, 0, 40)]
    client = VN.Client(ctxs[1], SKS[0], NB, giants(base["model"]), base["client_r"][0])
    verifier = VN.Verifier(ctxs[1])
    pair = Pair()
    out = {}

    def server():
        trace = VN.serve(ctxs[0], cfg, pair.server, base["keys"][0], base["bias_r"][0])
        VN.send_proofs(ctxs[0], trace, pair.server, master_seed=MASTER)
        VN.send_proofs(ctxs[0], trace, pair.server, per_layer=True, master_seed=MASTER)
        return trace

    def peer():
        res = client.run(pair.client, base["images"][0], base["image_r"][0], sched)
        out["ok"] = client.verify(pair.client, verifier, 1, expect, SEED32)
        out["text"] = verifier.last_text
        out["ok_layers"] = client.verify(pair.client, verifier, 1, per_layer, SEED32)
        out["text_layers"] = verifier.last_text
        return res

    trace, res = both(server, peer)
    no_exception(trace, res)
    try:
        scores, rounds = res
        assert ints(rounds) == ints(ref["rounds"]) and [int(a) for a in scores] == [int(a) for a in ref["scores"]]
        for i in range(5):
            assert_views_are(views(trace.layer(i)), [views(ref["trace"].layer(i))], "layer %d" % i)
        assert_views_are(views(trace.label(), left=False), [views(ref["trace"].label(), left=False)], "the label")
        assert out["ok"] == [[True, True]] and out["text"] == ""
        assert out["ok_layers"] == [[True] * len(per_layer)] and out["text_layers"] == ""
    finally:
        trace.free()
        verifier.free()
        client.free()
        pair.close()


def all_identity(c):
    x, y, f = (np.array(a).copy() for a in c)
    x[:], y[:], f[:] = 0, 0, 1
    return x, y, f


@pytest.mark.timeout(120)
def test_an_image_the_add_refuses_leaves_the_kept_tensor_too(ctxs, base):
    """the round before the ADD (round 1, behind layer 1) returns an all-identity c1 for image 1 only: the ADD's first operand.  The
    ADD refuses planes 4 and 5, image 1 leaves -- from c1, c2 AND from layer 0's kept output, or the second call's operands would be
    those of the wrong images -- and images 0 and 2 finish as their single runs"""
    from vpin_amd import net as VN

    def reply(b, rnd, out):
        return (all_identity(out[0]), out[1]) if (b, rnd) == (1, 1) else out

    run = InProcess(ctxs, base, giants=giants(base["model"]), reply=reply)
    trace, status = run.run(ctxs[0], "infer_isolated")
    try:
        assert [s["code"] for s in status] == [OK, ESHAPE, OK] and (status[1]["layer"], status[1]["round"]) == (2, -1)
        assert status[1]["text"].startswith("vpin_net_infer_isolated: layer 2 (add): vpin_enc_add: the first operand X[4][0] is the identity")
        assert [trace.layer_images(i) for i in range(5)] == [[0, 1, 2], [0, 1, 2], [0, 2], [0, 2], [0, 2]]
        assert [trace.layer(i).P for i in range(5)] == [12, 12, 8, 8, 4]
        assert_slot_is_its_single_run(trace, 1, base["refs"][1], layers=[0, 1])
        for b in (0, 2):
            assert_slot_is_its_single_run(trace, b, base["refs"][b], run)
        assert_result_is(trace, [0, 2], base["refs"])
        assert VN.last_isolation() == dict(refused=1, dropped=0, repeats=1)
    finally:
        trace.free()
        run.free()


@pytest.mark.timeout(120)
def test_an_image_dropped_in_a_round_leaves_the_kept_tensor_too(ctxs, base):
    """the callback drops image 0 in round 1, while layer 0's output is kept for the ADD: images 1 and 2 finish as their single runs"""
    from vpin_amd import net as VN

    def drop(run, rnd, slots):
        if rnd == 1:
            VN.round_drop_images([0], ECOMM, "slot 0 is gone")

    run = InProcess(ctxs, base, giants=giants(base["model"]), drop=drop)
    trace, status = run.run(ctxs[0], "infer_isolated")
    try:
        assert status[0] == dict(code=ECOMM, layer=1, round=1, text="slot 0 is gone") and [s["code"] for s in status[1:]] == [OK, OK]
        assert [trace.layer_images(i) for i in range(5)] == [[0, 1, 2], [0, 1, 2], [1, 2], [1, 2], [1, 2]]
        assert_slot_is_its_single_run(trace, 0, base["refs"][0], layers=[0, 1])
        for b in (1, 2):
            assert_slot_is_its_single_run(trace, b, base["refs"][b], run)
        assert_result_is(trace, [1, 2], base["refs"])
        assert VN.last_isolation() == dict(refused=0, dropped=1, repeats=0)
    finally:
        trace.free()
        run.free()
