"""GPU test of the trained convolution as a layer kind of the inference driver (VPIN_NET_CONVMC in vpin_net_infer): a
LeNet-5-shaped list -- CONVMC 1 -> 2 (f 3), pool 2 / 2, CONVMC 2 -> 3 under a connection table (f 2), FC, FC -- over a 10 x 10 crop
of the reference's image with signed weights |w| < 2^4, through the ready-made client over a table of 2^16 baby steps.  Every
round's decrypted values against the plaintext model, the label against the model on logarithms and against vpin_net_cfg_counts,
and the one label proven and verified.  tests/test_convmc_model.py asserts without a GPU that every round stays below 2^30."""
import numpy as np
import pytest

import convmc_model as CM
import elgamal_model as EL
import enc_conv_model as EM
import lenet_model as LM
import net_model as NM
from test_gpu_enc_conv import points_of

device_config = CM.device_config

pytestmark = pytest.mark.gpu

NB = 1 << 16
GIANTS = [1 << 14] * 5
SK = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def run(ctx):
    from vpin_amd import net as VN
    model = CM.lenet_shaped_config()
    image = [int(v) for v in CM.lenet_shaped_image().reshape(-1)]
    counts = CM.net_counts(model)
    image_r, bias_r = EL.splitmix_scalars(0x6A1, 100), EL.splitmix_scalars(0x6A2, counts["bias_r"])
    client_r = EL.splitmix_scalars(0x6A3, counts["encryptions"] - 100)
    keys = [NM.net_key(300 + i) for i in range(counts["prf_keys"])]
    assert all(NM.folded_fit(l["w"], l["N"], keys[10 + 2 * j + i], model["prf_bytes"]) for j, l in enumerate(model["layers"][3:]) for i in range(2))
    cfg = device_config(model, GIANTS)
    client = VN.Client(ctx, SK, NB, GIANTS, client_r)
    scores, rounds, trace = VN.infer(ctx, cfg, client, image, image_r, keys, bias_r)
    yield dict(model=model, image=image, counts=counts, cfg=cfg, scores=scores, rounds=rounds, trace=trace, keys=keys, image_r=image_r,
               bias_r=bias_r, client_r=client_r)
    trace.free()
    client.free()


def test_every_round_is_the_plaintext_network(run):
    vs, acts = CM.net_plaintext(run["model"], np.array(run["image"]).reshape(1, 10, 10))
    assert len(run["rounds"]) == 5
    for i, (v, act) in enumerate(run["rounds"]):
        assert [int(a) for a in v] == vs[i], "round %d v" % i
        assert [int(a) for a in act] == acts[i], "round %d act" % i
    assert [int(a) for a in run["scores"]] == acts[-1]


def test_label_is_the_models_and_its_counts_are_the_configurations(run):
    model, trace = run["model"], run["trace"]
    counts = run["cfg"].counts()
    assert counts == dict(run["counts"], rounds=5)
    label = trace.label()
    assert (label.n_mult, label.n_add) == (counts["n_mult"], counts["n_add"]) == (130, 322)
    assert trace.n_layers == 5 and [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(5)] == counts["layers"]
    assert [trace.layer(i).P for i in range(5)] == [4, 4, 6, 2, 2]
    # the model on discrete logarithms, the same keys and randomness
    c1, c2 = NM.log_encrypt(SK, run["image"], run["image_r"])
    biases, pos = [], 0
    for l in model["layers"]:
        if l["kind"] == "fc":
            biases.append(NM.log_encrypt(SK, l["bias"], run["bias_r"][pos:pos + l["N"]]))
            pos += l["N"]
    seen = []
    layers, exp = CM.net_infer_model(EM.LOGS, model, c1, c2, run["keys"], biases, NM.log_client(SK, run["client_r"], seen))
    assert [([int(a) for a in v], [int(a) for a in act]) for v, act in run["rounds"]] == [tuple(s) for s in seen]
    w, mx, my = label.mults()
    px, py, rx, ry, rz = label.adds()
    conv = LM.logs_to_points
    assert w == [m[0] for m in exp["mults"]] and points_of(mx, my) == conv([m[1] for m in exp["mults"]])
    assert points_of(px, py) == conv([a[0] for a in exp["adds"]]) and points_of(rx, ry, rz) == conv([a[1] for a in exp["adds"]])
    for i in (0, 2):  # the trained convolutions' own outputs
        assert points_of(*trace.layer(i).output()) == conv([v for plane in layers[i]["out"] for v in plane]), "output of layer %d" % i


def test_the_one_label_is_proven_and_verified(ctx, run):
    gm, ga = run["trace"].instances()
    for g in (gm, ga):
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        g.free()


def test_missing_weights_are_refused(ctx, run):
    import vpin_amd
    from vpin_amd import net as VN
    cfg = device_config(run["model"], GIANTS)
    cfg.layers[2].w_mc = None
    client = VN.Client(ctx, SK, NB, GIANTS, [])
    c1, c2 = client.encrypt(np.array(run["image"], dtype=np.int64), run["image_r"])
    with pytest.raises(vpin_amd.VpinError, match="a trained convolution has no weights") as e:
        VN.run(ctx, cfg, c1, c2, client.base_g, client.base_h, run["keys"], run["bias_r"], client.round_fn, client.user)
    assert e.value.code == -1
    client.free()
