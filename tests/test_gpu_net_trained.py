"""GPU test of a trained model's network through the inference driver: the LeNet-5-shaped list of test_gpu_net_convmc.py over the same
10 x 10 crop with every weight left signed and a bias on every weighted layer -- CONVMC 1 -> 2 (f 3) with bias, pool 2 / 2, CONVMC
2 -> 3 under a connection table (f 2) with bias, FCS 27 -> 4, FCS 4 -> 3 -- through the ready-made client over a table of 2^16 baby
steps.  Every round's decrypted values against the plaintext model, the label against the model on logarithms and against
vpin_net_cfg_counts, the one label proven and verified; VPIN_NET_FC still refuses the signed weights, and a CONVMC layer without a
bias is vpin_enc_conv2d_mc.  tests/test_fcs_model.py asserts without a GPU that every round stays below 2^30."""
import numpy as np
import pytest

import elgamal_model as EL
import enc_conv_model as EM
import fcs_model as TM
import lenet_model as LM
import net_model as NM
from test_gpu_enc_conv import points_of

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
    model = TM.trained_config()
    image = [int(v) for v in TM.trained_image().reshape(-1)]
    counts = TM.net_counts(model)
    image_r, bias_r = EL.splitmix_scalars(0x7A1, 100), EL.splitmix_scalars(0x7A2, counts["bias_r"])
    client_r = EL.splitmix_scalars(0x7A3, counts["encryptions"] - 100)
    keys = [NM.net_key(300 + i) for i in range(counts["prf_keys"])]
    cfg = TM.device_config(model, GIANTS)
    client = VN.Client(ctx, SK, NB, GIANTS, client_r)
    scores, rounds, trace = VN.infer(ctx, cfg, client, image, image_r, keys, bias_r)
    yield dict(model=model, image=image, counts=counts, cfg=cfg, scores=scores, rounds=rounds, trace=trace, keys=keys, image_r=image_r,
               bias_r=bias_r, client_r=client_r)
    trace.free()
    client.free()


def test_every_round_is_the_plaintext_network(run):
    vs, acts = TM.net_plaintext(run["model"], np.array(run["image"]).reshape(1, 10, 10))
    assert len(run["rounds"]) == 5
    for i, (v, act) in enumerate(run["rounds"]):
        assert [int(a) for a in v] == vs[i], "round %d v" % i
        assert [int(a) for a in act] == acts[i], "round %d act" % i
    assert [int(a) for a in run["scores"]] == acts[-1]


def test_label_is_the_models_and_its_counts_are_the_configurations(run):
    model, trace = run["model"], run["trace"]
    counts = run["cfg"].counts()
    assert counts == dict(run["counts"], rounds=5) and counts["bias_r"] == 2 + 3 + 4 + 3
    label = trace.label()
    assert (label.n_mult, label.n_add) == (counts["n_mult"], counts["n_add"]) == (130, 632)
    assert trace.n_layers == 5 and [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(5)] == counts["layers"]
    # the model on discrete logarithms, the same keys and randomness; the bias r are drawn in layer order
    c1, c2 = NM.log_encrypt(SK, run["image"], run["image_r"])
    biases, pos = [], 0
    for l in model["layers"]:
        if l.get("bias") is not None:
            biases.append(NM.log_encrypt(SK, l["bias"], run["bias_r"][pos:pos + len(l["bias"])]))
            pos += len(l["bias"])
    seen = []
    layers, exp = TM.net_infer_model(EM.LOGS, model, c1, c2, run["keys"], biases, NM.log_client(SK, run["client_r"], seen))
    assert [([int(a) for a in v], [int(a) for a in act]) for v, act in run["rounds"]] == [tuple(s) for s in seen]
    w, mx, my = label.mults()
    px, py, rx, ry, rz = label.adds()
    conv = LM.logs_to_points
    assert w == [m[0] for m in exp["mults"]] and points_of(mx, my) == conv([m[1] for m in exp["mults"]])
    assert points_of(px, py) == conv([a[0] for a in exp["adds"]]) and points_of(rx, ry, rz) == conv([a[1] for a in exp["adds"]])
    for i in (0, 2, 3, 4):  # the outputs of the layers this network adds
        assert points_of(*trace.layer(i).output()) == conv([v for plane in layers[i]["out"] for v in plane]), "output of layer %d" % i


def test_the_one_label_is_proven_and_verified(ctx, run):
    gm, ga = run["trace"].instances()
    for g in (gm, ga):
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        g.free()


def test_the_unsigned_kind_still_refuses_a_negative_weight(ctx, run):
    import vpin_amd
    from vpin_amd import net as VN
    model = dict(run["model"], layers=[dict(l, kind="fc") if l["kind"] == "fcs" else l for l in run["model"]["layers"]])
    cfg = TM.device_config(model, GIANTS)
    assert [l.kind for l in cfg.layers][3:] == [VN.FC, VN.FC]
    client = VN.Client(ctx, SK, NB, GIANTS, [])
    c1, c2 = client.encrypt(np.array(run["image"], dtype=np.int64), run["image_r"])
    with pytest.raises(vpin_amd.VpinError, match="a weight of a fully connected layer is negative") as e:
        VN.run(ctx, cfg, c1, c2, client.base_g, client.base_h, run["keys"], run["bias_r"], client.round_fn, client.user)
    assert e.value.code == -1
    client.free()


def test_a_layer_without_a_bias_is_the_unbiased_entry_point(ctx, run):
    """bias = NULL: one CONVMC layer and no round through the driver against vpin_enc_conv2d_mc called directly on the c1 planes and
    then the c2 planes under the same keys -- output, both lists and left sides byte for byte; and it consumes no bias r"""
    from vpin_amd import net as VN
    l0 = {k: v for k, v in run["model"]["layers"][0].items() if k not in ("bias", "round")}
    cfg = TM.device_config(dict(run["model"], layers=[l0]), [])
    assert cfg.counts()["bias_r"] == 0 and cfg.counts()["layers"] == [(36, 32)]
    client = VN.Client(ctx, SK, NB, GIANTS, [])
    c1, c2 = client.encrypt(np.array(run["image"], dtype=np.int64), run["image_r"])
    trace = VN.run(ctx, cfg, c1, c2, client.base_g, client.base_h, run["keys"][:4], [], client.round_fn, client.user)
    x, y, inf = (np.concatenate([np.asarray(a[i]).reshape(100, -1) for a in (c1, c2)]) for i in range(3))
    w = np.array(l0["w"]).reshape(2, 1, 3, 3)
    direct = ctx.enc_conv2d_mc(x, y, inf.reshape(-1), 2, 1, 2, 10, 10, w, None, 3, 3, 0, 1, run["keys"][:4], run["model"]["prf_bytes"])
    got = trace.layer(0)
    assert got.mults()[0] == direct.mults()[0]
    for u, v in zip(list(got.output()) + list(got.adds()) + list(got.mults()[1:]) + list(got.left()),
                    list(direct.output()) + list(direct.adds()) + list(direct.mults()[1:]) + list(direct.left())):
        assert np.array_equal(u, v)
    direct.free()
    trace.free()
    client.free()
