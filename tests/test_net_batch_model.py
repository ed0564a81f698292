"""The batch rule on the models, without a GPU (tests/net_batch_model.py): the helper that builds a batch's keys, bias r and the
client's queue of r from the images' own, and the expected concatenations, against a model of the batch driver -- one layer call
over the planes [b][half][plane], one round over the values of all images -- on discrete logarithms.  B = 3 on the small trained
network of fcs_model (CONVMC with bias, POOL, CONVMC under a table with bias, FCS, FCS), B = 2 on a pinned 8 x 8 case of
net_pins.json (CONV, POOL, FC, FC).  Also what the inputs of the GPU tests must satisfy: every round of every image inside the
client's range, every folded weight inside 128 bits; and the host side of the interface: the counts and the schedule of a batch."""
import numpy as np
import pytest

import enc_conv_model as EM
import fcs_model as TM
import net_batch_model as BM
import net_model as NM

SK = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EM.ORDER


def single_runs(d, sk, infer_model):
    """per image the single model on its own inputs -> (layers, label, rounds, biases)"""
    out = []
    for b in range(len(d["images"])):
        c1, c2 = NM.log_encrypt(sk, d["images"][b], d["image_r"][b])
        biases, pos = [], 0
        for l in d["model"]["layers"]:
            if l.get("bias") is not None:
                biases.append(NM.log_encrypt(sk, l["bias"], d["bias_r"][b][pos:pos + len(l["bias"])]))
                pos += len(l["bias"])
        assert pos == len(d["bias_r"][b])
        seen = []
        client = NM.log_client(sk, d["client_r"][b], seen)
        layers, label = infer_model(EM.LOGS, d["model"], c1, c2, d["keys"][b], biases, client)
        assert not client.left
        out.append(dict(layers=layers, label=label, rounds=seen, biases=biases, c1=c1, c2=c2))
    return out


def check_batch_is_its_images(d, sk, infer_model):
    B = len(d["images"])
    singles = single_runs(d, sk, infer_model)
    seen = []
    client = NM.log_client(sk, BM.client_queue(d["model"], d["client_r"]), seen)
    layers, label = BM.infer_batch_model(EM.LOGS, d["model"], [s["c1"] for s in singles], [s["c2"] for s in singles], d["keys"],
                                         [s["biases"] for s in singles], client)
    assert not client.left, "the batch consumes exactly the queue the helper builds"
    # the expectation built from the single runs is what the batch driver's model gives ..
    want = BM.concat_layers([s["layers"] for s in singles])
    for i, (got, exp) in enumerate(zip(layers, want)):
        for key in ("out", "mults", "adds", "left"):
            assert list(got.get(key, [])) == exp[key], "layer %d %s" % (i, key)
    assert [(list(v), list(a)) for v, a in seen] == [(v, a) for v, a in BM.concat_rounds([s["rounds"] for s in singles])]
    assert label == BM.concat_labels([s["label"] for s in singles])
    # .. and its b-th part is image b run alone
    for b, s in enumerate(singles):
        for i, got in enumerate(layers):
            for key in ("out", "mults", "adds", "left"):
                assert BM.part(list(got.get(key, [])), b, B) == list(s["layers"][i].get(key, [])), "image %d layer %d %s" % (b, i, key)
        for r, (v, a) in enumerate(seen):
            assert (BM.part(v, b, B), BM.part(a, b, B)) == tuple(s["rounds"][r]), "image %d round %d" % (b, r)
        assert BM.part(label["mults"], b, B) == s["label"]["mults"] and BM.part(label["adds"], b, B) == s["label"]["adds"]
    return singles


def test_trained_network_batch_of_three_is_its_three_images():
    d = BM.trained_inputs(3)
    assert len({tuple(im) for im in d["images"]}) == 3 and len({k for ks in d["keys"] for k in ks}) == 3 * d["counts"]["prf_keys"]
    singles = check_batch_is_its_images(d, SK, TM.net_infer_model)
    # what the GPU test relies on: the plaintext model says the same, and every round of every image stays below 2^30
    for b, s in enumerate(singles):
        vs, acts = TM.net_plaintext(d["model"], np.array(d["images"][b]).reshape(1, 10, 10))
        assert [tuple(r) for r in s["rounds"]] == list(zip(vs, acts))
        assert max(abs(v) for r in vs for v in r) < 1 << 30
        fcs = [l for l in d["model"]["layers"] if l["kind"] == "fcs"]
        assert all(TM.folded_fit_signed(l["w"], l["N"], d["keys"][b][10 + 2 * j + i], d["model"]["prf_bytes"]) for j, l in enumerate(fcs) for i in range(2))


def test_the_queue_is_stage_major_and_differs_from_image_major():
    d = BM.trained_inputs(3)
    assert BM.stage_counts(d["model"]) == [128, 32, 27, 4]
    q = BM.client_queue(d["model"], d["client_r"])
    assert len(q) == 3 * 191 and q[:128] == d["client_r"][0][:128] and q[128:256] == d["client_r"][1][:128]
    assert q[384:416] == d["client_r"][0][128:160] and q != BM.flat(d["client_r"])
    assert BM.client_queue(d["model"], d["client_r"][:1]) == d["client_r"][0], "B = 1: the single run's queue"


def test_unsigned_kinds_batch_of_two_is_its_two_images():
    pins = NM.pins()
    d = BM.pinned_inputs(pins, pins["cases"][0])
    singles = check_batch_is_its_images(d, d["sk"], NM.infer_model)
    assert [(r[0], r[1]) for r in singles[0]["rounds"]] == [(r["v"], r["act"]) for r in pins["cases"][0]["rounds"]], "image 0 is the pinned run"
    for b in range(2):
        assert all(NM.keys_fit(d["model"], d["keys"][b]))
        vs, acts = NM.plaintext(d["model"], np.array(d["images"][b]).reshape(1, 8, 8))
        assert [tuple(r) for r in singles[b]["rounds"]] == list(zip(vs, acts))


def test_counts_and_schedule_of_a_batch():
    from vpin_amd import capi, net
    assert capi.lib().vpin_abi_version() >= 6
    cfg = TM.device_config(TM.trained_config(), [1 << 14] * 5)
    one, three = cfg.counts(), cfg.counts(3)
    assert cfg.counts(1) == one and (three["rounds"], len(three["layers"])) == (one["rounds"], len(one["layers"])) == (5, 5)
    for key in ("n_mult", "n_add", "decryptions", "encryptions", "prf_keys", "bias_r"):
        assert three[key] == 3 * one[key], key
    assert three["layers"] == [(3 * m, 3 * a) for m, a in one["layers"]] and three["per_round"] == [3 * n for n in one["per_round"]]
    assert net.schedule(cfg) == net.schedule(cfg, 1) == [(3, 28, 128), (2, 17, 32), (3, 20, 27), (3, 21, 4), (0, 0, 3)]
    assert net.schedule(cfg, 3) == [(f, s, 3 * n) for f, s, n in net.schedule(cfg)]
