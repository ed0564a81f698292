"""GPU tests of a batch of images through ONE inference (vpin_net_infer_batch, vpin_net_trace_image_*, vpin_amd.net.infer_batch)
against the single path, vpin_net_infer, which the other tests pin to the reference's recorded runs and to the plaintext models.
A batch is byte for byte its images' single runs, everything image-major (tests/net_batch_model.py builds a batch's inputs and
the client's queue of r from the images' own): the small trained network of fcs_model (CONVMC with bias, POOL, CONVMC under a
table with bias, FCS, FCS) with B = 1, 2 and 3 -- 3 because it is odd: it tells [b][half] from [half][b] and from an
interleaving by pairs; every image has its own crop, keys and r, so a swapped slice shows --, a pinned 8 x 8 case of the
reference's CNN service (CONV, POOL, FC, FC) with B = 2, the batch's label proven and verified, and the refusals.  A table of
2^16 baby steps throughout."""
import re

import numpy as np
import pytest

import elgamal_model as EL
import fcs_model as TM
import net_batch_model as BM
import net_model as NM
from test_gpu_enc_conv import points_of
from test_gpu_net import device_config, pin_points

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


def single_runs(ctx, d, cfg, sk, giants):
    """the reference of every equality: vpin_net_infer per image on that image's own inputs"""
    from vpin_amd import net as VN
    out = []
    for b in range(len(d["images"])):
        client = VN.Client(ctx, sk, NB, giants, d["client_r"][b])
        scores, rounds, trace = VN.infer(ctx, cfg, client, d["images"][b], d["image_r"][b], d["keys"][b], d["bias_r"][b])
        client.free()
        out.append(dict(scores=scores, rounds=rounds, trace=trace))
    return out


def batch_run(ctx, d, cfg, sk, giants, B):
    """the first B images through one inference, the client's queue built from the images' own"""
    from vpin_amd import net as VN
    client = VN.Client(ctx, sk, NB, giants, BM.client_queue(d["model"], d["client_r"][:B]))
    try:
        return VN.infer_batch(ctx, cfg, client, d["images"][:B], d["image_r"][:B], d["keys"][:B], d["bias_r"][:B])
    finally:
        client.free()


@pytest.fixture(scope="module")
def trained(ctx):
    d = BM.trained_inputs(3)
    cfg = TM.device_config(d["model"], GIANTS)
    singles = single_runs(ctx, d, cfg, SK, GIANTS)
    plain = [TM.net_plaintext(d["model"], np.array(im).reshape(1, 10, 10)) for im in d["images"]]
    yield dict(d, cfg=cfg, singles=singles, plain=plain)
    for s in singles:
        s["trace"].free()


def views(t, left=True):
    """a ConvTrace as flat arrays: output, the two lists and, for a layer call, the left sides"""
    ox, oy, oi = t.output()
    w, mx, my = t.mults()
    out = [ox.reshape(-1, 32), oy.reshape(-1, 32), oi.reshape(-1), np.array(w, dtype=object), mx, my] + list(t.adds())
    return out + list(t.left()) if left else out


def assert_views_are(got, parts, what):
    for j, g in enumerate(got):
        assert np.array_equal(g, np.concatenate([p[j] for p in parts])), "%s, array %d" % (what, j)


def assert_batch_is_its_images(scores, rounds, trace, singles):
    B = len(singles)
    assert trace.images == B and trace.n_layers == singles[0]["trace"].n_layers
    for i in range(trace.n_layers):
        got, alone = trace.layer(i), [s["trace"].layer(i) for s in singles]
        assert (got.P, got.oh, got.ow) == (B * alone[0].P, alone[0].oh, alone[0].ow), "layer %d is ONE call over B times the planes" % i
        assert (got.n_mult, got.n_add) == (B * alone[0].n_mult, B * alone[0].n_add)
        assert_views_are(views(got), [views(a) for a in alone], "layer %d" % i)
    assert len(rounds) == len(singles[0]["rounds"])
    for r, (v, act) in enumerate(rounds):
        assert np.array_equal(v, np.concatenate([s["rounds"][r][0] for s in singles])), "round %d v" % r
        assert np.array_equal(act, np.concatenate([s["rounds"][r][1] for s in singles])), "round %d act" % r
    labels = [s["trace"].label() for s in singles]
    for b, alone in enumerate(labels):
        got = trace.image_label(b)
        assert (got.P, got.oh, got.ow, got.n_mult, got.n_add) == (alone.P, alone.oh, alone.ow, alone.n_mult, alone.n_add)
        assert_views_are(views(got, left=False), [views(alone, left=False)], "the label of image %d" % b)
        assert np.array_equal(scores[b], singles[b]["scores"])
    whole = trace.label()
    assert (whole.P, whole.n_mult, whole.n_add) == (B * labels[0].P, B * labels[0].n_mult, B * labels[0].n_add)
    assert_views_are(views(whole, left=False), [views(l, left=False) for l in labels], "the batch's label")
    for got, alone in zip(trace.result(), zip(*[s["trace"].result() for s in singles])):  # c1, then c2
        for j in range(3):
            assert np.array_equal(np.asarray(got[j]).reshape(B, -1), np.stack([np.asarray(a[j]).reshape(-1) for a in alone]))


@pytest.mark.parametrize("B", [1, 2, 3])
def test_trained_network_batch_is_its_images_single_runs(ctx, trained, B):
    scores, rounds, trace = batch_run(ctx, trained, trained["cfg"], SK, GIANTS, B)
    try:
        assert scores.shape == (B, 3)
        assert_batch_is_its_images(scores, rounds, trace, trained["singles"][:B])
        for b in range(B):
            assert [int(a) for a in scores[b]] == trained["plain"][b][1][-1], "image %d: the plaintext model's scores" % b
        label = trace.label()
        assert (label.n_mult, label.n_add) == (B * 130, B * 632)
        assert trained["cfg"].counts(B)["layers"] == [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(5)]
    finally:
        trace.free()


def test_unsigned_kinds_batch_of_two_with_the_pinned_run_as_image_0(ctx):
    pins = NM.pins()
    case = pins["cases"][0]
    d = BM.pinned_inputs(pins, case)
    plain = [NM.plaintext(d["model"], np.array(im).reshape(1, 8, 8)) for im in d["images"]]
    giants = [max(abs(v) for vs, _ in plain for v in vs[r]) // NB + 1 for r in range(4)]
    cfg = device_config(d["model"], giants)
    singles = single_runs(ctx, d, cfg, d["sk"], giants)
    scores, rounds, trace = batch_run(ctx, d, cfg, d["sk"], giants, 2)
    try:
        assert_batch_is_its_images(scores, rounds, trace, singles)
        for b in range(2):
            assert [int(a) for a in scores[b]] == plain[b][1][-1]
        # image 0's slice is the reference's recorded run
        assert [([int(a) for a in BM.part(list(v), 0, 2)], [int(a) for a in BM.part(list(act), 0, 2)]) for v, act in rounds] == \
            [(r["v"], r["act"]) for r in case["rounds"]]
        label = trace.image_label(0)
        w, mx, my = label.mults()
        px, py, rx, ry, rz = label.adds()
        assert [str(v) for v in w] == case["mult_weights"] and points_of(mx, my) == pin_points(pins, case["mult_points"])
        assert points_of(px, py) == pin_points(pins, case["add_p"]) and points_of(rx, ry, rz) == pin_points(pins, case["add_r"])
        r1, r2 = trace.result()
        assert points_of(*(a[0] for a in r1)) == pin_points(pins, case["result"][0])
        assert points_of(*(a[0] for a in r2)) == pin_points(pins, case["result"][1])
    finally:
        trace.free()
        for s in singles:
            s["trace"].free()


def test_the_batchs_label_is_proven_and_an_images_instances_are_its_single_runs(ctx, trained):
    scores, rounds, trace = batch_run(ctx, trained, trained["cfg"], SK, GIANTS, 2)
    try:
        for g in trace.instances():
            assert g.is_sat()
            got = g.snark_prove(SEED_C, SEED_P)
            assert ctx.snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
            g.free()
        assert (trace.image_label(1).n_mult, trace.image_label(1).n_add) == (130, 632)
        for got, alone in zip(trace.image_instances(1), trained["singles"][1]["trace"].instances()):
            assert got.is_sat()
            assert (got.num_cons_unpadded, got.num_vars_unpadded, got.num_inputs, got.nnz) == \
                (alone.num_cons_unpadded, alone.num_vars_unpadded, alone.num_inputs, alone.nnz)
            assert np.array_equal(got.inputs, alone.inputs)
            got.free()
            alone.free()
    finally:
        trace.free()


def _off_curve(c1, index):
    x, y, inf = (np.array(a, copy=True) for a in c1)
    y.reshape(-1, 32)[index, 0] ^= 1
    return x, y, inf


@pytest.mark.parametrize("what", ["B = 0", "B = VPIN_NET_MAX_BATCH + 1", "one key too few", "one bias r too few", "an input point off the curve"])
def test_refusals_leave_the_context_good_for_a_batch(ctx, trained, what):
    import vpin_amd
    from vpin_amd import net as VN
    d = trained
    B = 3 if what == "an input point off the curve" else 2
    client = VN.Client(ctx, SK, NB, GIANTS, BM.client_queue(d["model"], d["client_r"][:B]))
    c1, c2 = client.encrypt(np.array(BM.flat(d["images"][:B]), dtype=np.int64), BM.flat(d["image_r"][:B]))
    keys, bias_r, batch = BM.flat(d["keys"][:B]), BM.flat(d["bias_r"][:B]), B
    if what == "B = 0":
        batch, text = 0, "vpin_net_infer_batch: B = 0 is outside 1 .. VPIN_NET_MAX_BATCH"
    elif what == "B = VPIN_NET_MAX_BATCH + 1":
        batch, text = 1025, "vpin_net_infer_batch: B = 1025 is outside 1 .. VPIN_NET_MAX_BATCH"
    elif what == "one key too few":
        keys, text = keys[:-1], "vpin_net_infer_batch: the number of PRF keys"
    elif what == "one bias r too few":
        bias_r, text = bias_r[:-1], "vpin_net_infer_batch: the number of bias randomness values"
    else:
        c1, text = _off_curve(c1, 250), r"vpin_net_infer_batch: layer 0 \(convmc\): .*is not on the curve E2; the input's c1: vpin_e2_pack: point (\d+):"
    with pytest.raises(vpin_amd.VpinError, match=text) as e:
        VN.run(ctx, d["cfg"], c1, c2, client.base_g, client.base_h, keys, bias_r, client.round_fn, client.user, batch=batch)
    assert e.value.code == -1  # VPIN_EINVAL
    if what == "an input point off the curve":
        index = int(re.search(text, str(e.value)).group(1))
        assert 2 * 100 <= index < 3 * 100 and index == 250, "the index counts over the batch: image = index / (C H W) = 2"
    client.free()
    scores, rounds, trace = batch_run(ctx, d, d["cfg"], SK, GIANTS, 2)
    assert [[int(a) for a in s] for s in scores] == [d["plain"][b][1][-1] for b in range(2)]
    trace.free()
