"""GPU tests of the reference's LeNet through the layer-list inference (vpin_lenet_as_net, vpin_net_infer[_batch],
vpin_net_serve_batch, vpin_net_serve_multi, vpin_net_trace_image_layer; vpin_amd.net.from_lenet) on the tiny network of
tests/tiny_lenet.py.  The reference of every equality is vpin_lenet_infer itself: one run per image with that image's keys, bias r
and client r.  The layer list alone (B = 1) is that run list by list; in a batch of 2 and of 3 every image's share of every layer
call is its own run's label, byte for byte, and a label taken from a batch is satisfied and proves; over a socketpair the
unchanged client is served seven rounds with the traffic of the wire's formula and gets the plaintext model's scores; two clients
with 2 and 1 images under their own keys end with the bytes of their own runs.  A batch needs the channel sums of all images in
one call (vpin_e2_plane_sums_batch): before it existed a step with sums answered VPIN_EINVAL for B > 1."""
import numpy as np
import pytest

import elgamal_model as EL
import lenet_model as LM
import tiny_lenet as TL
from test_gpu_net_batch import assert_views_are, views
from test_gpu_net_multi import no_exception, run_all, status_is
from test_gpu_net_wire import Pair, assert_traffic, both, ints

pytestmark = pytest.mark.gpu

SKS = [0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER]
GIANTS = [TL.GIANT] * 7
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))
OK, DONE = 0, -1


@pytest.fixture(scope="module")
def plain():
    """the plaintext model of the three images; the bound is asserted before anything goes to the GPU"""
    out = [LM.plaintext(TL.CFG, TL.image(b), TL.W1, TL.B1, TL.W2, TL.B2) for b in range(3)]
    for vs, _ in out:
        assert max(abs(v) for r in vs for v in r) < TL.BOUND and [len(v) for v in vs] == TL.COUNTS["per_round"]
        assert any(v < 0 for v in vs[0]) and any(v < 0 for v in vs[5]), "ReLU cuts something"
    return out


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and one per client"""
    import vpin_amd
    out = [vpin_amd.Context(0) for _ in range(3)]
    yield out
    for c in reversed(out):
        c.close()


@pytest.fixture(scope="module")
def cfgs():
    from vpin_amd import lenet as VL
    from vpin_amd import net as VN
    lcfg = TL.make_cfg(VL)
    return lcfg, VN.from_lenet(lcfg)


@pytest.fixture(scope="module")
def singles(ctxs, cfgs, plain):
    """vpin_lenet_infer of image b under key k alone, with the image's own keys, bias r and client r: (b, k) -> scores, rounds, trace"""
    from vpin_amd import lenet as VL
    out = {}
    for b, k in ((0, 0), (1, 0), (2, 0), (2, 1)):
        client = VL.Client(ctxs[0], SKS[k], TL.NB, GIANTS, TL.client_r(b))
        scores, rounds, trace = VL.infer(ctxs[0], cfgs[0], client, TL.image(b), TL.image_r(b), TL.keys(b), TL.bias_r(b))
        client.free()
        assert ints(rounds) == list(zip(*plain[b])), "vpin_lenet_infer itself gives the plaintext model's values"
        out[b, k] = dict(scores=scores, rounds=rounds, trace=trace)
    yield out
    for s in out.values():
        s["trace"].free()


def assert_image_is_its_lenet_run(trace, b, single, what):
    """image b of a net.Trace against a vpin_lenet_infer run: layer i's share is label L(i + 1), list by list; the result"""
    from vpin_amd import lenet as VL
    ref = single["trace"]
    for i, name in enumerate(VL.LABELS):
        got, alone = trace.image_layer(b, i), ref.label(name)
        assert (got.P, got.oh, got.ow, got.n_mult, got.n_add) == (alone.P, alone.oh, alone.ow, alone.n_mult, alone.n_add), "%s, %s" % (what, name)
        assert_views_are(views(got), [views(alone)], "%s, %s" % (what, name))
    res, want = trace.result(), ref.result()
    for h in range(2):
        for u, v in zip(res[h], want[h]):
            assert np.array_equal(u[b] if trace.images > 1 else u, v), "%s, the result" % what


def test_the_layer_list_alone_is_lenet_infer(ctxs, cfgs, singles):
    from vpin_amd import net as VN
    client = VN.Client(ctxs[0], SKS[0], TL.NB, GIANTS, TL.client_r(0))
    scores, rounds, trace = VN.infer(ctxs[0], cfgs[1], client, TL.image(0), TL.image_r(0), TL.keys(0), TL.bias_r(0))
    client.free()
    s = singles[0, 0]
    assert trace.images == 1 and trace.n_layers == 7
    assert ints(rounds) == ints(s["rounds"]) and [int(a) for a in scores] == [int(a) for a in s["scores"]]
    assert_image_is_its_lenet_run(trace, 0, s, "B = 1")
    for i in range(7):  # without a batch the image's share of a layer call is the call
        assert_views_are(views(trace.image_layer(0, i)), [views(trace.layer(i))], "layer %d" % i)
    trace.free()


@pytest.mark.parametrize("B", [2, 3])
def test_a_batch_is_every_images_own_lenet_run(ctxs, cfgs, singles, plain, B):
    from vpin_amd import lenet as VL
    client = VL.Client(ctxs[0], SKS[0], TL.NB, GIANTS, TL.batch_queue(range(B)))
    bs = range(B)
    scores, rounds, trace = VL.infer_batch(ctxs[0], cfgs[0], client, [TL.image(b) for b in bs], [TL.image_r(b) for b in bs],
                                           [TL.keys(b) for b in bs], [TL.bias_r(b) for b in bs])
    client.free()
    assert trace.images == B and trace.n_layers == 7 and len(rounds) == 7
    for r, (v, act) in enumerate(rounds):
        assert np.array_equal(v, np.concatenate([singles[b, 0]["rounds"][r][0] for b in bs])), "R%d v" % (r + 1)
        assert np.array_equal(act, np.concatenate([singles[b, 0]["rounds"][r][1] for b in bs])), "R%d act" % (r + 1)
    for b in bs:
        assert [int(a) for a in scores[b]] == plain[b][1][6]
        assert_image_is_its_lenet_run(trace, b, singles[b, 0], "image %d of %d" % (b, B))
        call, alone = trace.layer(2), singles[b, 0]["trace"].label("L3")
        assert (call.P, call.n_mult, call.n_add) == (B * alone.P, B * alone.n_mult, B * alone.n_add), "L3 is ONE call over the batch"
    if B == 2:  # a label out of a batch goes to the prover like any other
        gm, ga = trace.image_layer(1, 5).instances()
        for g in (gm, ga):
            assert g.is_sat()
            got = g.snark_prove(SEED_C, SEED_P)
            assert ctxs[0].snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
            g.free()
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_trace_image_layer: null argument, no such image or no such layer"):
        trace.image_layer(B, 0)
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_trace_image_layer"):
        trace.image_layer(0, 7)
    trace.free()


@pytest.mark.timeout(120)
def test_two_images_over_a_socketpair_with_the_unchanged_client(ctxs, cfgs, singles, plain):
    from vpin_amd import net as VN
    cfg = cfgs[1]
    sched = VN.schedule(cfg, batch=2)
    assert len(sched) == 7 and [n for _, _, n in sched] == [2 * n for n in TL.COUNTS["per_round"]]
    client = VN.Client(ctxs[1], SKS[0], TL.NB, GIANTS, TL.batch_queue(range(2)))
    pair = Pair()
    flat = lambda f, n: [v for b in range(n) for v in f(b)]
    trace, res = both(lambda: VN.serve(ctxs[0], cfg, pair.server, flat(TL.keys, 3), flat(TL.bias_r, 3), max_batch=3),
                      lambda: client.run(pair.client, [v for b in range(2) for row in TL.image(b) for v in row], flat(TL.image_r, 2), sched))
    no_exception(trace, res)
    scores, rounds = res
    assert len(rounds) == 7 and [int(a) for a in scores] == plain[0][1][6] + plain[1][1][6]
    for r in range(7):
        assert ints(rounds)[r] == (plain[0][0][r] + plain[1][0][r], plain[0][1][r] + plain[1][1][r]), "R%d" % (r + 1)
    assert trace.images == 2
    for b in range(2):
        assert_image_is_its_lenet_run(trace, b, singles[b, 0], "image %d over the wire" % b)
    assert_traffic(2 * TL.N_PIX, sched, pair.client.stats(), pair.server.stats())
    trace.free()
    client.free()
    pair.close()


@pytest.mark.timeout(120)
def test_two_clients_with_two_and_one_image_end_with_their_own_runs(ctxs, cfgs, singles, plain):
    from vpin_amd import net as VN
    cfg = cfgs[1]
    server = VN.Server(ctxs[0], cfg, 3)
    images_of = [(0, 2), (2, 1)]  # per client (first_image, n_images): the slots 0, 1 and the slot 2
    pairs = [Pair(), Pair()]
    clients = [VN.Client(ctxs[1 + i], SKS[i], TL.NB, GIANTS, TL.batch_queue(range(first, first + n))) for i, (first, n) in enumerate(images_of)]
    scheds = [VN.schedule(cfg, batch=n) for _, n in images_of]
    flat = lambda f, bs: [v for b in bs for v in f(b)]
    pixels = lambda bs: [v for b in bs for row in TL.image(b) for v in row]
    res, got = run_all(lambda: server.serve([p.server for p in pairs], flat(TL.keys, range(3)), flat(TL.bias_r, range(3))),
                       [lambda i=i, bs=range(first, first + n): clients[i].run(pairs[i].client, pixels(bs), flat(TL.image_r, bs), scheds[i])
                        for i, (first, n) in enumerate(images_of)])
    no_exception(res, *got)
    trace, statuses = res
    assert trace.images == 3 and trace.n_layers == 7
    for i, (first, n) in enumerate(images_of):
        status_is(statuses[i], OK, DONE, first, n)
        bs = range(first, first + n)
        scores, rounds = got[i]
        assert [int(a) for a in scores] == [a for b in bs for a in plain[b][1][6]]
        for r in range(7):
            assert np.array_equal(rounds[r][0], np.concatenate([singles[b, i]["rounds"][r][0] for b in bs])), "client %d, R%d" % (i, r + 1)
        for b in bs:
            assert_image_is_its_lenet_run(trace, b, singles[b, i], "client %d, image %d" % (i, b))
        assert_traffic(n * TL.N_PIX, scheds[i], pairs[i].client.stats(), pairs[i].server.stats())
    # the third image under the other key is other bytes: the equality above is not vacuous
    assert not np.array_equal(views(trace.image_layer(2, 0))[0], views(singles[2, 0]["trace"].label("L1"))[0])
    trace.free()
    for c in clients:
        c.free()
    for p in pairs:
        p.close()
    server.free()
