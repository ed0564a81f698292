"""GPU tests of max pooling inside the client's round through the inference driver (vpin_net_layer's round_pool_k and
round_pool_stride, VPIN_LENET_MAXPOOL, vpin_net_round_pool, vpin_net_client_set_pools) with the ready-made client over a table of
2^16 baby steps.  The network is 1 x 8 x 8: CONVMC 1 -> 2 with a round of ReLU, shifting(., 20) and max pooling (2, 2); CONVMC 2 -> 2;
an ADD whose skip_from names the pooled tensor; FCS 32 -> 3 (tests/maxpool_model.py).  Byte-exact against the model on logarithms:
every round's (v, act), the scores and the label's two lists; the label proven and verified; a batch of three and three clients
under their own keys as the images' single runs; a foreign Python callback that reads round_pool(); the wire with the REPLY
counts; a client whose pooling schedule disagrees with the server's, both ways; isolation with the middle image dropped in the
pooled round; and the multi-client server's refusal of the configuration.  The refusals are ordinary error returns."""
import numpy as np
import pytest

import lenet_model as LM
import maxpool_model as MM
import net_isolate_model as IM
import net_model as NM
from test_gpu_enc_conv import points_of
from test_gpu_net_batch import SEED_C, SEED_P, assert_batch_is_its_images, assert_views_are, views
from test_gpu_net_isolate import InProcess, assert_result_is, assert_slot_is_its_single_run
from test_gpu_net_multi import client_round, image_of, no_exception
from test_gpu_net_wire import Pair, both, ints

pytestmark = pytest.mark.gpu

NB = 1 << 16
GIANT = 1 << 14
OK, EINVAL, ESHAPE, ECOMM = 0, -1, -5, -7
SKS = IM.TWO_ROUND_SKS
MODEL = MM.small_config()
POOLS = MM.pool_schedule(MODEL)
GIANTS = [GIANT] * 4


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and one per client"""
    import vpin_amd
    out = [vpin_amd.Context(0) for _ in range(4)]
    yield out
    for c in reversed(out):
        c.close()


def new_client(ctx, sk, rs, pools=POOLS, giants=GIANTS):
    from vpin_amd import net as VN
    client = VN.Client(ctx, sk, NB, giants, rs)
    return client.set_pools(pools) if pools is not None else client


def single_run(ctx, cfg, d, sk, b):
    from vpin_amd import net as VN
    client = new_client(ctx, sk, d["client_r"][b])
    scores, rounds, trace = VN.infer(ctx, cfg, client, d["images"][b], d["image_r"][b], d["keys"][b], d["bias_r"][b])
    client.free()
    return dict(scores=scores, rounds=rounds, trace=trace)


@pytest.fixture(scope="module")
def net(ctxs):
    """the network over three images: the single runs under one key (a batch's images) and under a key each (the clients')"""
    from vpin_amd import elgamal as E
    d = MM.inputs(MODEL, 3)
    cfg = MM.device_config(MODEL, GIANTS)
    same = [single_run(ctxs[0], cfg, d, SKS[0], b) for b in range(3)]
    refs = {0: same[0], 1: single_run(ctxs[0], cfg, d, SKS[1], 1), 2: single_run(ctxs[0], cfg, d, SKS[2], 2)}
    base_g = E.BaseTable(ctxs[0])
    yield dict(d, cfg=cfg, same=same, refs=refs, sks=SKS, base_g=base_g, pubs=[E.keygen(base_g, sk) for sk in SKS])
    base_g.free()
    for r in same + [refs[1], refs[2]]:
        r["trace"].free()


def model_run(d, sk, b=0):
    """the model on discrete logarithms under the same keys and randomness -> (layers, label, rounds seen)"""
    c1, c2 = NM.log_encrypt(sk, d["images"][b], d["image_r"][b])
    biases, pos = [], 0
    for l in MODEL["layers"]:
        if l.get("bias") is not None:
            biases.append(NM.log_encrypt(sk, l["bias"], d["bias_r"][b][pos:pos + len(l["bias"])]))
            pos += len(l["bias"])
    seen = []
    layers, label = MM.infer_model(MM.LOGS, MODEL, [c1], [c2], [d["keys"][b]], [biases], MM.log_client(sk, d["client_r"][b], seen, POOLS))
    return layers, label, seen


def test_the_network_is_the_models_byte_for_byte(net):
    run, trace = net["same"][0], net["same"][0]["trace"]
    layers, exp, seen = model_run(net, SKS[0])
    assert ints(run["rounds"]) == [(list(v), list(a)) for v, a in seen], "every round's (v, act)"
    assert [(len(v), len(a)) for v, a in run["rounds"]] == [(128, 32), (32, 32), (32, 32), (3, 3)]
    vs, acts = MM.net_plaintext(MODEL, net["images"][0])
    assert [r[0] for r in ints(run["rounds"])] == vs and [r[1] for r in ints(run["rounds"])] == acts
    assert [int(a) for a in run["scores"]] == acts[-1]
    counts = MM.net_counts(MODEL)
    label = trace.label()
    assert (label.n_mult, label.n_add) == (counts["n_mult"], counts["n_add"])
    assert [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(trace.n_layers)] == counts["layers"] == net["cfg"].counts()["layers"]
    assert [(trace.layer(i).P, trace.layer(i).oh, trace.layer(i).ow) for i in range(4)] == [(4, 8, 8), (4, 4, 4), (4, 4, 4), (2, 1, 3)]
    conv = LM.logs_to_points
    w, mx, my = label.mults()
    px, py, rx, ry, rz = label.adds()
    assert w == [m[0] for m in exp["mults"]] and points_of(mx, my) == conv([m[1] for m in exp["mults"]])
    assert points_of(px, py) == conv([a[0] for a in exp["adds"]]) and points_of(rx, ry, rz) == conv([a[1] for a in exp["adds"]])
    add = trace.layer(2)  # its second operand is the pooled tensor: the encryption of round 0's 32 maxima
    assert points_of(*add.output()) == conv([v for plane in layers[2]["out"] for v in plane])


def test_both_label_instances_are_proven_and_verified(ctxs, net):
    gm, ga = net["same"][0]["trace"].instances()
    for g in (gm, ga):
        assert g.is_sat()
        got = g.snark_prove(SEED_C, SEED_P)
        assert ctxs[0].snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
        g.free()


def test_a_batch_of_three_is_its_images_single_runs(ctxs, net):
    from vpin_amd import net as VN
    client = new_client(ctxs[0], SKS[0], MM.client_queue(MODEL, net["client_r"]))
    scores, rounds, trace = VN.infer_batch(ctxs[0], net["cfg"], client, net["images"], net["image_r"], net["keys"], net["bias_r"])
    client.free()
    try:
        assert scores.shape == (3, 3) and [(len(v), len(a)) for v, a in rounds] == [(384, 96), (96, 96), (96, 96), (9, 9)]
        assert_batch_is_its_images(scores, rounds, trace, net["same"])
        for b in range(3):
            assert_slot_is_its_single_run(trace, b, net["same"][b])
        assert net["cfg"].counts(3)["layers"] == [(trace.layer(i).n_mult, trace.layer(i).n_add) for i in range(4)]
    finally:
        trace.free()


class Pooling(InProcess):
    """InProcess whose clients hold the pooling schedule and whose round function, a foreign Python callback, reads round_pool():
    it hands every client its image's planes with the flag the driver gave, and takes back the pooled count"""

    def __init__(self, ctxs, d, drop=None):
        super().__init__(ctxs, d, giants=GIANTS, drop=drop)
        for c in self.clients:
            c.set_pools(POOLS)
        self.shapes = []

    def round(self, rnd, relu, reencrypt, bits, r1, r2):
        from vpin_amd import net as VN
        slots = VN.round_images()
        planes, H, W, k, stride = shape = VN.round_pool()
        self.seen.append((rnd, slots))
        self.shapes.append((rnd, shape))
        n = len(slots)
        assert planes % n == 0 and planes * H * W == r1[2].shape[0]
        per_out = planes // n * (MM.out_dims(H, W, k, stride)[0] * MM.out_dims(H, W, k, stride)[1] if k else H * W)
        flags = (1 if relu else 0) | (2 if reencrypt else 0) | (VN.MAXPOOL if k else 0)
        outs = [client_round(self.clients[b], rnd, flags, bits, image_of(r1, at, n), image_of(r2, at, n)) for at, b in enumerate(slots)]
        if self.drop:
            self.drop(self, rnd, slots)
        if not reencrypt:
            return None
        return tuple(tuple(np.concatenate([o[h][j][:per_out] for o in outs]) for j in range(3)) for h in range(2))


def test_three_clients_under_their_own_keys_through_a_callback_that_reads_round_pool(ctxs, net):
    run = Pooling(ctxs, net)
    trace = run.run(ctxs[0], "infer_multi")
    try:
        assert run.shapes == [(0, (6, 8, 8, 2, 2)), (1, (6, 4, 4, 0, 0)), (2, (6, 4, 4, 0, 0)), (3, (3, 1, 3, 0, 0))]
        assert trace.images == 3 and all(trace.layer_images(i) == [0, 1, 2] for i in range(4))
        for b in range(3):
            assert_slot_is_its_single_run(trace, b, net["refs"][b], run)
        assert_result_is(trace, [0, 1, 2], net["refs"])
    finally:
        trace.free()
        run.free()


@pytest.mark.timeout(120)
def test_the_middle_image_dropped_in_the_pooled_round(ctxs, net):
    """the callback drops image 1 in round 0, the round that pools: the batch goes on at the POOLED per-image size, the kept pooled
    tensor (the ADD's second operand) without image 1 too, and images 0 and 2 finish as their single runs"""
    from vpin_amd import net as VN

    def drop(run, rnd, slots):
        if rnd == 0:
            VN.round_drop_images([1], ECOMM, "slot 1 is gone")

    run = Pooling(ctxs, net, drop=drop)
    trace, status = run.run(ctxs[0], "infer_isolated")
    try:
        assert status[1] == dict(code=ECOMM, layer=0, round=0, text="slot 1 is gone") and [status[0]["code"], status[2]["code"]] == [OK, OK]
        assert [trace.layer_images(i) for i in range(4)] == [[0, 1, 2], [0, 2], [0, 2], [0, 2]]
        assert [trace.layer(i).P for i in range(4)] == [12, 8, 8, 4]
        assert run.shapes == [(0, (6, 8, 8, 2, 2)), (1, (4, 4, 4, 0, 0)), (2, (4, 4, 4, 0, 0)), (3, (2, 1, 3, 0, 0))]
        assert_slot_is_its_single_run(trace, 1, net["refs"][1], layers=[0])
        for b in (0, 2):
            assert_slot_is_its_single_run(trace, b, net["refs"][b], run)
        assert_result_is(trace, [0, 2], net["refs"])
        assert VN.last_isolation() == dict(refused=0, dropped=1, repeats=0)
    finally:
        trace.free()
        run.free()


def reply_bytes(sched, pools, batch=1):
    """what the REPLYs of a run carry: per round that encrypts again, 64 bytes per pooled element"""
    out = []
    for (flags, _, cnt), (H, W, k, stride) in zip(sched, pools):
        n = cnt // (H * W) * MM.out_dims(H, W, k, stride)[0] * MM.out_dims(H, W, k, stride)[1] if k else cnt
        out.append(n if flags & 2 else 0)
    return out


@pytest.mark.timeout(240)
@pytest.mark.parametrize("B", [1, 2])
def test_over_a_socketpair(ctxs, net, B):
    """serve / Client.run (B = 1) and serve_batch with two images: the client's values and the server's trace are the in-process
    runs', and the REPLY to the pooled round carries the pooled count -- any other count vpin_wire_round refuses"""
    from vpin_amd import net as VN
    cfg = net["cfg"]
    sched = VN.schedule(cfg, batch=B)
    assert sched == [(7, 20, 128 * B), (2, 20, 32 * B), (3, 0, 32 * B), (0, 0, 3 * B)]
    replies = reply_bytes(sched, POOLS)
    assert replies == [32 * B, 32 * B, 32 * B, 0]
    client = new_client(ctxs[1], SKS[0], MM.client_queue(MODEL, net["client_r"][:B]))
    pair = Pair()
    flat = lambda a: [v for x in a for v in x]
    if B == 1:
        server = lambda: VN.serve(ctxs[0], cfg, pair.server, net["keys"][0], net["bias_r"][0])
    else:
        server = lambda: VN.serve(ctxs[0], cfg, pair.server, flat(net["keys"][:B]), flat(net["bias_r"][:B]), max_batch=B)
    trace, res = both(server, lambda: client.run(pair.client, flat(net["images"][:B]), flat(net["image_r"][:B]), sched))
    no_exception(trace, res)
    try:
        scores, rounds = res
        singles = net["same"][:B]
        for r, (v, act) in enumerate(rounds):
            assert np.array_equal(v, np.concatenate([s["rounds"][r][0] for s in singles])), "round %d v" % r
            assert np.array_equal(act, np.concatenate([s["rounds"][r][1] for s in singles])), "round %d act" % r
        for i in range(4):
            assert_views_are(views(trace.layer(i)), [views(s["trace"].layer(i)) for s in singles], "layer %d" % i)
        for b in range(B):
            assert_views_are(views(trace.image_label(b), left=False), [views(singles[b]["trace"].label(), left=False)], "the label of image %d" % b)
        up = 24 * (2 + 4) + 32 + 64 * (64 * B + sum(replies))       # HELLO, INPUT and four REPLYs
        down = 24 * (4 + 1) + 64 * sum(cnt for _, _, cnt in sched)   # four ROUNDs and DONE
        assert pair.client.stats() == dict(bytes_sent=up, bytes_received=down, frames_sent=6, frames_received=5)
        assert pair.server.stats() == dict(bytes_sent=down, bytes_received=up, frames_sent=5, frames_received=6)
    finally:
        trace.free()
        client.free()
        pair.close()


def tiny(maxpool):
    """1 x 4 x 4 through a 1 x 1 convolution and one round that may pool (2, 2) and encrypts nothing: valid either way"""
    from vpin_amd import net as VN
    return VN.Config(1, 4, 4, 13).convmc([[[[3]]]]).round(relu=True, max_giant=4, reencrypt=False, maxpool=maxpool)


TINY_IMAGE = [5, -7, 9, 11, 2, 40, -3, 6, 8, 1, -20, 4, 12, 7, 3, 10]


@pytest.mark.parametrize("server_pools", [True, False])
def test_a_client_whose_pooling_schedule_disagrees_decrypts_nothing(ctxs, server_pools):
    """in both directions: VPIN_ESHAPE with a text that gives both sides, vpin_net_client_values empty for that round, and no r
    consumed -- the same client, given the server's schedule, then runs as a fresh one does"""
    import vpin_amd
    from vpin_amd import net as VN
    import elgamal_model as EL
    server_cfg, other_cfg = tiny((2, 2) if server_pools else None), tiny(None if server_pools else (2, 2))
    rs, keys = EL.splitmix_scalars(0x5A1, 16), [NM.net_key(900 + i) for i in range(2)]
    client = VN.Client(ctxs[1], SKS[0], NB, [4], EL.splitmix_scalars(0x5A2, 4))
    client.set_pools(VN.pool_schedule(other_cfg))
    text = ("round 0: the server asks for max pooling \\(flags 5\\), the client's schedule has none in this round" if server_pools else
            "round 0: the server asks for a round without max pooling, the client's schedule pools 4 x 4 planes by k = 2, stride = 2")
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_infer: round 0: vpin_net_client_round: " + text) as e:
        VN.infer(ctxs[1], server_cfg, client, TINY_IMAGE, rs, keys, [])
    assert e.value.code == ESHAPE
    v, act = client.values(0)
    assert len(v) == 0 and len(act) == 0, "nothing was decrypted"
    client.set_pools(VN.pool_schedule(server_cfg))
    scores, rounds, trace = VN.infer(ctxs[1], server_cfg, client, TINY_IMAGE, rs, keys, [])
    trace.free()
    v = [3 * x for x in TINY_IMAGE]
    want = MM.pooled_round(v, 1, 4, 4, 2, 2, 1, 0) if server_pools else [max(x, 0) for x in v]
    assert ints(rounds) == [(v, want)] and [int(a) for a in scores] == want
    # a count that is no multiple of the client's H * W is refused the same way
    if server_pools:
        client.set_pools([(3, 3, 2, 1)])
        with pytest.raises(vpin_amd.VpinError, match="the server sends 16 ciphertexts, the client's schedule pools planes of 3 x 3 = 9") as e:
            VN.infer(ctxs[1], server_cfg, client, TINY_IMAGE, rs, keys, [])
        assert e.value.code == ESHAPE and len(client.values(0)[0]) == 0
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_client_set_pools: round 0: H, W, k and stride are neither all zero nor a window") as e:
        client.set_pools([(4, 4, 5, 1)])
    assert e.value.code == EINVAL
    client.free()


def test_a_disagreeing_client_over_the_wire_consumes_no_r(ctxs, net):
    """the flags of the client's wire schedule carry bit 4 but its pooling schedule has none: the round is refused by the client
    before anything is decrypted, the server hears ERROR; then the same client, with the schedule, is served as a fresh one"""
    import vpin_amd
    from vpin_amd import net as VN
    cfg, sched = net["cfg"], VN.schedule(net["cfg"])
    client = new_client(ctxs[1], SKS[0], net["client_r"][0], pools=None)
    pair = Pair()
    trace, res = both(lambda: VN.serve(ctxs[0], cfg, pair.server, net["keys"][0], net["bias_r"][0]),
                      lambda: client.run(pair.client, net["images"][0], net["image_r"][0], sched))
    pair.close()
    assert isinstance(res, vpin_amd.VpinError) and res.code == ESHAPE and "the server asks for max pooling (flags 7)" in str(res)
    assert isinstance(trace, vpin_amd.VpinError) and trace.code == ECOMM and "the server asks for max pooling" in str(trace)
    assert len(client.values(0)[0]) == 0
    client.set_pools(POOLS)
    pair = Pair()
    trace, res = both(lambda: VN.serve(ctxs[0], cfg, pair.server, net["keys"][0], net["bias_r"][0]),
                      lambda: client.run(pair.client, net["images"][0], net["image_r"][0], sched))
    no_exception(trace, res)
    try:
        assert ints(res[1]) == ints(net["same"][0]["rounds"]), "the queue of r was untouched by the refused round"
        assert_views_are(views(trace.label(), left=False), [views(net["same"][0]["trace"].label(), left=False)], "the label")
    finally:
        trace.free()
        client.free()
        pair.close()


def test_the_multi_client_server_refuses_the_configuration(ctxs, net):
    import vpin_amd
    from vpin_amd import net as VN
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_server_create: layer 0: a round with max pooling is not served to several clients yet") as e:
        VN.Server(ctxs[0], net["cfg"], 2)
    assert e.value.code == EINVAL
    server = VN.Server(ctxs[0], tiny(None), 2)  # the same network without the pooling is served
    server.free()
