"""GPU tests of several clients in ONE batched inference (vpin_net_server_*, vpin_net_serve_multi, vpin_net_infer_multi;
vpin_amd.net.Server and net.infer_multi): every client under its own key, the endpoints as threads over socketpairs with a context
each.  The rule is that of a batch (tests/test_gpu_net_batch.py): an image's planes, lists, label and values are byte for byte those
of its client served alone with the same slots' keys and bias r, whoever else is in the batch -- also when one of the others
disappears or misbehaves on the wire and is dropped.  Three clients on the one-layer network of test_gpu_net_wire.py; two clients
on the small trained network (biased convolutions and signed FC layers: the keyed bias encryption is on the path), over the wire
and in process; a hand-written peer that fails in every way the endpoint names, on a two-round network of the smallest sizes;
the server's statistics across calls; and the refusals before anything is read.  2^16 baby steps throughout."""
import ctypes as C
import threading

import numpy as np
import pytest

import elgamal_model as EL
import fcs_model as TM
import net_batch_model as BM
import net_model as NM
import wire_model as WM
from test_gpu_net_batch import assert_views_are, views
from test_gpu_net_wire import WIRE_MS, Pair, assert_traffic, ints, small_model

pytestmark = pytest.mark.gpu

NB = 1 << 16
GIANTS = [1 << 14] * 5
SKS = [0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER, 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER,
       EL.ORDER - 1, 0x55AA55AA55AA55AA55AA55AA % EL.ORDER]
OK, EINVAL, ESHAPE, ECOMM = 0, -1, -5, -7
DONE, ADMISSION = -1, -2


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and one per client"""
    import vpin_amd
    out = [vpin_amd.Context(0) for _ in range(4)]
    yield out
    for c in reversed(out):
        c.close()


def run_all(server_fn, client_fns):
    """server_fn and every client_fn in a thread of its own -> (the server's result, the clients' results), an exception as a
    result; none may hang"""
    out = {}

    def body(key, fn):
        try:
            out[key] = fn()
        except BaseException as e:  # noqa: BLE001
            out[key] = e

    threads = [threading.Thread(target=body, args=("server", server_fn))]
    threads += [threading.Thread(target=body, args=(i, fn)) for i, fn in enumerate(client_fns)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(3 * WIRE_MS / 1000)
        assert not t.is_alive(), "an endpoint did not return"
    return out["server"], [out[i] for i in range(len(client_fns))]


def no_exception(*results):
    for r in results:
        assert not isinstance(r, BaseException), r


def assert_images_are(got, B, first, n, ref, what):
    """the images [first, first + n) of a trace over B images (views of a layer call or of nothing but one image) are `ref`"""
    for j, (g, r) in enumerate(zip(got, ref)):
        per = len(g) // B
        assert per * B == len(g) and np.array_equal(g[first * per:(first + n) * per], r), "%s, array %d" % (what, j)


def assert_client_is_its_own_run(trace, first, n, ref, what):
    """a client's images in every layer of the batch's trace and their labels: those of `ref`, the trace of that client alone"""
    assert trace.n_layers == ref.n_layers and ref.images == n
    for i in range(ref.n_layers):
        assert_images_are(views(trace.layer(i)), trace.images, first, n, views(ref.layer(i)), "%s, layer %d" % (what, i))
    for b in range(n):
        got, alone = trace.image_label(first + b), ref.image_label(b)
        assert (got.n_mult, got.n_add) == (alone.n_mult, alone.n_add)
        assert_views_are(views(got, left=False), [views(alone, left=False)], "%s, the label of its image %d" % (what, b))


def status_is(s, code, stage, first, n, text=""):
    assert (s["code"], s["stage"], s["first_image"], s["n_images"]) == (code, stage, first, n) and text in s["text"], s
    assert (s["text"] == "") == (code == OK)


# ---- three clients on the one-layer network ------------------------------------------------------------------------------------
SMALL_IMAGES = [[3, -50, 7, 9, 11, 13, 15, -17], [-4, 8, 21, -6, 10, 2, -30, 5], [1, 2, 3, 4, 5, 6, 7, 8], [9, -9, 8, -8, 7, -7, 6, 60]]
IMAGES_OF = [(0, 1), (1, 2), (3, 1)]  # per client (first_image, n_images) at B_i = (1, 2, 1)


def small_inputs(i):
    first, n = IMAGES_OF[i]
    return BM.flat(SMALL_IMAGES[first:first + n]), EL.splitmix_scalars(0x9A0 + i, 8 * n), EL.splitmix_scalars(0x9B0 + i, 2 * n)


@pytest.mark.timeout(120)
def test_three_clients_with_three_keys_on_the_one_layer_network(ctxs):
    from vpin_amd import net as VN
    cfg = TM.device_config(small_model(), [4])
    server = VN.Server(ctxs[0], cfg, 4)
    pairs = [Pair() for _ in range(3)]
    clients = [VN.Client(ctxs[1 + i], SKS[i], NB, [4], small_inputs(i)[2]) for i in range(3)]
    scheds = [VN.schedule(cfg, batch=n) for _, n in IMAGES_OF]
    res, got = run_all(lambda: server.serve([p.server for p in pairs], [], []),
                       [lambda i=i: clients[i].run(pairs[i].client, small_inputs(i)[0], small_inputs(i)[1], scheds[i]) for i in range(3)])
    no_exception(res, *got)
    trace, statuses = res
    assert trace.images == 4 and trace.layer(0).P == 8
    for i, (first, n) in enumerate(IMAGES_OF):
        status_is(statuses[i], OK, DONE, first, n)
        plain = [TM.net_plaintext(small_model(), np.array(im).reshape(1, 2, 4)) for im in SMALL_IMAGES[first:first + n]]
        assert ints(got[i][1]) == [([v for vs, _ in plain for v in vs[0]], [a for _, acts in plain for a in acts[0]])]
        assert [int(a) for a in got[i][0]] == [a for _, acts in plain for a in acts[0]]
        assert_traffic(8 * n, scheds[i], pairs[i].client.stats(), pairs[i].server.stats())
    # every client alone through vpin_net_serve_batch, with the same key, image r and queue
    for i, (first, n) in enumerate(IMAGES_OF):
        client = VN.Client(ctxs[1 + i], SKS[i], NB, [4], small_inputs(i)[2])
        pair = Pair()
        alone, res = run_all(lambda: VN.serve(ctxs[0], cfg, pair.server, [], [], max_batch=4),
                             [lambda: client.run(pair.client, small_inputs(i)[0], small_inputs(i)[1], scheds[i])])
        no_exception(alone, *res)
        assert ints(res[0][1]) == ints(got[i][1])
        assert_client_is_its_own_run(trace, first, n, alone, "client %d" % i)
        alone.free()
        client.free()
        pair.close()
    assert server.stats() == dict(calls=1, clients_admitted=3, clients_served=3, images=4, base_tables_built=1)
    trace.free()
    for c in clients:
        c.free()
    for p in pairs:
        p.close()
    server.free()


# ---- two clients on the small trained network --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(ctxs):
    """per image b its single run in process under client b's key, with slot b's keys and bias r: the reference of every equality"""
    from vpin_amd import net as VN
    d = BM.trained_inputs(2)
    cfg = TM.device_config(d["model"], GIANTS)
    refs = []
    for b in range(2):
        client = VN.Client(ctxs[0], SKS[b], NB, GIANTS, d["client_r"][b])
        scores, rounds, trace = VN.infer(ctxs[0], cfg, client, d["images"][b], d["image_r"][b], d["keys"][b], d["bias_r"][b])
        client.free()
        refs.append(dict(scores=scores, rounds=rounds, trace=trace))
    plain = [TM.net_plaintext(d["model"], np.array(im).reshape(1, 10, 10)) for im in d["images"]]
    yield dict(d, cfg=cfg, refs=refs, plain=plain)
    for r in refs:
        r["trace"].free()


def assert_trained_client(t, b, trace, scores, rounds):
    """client b of the trained network: five layers' planes of its image, its label, every round's (v, act), the scores"""
    ref = t["refs"][b]
    assert_client_is_its_own_run(trace, b, 1, ref["trace"], "client %d" % b)
    assert ints(rounds) == ints(ref["rounds"]) and len(rounds) == 5
    assert [r[0] for r in ints(rounds)] == t["plain"][b][0]
    assert [int(a) for a in scores] == t["plain"][b][1][-1] == [int(a) for a in ref["scores"]]


@pytest.mark.timeout(240)
def test_two_clients_on_the_trained_network_are_their_single_runs(ctxs, trained):
    from vpin_amd import net as VN
    t = trained
    server = VN.Server(ctxs[0], t["cfg"], 2)
    pairs = [Pair(), Pair()]
    clients = [VN.Client(ctxs[1 + b], SKS[b], NB, GIANTS, t["client_r"][b]) for b in range(2)]
    sched = VN.schedule(t["cfg"])
    res, got = run_all(lambda: server.serve([p.server for p in pairs], BM.flat(t["keys"]), BM.flat(t["bias_r"])),
                       [lambda b=b: clients[b].run(pairs[b].client, t["images"][b], t["image_r"][b], sched) for b in range(2)])
    no_exception(res, *got)
    trace, statuses = res
    assert trace.images == 2 and trace.n_layers == 5
    for b in range(2):
        status_is(statuses[b], OK, DONE, b, 1)
        assert_trained_client(t, b, trace, *got[b])
        assert_traffic(100, sched, pairs[b].client.stats(), pairs[b].server.stats())
    trace.free()
    for c in clients:
        c.free()
    for p in pairs:
        p.close()
    server.free()


def client_round(client, rnd, flags, bits, c1, c2):
    """vpin_net_client_round on the ciphertexts (c1, c2), each (x, y, inf) -> (c1, c2) encrypted again, or None"""
    from vpin_amd import capi
    ins = [np.ascontiguousarray(a, dtype=np.uint8) for a in tuple(c1) + tuple(c2)]
    n = ins[2].shape[0]
    outs = [np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)] * 2
    outs = [a.copy() for a in outs]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().vpin_net_client_round(C.c_void_p(client.h.value), C.c_int(rnd), C.c_int(flags), C.c_int(bits), *[p(a) for a in ins],
                                          C.c_size_t(n), *[p(a) for a in outs])
    capi._chk(rc, "vpin_net_client_round")
    return (tuple(outs[:3]), tuple(outs[3:])) if flags & 2 else None


def image_of(c, b, B):
    """image b's ciphertexts of a triple over B images"""
    per = c[2].shape[0] // B
    return tuple(np.asarray(a)[b * per:(b + 1) * per] for a in c)


@pytest.mark.timeout(240)
def test_infer_multi_in_process_with_a_client_per_image(ctxs, trained):
    from vpin_amd import elgamal as E
    from vpin_amd import net as VN
    t = trained
    base_g = E.BaseTable(ctxs[0])
    clients = [VN.Client(ctxs[1 + b], SKS[b], NB, GIANTS, t["client_r"][b]) for b in range(2)]
    enc = [clients[b].encrypt(np.array(t["images"][b], dtype=np.int64), t["image_r"][b]) for b in range(2)]
    c1, c2 = (tuple(np.concatenate([e[h][j] for e in enc]) for j in range(3)) for h in range(2))

    def fn(rnd, relu, reencrypt, bits, r1, r2):
        flags = (1 if relu else 0) | (2 if reencrypt else 0)
        outs = [client_round(clients[b], rnd, flags, bits, image_of(r1, b, 2), image_of(r2, b, 2)) for b in range(2)]
        if reencrypt:
            return tuple(tuple(np.concatenate([o[h][j] for o in outs]) for j in range(3)) for h in range(2))

    trace = VN.infer_multi(ctxs[0], t["cfg"], base_g.h, [E.keygen(base_g, sk) for sk in SKS[:2]], [0, 1], c1, c2, BM.flat(t["keys"]),
                           BM.flat(t["bias_r"]), VN.python_round(fn))
    assert trace.images == 2
    for b in range(2):
        rounds = [clients[b].values(r) for r in range(5)]
        assert_trained_client(t, b, trace, rounds[-1][1], rounds)
    trace.free()
    for c in clients:
        c.free()
    base_g.free()


@pytest.mark.timeout(240)
def test_infer_multi_with_one_key_is_infer_batch_byte_for_byte(ctxs, trained):
    from vpin_amd import elgamal as E
    from vpin_amd import net as VN
    t = trained
    queue = BM.client_queue(t["model"], t["client_r"])
    client = VN.Client(ctxs[0], SKS[0], NB, GIANTS, queue)
    _, ref_rounds, ref = VN.infer_batch(ctxs[0], t["cfg"], client, t["images"], t["image_r"], t["keys"], t["bias_r"])
    client.free()
    client = VN.Client(ctxs[0], SKS[0], NB, GIANTS, queue)
    base_g = E.BaseTable(ctxs[0])
    c1, c2 = client.encrypt(np.array(BM.flat(t["images"]), dtype=np.int64), BM.flat(t["image_r"]))
    trace = VN.infer_multi(ctxs[0], t["cfg"], base_g.h, [E.keygen(base_g, SKS[0])], [0, 0], c1, c2, BM.flat(t["keys"]), BM.flat(t["bias_r"]),
                           client.round_fn, client.user)
    assert trace.images == ref.images == 2
    for i in range(5):
        assert_views_are(views(trace.layer(i)), [views(ref.layer(i))], "layer %d" % i)
    assert_views_are(views(trace.label(), left=False), [views(ref.label(), left=False)], "the label")
    assert ints([client.values(r) for r in range(5)]) == ints(ref_rounds)
    for got, exp in zip(trace.result(), ref.result()):
        for u, v in zip(got, exp):
            assert np.array_equal(u, v)
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError, match=r"vpin_net_infer_multi: key_of_image\[1\] = 1 is not below n_pub = 1") as e:
        VN.infer_multi(ctxs[0], t["cfg"], base_g.h, [E.keygen(base_g, SKS[0])], [0, 1], c1, c2, BM.flat(t["keys"]), BM.flat(t["bias_r"]),
                       client.round_fn, client.user)
    assert e.value.code == EINVAL
    trace.free()
    ref.free()
    client.free()
    base_g.free()


# ---- drops, on two signed FC layers 8 -> 4 -> 2 with a round after each --------------------------------------------------------------
def two_round_model():
    w1 = [[((3 * k + 5 * j) % 7) - 3 for j in range(4)] for k in range(8)]
    w2 = [[2, -1], [-3, 1], [1, 2], [-2, -2]]
    rnd = lambda relu, re: dict(relu=relu, shift_bits=0, reencrypt=re)
    return dict(C=1, H=2, W=4, prf_bytes=13, layers=[dict(kind="fcs", N=4, w=w1, bias=[5, -7, 0, 11], round=rnd(1, True)),
                                                     dict(kind="fcs", N=2, w=w2, bias=[-3, 4], round=rnd(0, False))])


GOOD = [dict(sk=SKS[0], image=SMALL_IMAGES[0], image_r=EL.splitmix_scalars(0x9C0, 8), queue=EL.splitmix_scalars(0x9C1, 4)),
        dict(sk=SKS[1], image=SMALL_IMAGES[1], image_r=EL.splitmix_scalars(0x9C2, 8), queue=EL.splitmix_scalars(0x9C3, 4))]
BAD_IMAGE = SMALL_IMAGES[2]
SHORT_MS = 300


class ShortPair(Pair):
    """a Pair whose server side waits SHORT_MS for its peer"""

    def __init__(self):
        from vpin_amd import wire as W
        super().__init__()
        self.server.free()
        self.server = W.Wire.from_fds(self.socks[0].fileno(), self.socks[0].fileno(), SHORT_MS)


@pytest.fixture(scope="module")
def drops(ctxs):
    """the server of up to three images, its keys and bias r per slot, and the references: good client 0 alone in slot 0, good
    client 1 alone in slot 1 (the bad one was not admitted) and in slot 2 (it was, and is dropped later)"""
    from vpin_amd import net as VN
    model = two_round_model()
    counts = TM.net_counts(model)
    assert (counts["prf_keys"], counts["bias_r"], counts["per_round"]) == (4, 6, [4, 2])
    cfg = TM.device_config(model, [4, 4])
    keys = [[NM.net_key(900 + 10 * s + i) for i in range(4)] for s in range(3)]
    bias_r = [EL.splitmix_scalars(0x9C8 + s, 6) for s in range(3)]
    refs = {}
    for g, slot in ((0, 0), (1, 1), (1, 2)):
        client = VN.Client(ctxs[0], GOOD[g]["sk"], NB, [4, 4], GOOD[g]["queue"])
        scores, rounds, trace = VN.infer(ctxs[0], cfg, client, GOOD[g]["image"], GOOD[g]["image_r"], keys[slot], bias_r[slot])
        client.free()
        vs, acts = TM.net_plaintext(model, np.array(GOOD[g]["image"]).reshape(1, 2, 4))
        assert ints(rounds) == list(zip(vs, acts)) and max(abs(v) for r in vs for v in r) < 4 * NB
        refs[g, slot] = dict(scores=scores, rounds=rounds, trace=trace)
    server = VN.Server(ctxs[0], cfg, 3)
    bad = VN.Client(ctxs[3], SKS[3], NB, [4, 4], EL.splitmix_scalars(0x9CF, 64))
    yield dict(cfg=cfg, keys=keys, bias_r=bias_r, refs=refs, server=server, bad=bad, sched=VN.schedule(cfg))
    bad.free()
    server.free()
    for r in refs.values():
        r["trace"].free()


def packed_pair(ctx, c1, c2):
    return bytes(ctx.e2_pack(*[np.concatenate([a, b]) for a, b in zip(c1, c2)]).reshape(-1))


def bad_frames(ctxs, bad, n_images=1):
    """the hand-written peer's HELLO and INPUT payloads, as the protocol says"""
    ctx = ctxs[3]
    hello = bytes(ctx.e2_pack(*ctx.e2_base_mul(bad.base_g, [SKS[3]])).reshape(-1))
    c1, c2 = bad.encrypt(np.array(BAD_IMAGE * n_images, dtype=np.int64), EL.splitmix_scalars(0x9D0, 8 * n_images))
    return hello, packed_pair(ctx, c1, c2)


NON_SQUARE = (5).to_bytes(32, "little")
ADMISSION_MODES = ("identity", "no multiple", "too many", "bad input point")


def bad_peer(ctxs, bad, pair, mode, hello, packed):
    """a client by hand that fails as `mode` says -> the frame the server answers it with, or None where it says nothing"""
    ctx, w, good = ctxs[3], pair.client, WM.pack(WM.G)
    w.send(WM.HELLO, WM.pack(None) if mode == "identity" else hello, cnt=1)
    if mode == "no multiple":
        w.send(WM.INPUT, packed + good * 2, cnt=9)
    elif mode == "bad input point":
        w.send(WM.INPUT, packed[:-32] + NON_SQUARE, cnt=8)
    else:
        w.send(WM.INPUT, packed, cnt=len(packed) // 64)
    if mode == "closes":
        pair.socks[1].close()
        return None
    if mode in ADMISSION_MODES:
        return w.recv()
    h, p = w.recv()
    assert (h["type"], h["round"], h["flags"], h["cnt"]) == (WM.ROUND, 0, 3, 4)
    if mode == "non-square":
        w.send(WM.REPLY, good * 3 + NON_SQUARE + good * 4, round_=0, cnt=4)
        return w.recv()
    if mode == "wrong round":
        w.send(WM.REPLY, good * 8, round_=1, cnt=4)
        return w.recv()
    pts = ctx.e2_unpack(p)  # round 0 answered as the protocol says
    o1, o2 = client_round(bad, 0, h["flags"], h["shift_bits"], tuple(a[:4] for a in pts), tuple(a[4:] for a in pts))
    w.send(WM.REPLY, packed_pair(ctx, o1, o2), round_=0, cnt=4)
    h, p = w.recv()
    assert (h["type"], h["round"], h["flags"], h["cnt"]) == (WM.ROUND, 1, 0, 2)
    if mode == "error":
        w.send_error(ESHAPE, "the client gives up")
        return None
    assert mode == "silent"
    return w.recv()  # says nothing: the server tells it so once its wire's time is up


def serve_with(ctxs, d, wires, peers):
    """the server over `wires` against the peers' functions -> (trace, statuses) or the exception, and the peers' results"""
    return run_all(lambda: d["server"].serve(wires, BM.flat(d["keys"]), BM.flat(d["bias_r"])), peers)


def good_clients(ctxs):
    from vpin_amd import net as VN
    return [VN.Client(ctxs[1 + g], GOOD[g]["sk"], NB, [4, 4], GOOD[g]["queue"]) for g in range(2)]


def assert_good_client(d, g, slot, trace, res, status, pair):
    """good client g in `slot`: VPIN_OK, and exactly the bytes and values of its run without anybody else in that slot"""
    ref = d["refs"][g, slot]
    status_is(status, OK, DONE, slot, 1)
    no_exception(res)
    scores, rounds = res
    assert ints(rounds) == ints(ref["rounds"]) and [int(a) for a in scores] == [int(a) for a in ref["scores"]]
    assert_client_is_its_own_run(trace, slot, 1, ref["trace"], "good client %d in slot %d" % (g, slot))
    assert_traffic(8, d["sched"], pair.client.stats(), pair.server.stats())


CASES = [  # mode, the bad client's code, stage, images it holds, its text, what the server tells it
    ("identity", EINVAL, ADMISSION, 0, "vpin_net_serve_multi: HELLO: the public key is the identity", True),
    ("no multiple", ESHAPE, ADMISSION, 0, "expected INPUT of whole images of 8 ciphertexts, the peer sent cnt 9", True),
    ("too many", ESHAPE, ADMISSION, 0, "the peer sent 3 images, the batch has room for 2 more", True),
    ("bad input point", EINVAL, ADMISSION, 0, "INPUT: vpin_e2_unpack: point 15: x is not on the curve E2", True),
    ("closes", ECOMM, 0, 1, "round 0: vpin_wire: the peer closed the stream", False),
    ("non-square", EINVAL, 0, 1, "round 0: the reply (c1, then c2): vpin_e2_unpack: point 3: x is not on the curve E2", True),
    ("wrong round", ESHAPE, 0, 1, "round 0: the reply is for round 1", True),
    ("error", ECOMM, 1, 1, "round 1: the client: the peer reported an error (-5): the client gives up", False),
    ("silent", ECOMM, 1, 1, "round 1: vpin_wire: timed out after 300 ms waiting for the peer", True),
]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode, code, stage, held, text, told", CASES, ids=[c[0] for c in CASES])
def test_a_bad_client_between_two_good_ones_is_dropped_and_they_finish(ctxs, drops, mode, code, stage, held, text, told):
    d = drops
    pairs = [Pair(), ShortPair() if mode == "silent" else Pair(), Pair()]
    clients = good_clients(ctxs)
    hello, packed = bad_frames(ctxs, d["bad"], 3 if mode == "too many" else 1)
    run = lambda g, pair: lambda: clients[g].run(pair.client, GOOD[g]["image"], GOOD[g]["image_r"], d["sched"])
    res, got = serve_with(ctxs, d, [p.server for p in pairs],
                          [run(0, pairs[0]), lambda: bad_peer(ctxs, d["bad"], pairs[1], mode, hello, packed), run(1, pairs[2])])
    no_exception(res)
    trace, statuses = res
    assert trace.images == 2 + held
    assert_good_client(d, 0, 0, trace, got[0], statuses[0], pairs[0])
    assert_good_client(d, 1, 1 + held, trace, got[2], statuses[2], pairs[2])
    status_is(statuses[1], code, stage, 1 if held else 0, held, text)
    no_exception(got[1])
    if told:
        h, p = got[1]
        assert h["type"] == WM.ERROR and p[:4] == code.to_bytes(4, "little", signed=True) and text[:40].encode() in p
    else:
        assert got[1] is None
    trace.free()
    for c in clients:
        c.free()
    for p in pairs:
        p.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode, code, text", [("identity", ESHAPE, "vpin_net_serve_multi: no client was admitted"),
                                              ("closes", ECOMM, "vpin_net_serve_multi: round 0: no client is left")], ids=["nobody admitted", "everybody gone"])
def test_all_clients_bad_returns_no_trace_and_the_server_serves_a_good_pair_after(ctxs, drops, mode, code, text):
    import vpin_amd
    d = drops
    pairs = [Pair() for _ in range(3)]
    hello, packed = bad_frames(ctxs, d["bad"])
    res, got = serve_with(ctxs, d, [p.server for p in pairs], [lambda p=p: bad_peer(ctxs, d["bad"], p, mode, hello, packed) for p in pairs])
    assert isinstance(res, vpin_amd.VpinError) and res.code == code and text in str(res), res
    no_exception(*got)
    for i, s in enumerate(res.statuses):
        if mode == "identity":
            status_is(s, EINVAL, ADMISSION, 0, 0, "the public key is the identity")
        else:
            status_is(s, ECOMM, 0, i, 1, "the peer closed the stream")
    for p in pairs:
        p.close()
    # the same server and contexts, a good pair
    pairs = [Pair(), Pair()]
    clients = good_clients(ctxs)
    res, got = serve_with(ctxs, d, [p.server for p in pairs],
                          [lambda g=g: clients[g].run(pairs[g].client, GOOD[g]["image"], GOOD[g]["image_r"], d["sched"]) for g in range(2)])
    no_exception(res)
    trace, statuses = res
    for g in range(2):
        assert_good_client(d, g, g, trace, got[g], statuses[g], pairs[g])
    trace.free()
    for c in clients:
        c.free()
    for p in pairs:
        p.close()


# ---- the server object ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_a_server_builds_its_table_once_for_three_calls(ctxs):
    from vpin_amd import net as VN
    cfg = TM.device_config(small_model(), [4])
    server = VN.Server(ctxs[0], cfg, 2)
    assert server.stats() == dict(calls=0, clients_admitted=0, clients_served=0, images=0, base_tables_built=1)
    sched = VN.schedule(cfg)
    for call in range(3):
        i = call % 2 * 2  # clients 0 and 2 hold one image each
        client = VN.Client(ctxs[1], SKS[call], NB, [4], small_inputs(i)[2])
        pair = Pair()
        res, got = run_all(lambda: server.serve([pair.server], [], []), [lambda: client.run(pair.client, small_inputs(i)[0], small_inputs(i)[1], sched)])
        no_exception(res, *got)
        status_is(res[1][0], OK, DONE, 0, 1)
        plain = TM.net_plaintext(small_model(), np.array(small_inputs(i)[0]).reshape(1, 2, 4))
        assert [int(a) for a in got[0][0]] == plain[1][0]
        res[0].free()
        client.free()
        pair.close()
    assert server.stats() == dict(calls=3, clients_admitted=3, clients_served=3, images=3, base_tables_built=1)
    server.free()


@pytest.mark.timeout(60)
def test_the_einvals_come_before_anything_is_read(ctxs):
    import vpin_amd
    from vpin_amd import capi
    from vpin_amd import net as VN
    cfg = TM.device_config(small_model(), [4])
    server = VN.Server(ctxs[0], cfg, 2)
    pairs = [Pair() for _ in range(3)]
    for p in pairs:
        p.client.send(WM.HELLO, WM.pack(WM.G), cnt=1)  # a peer by hand: its bytes wait in the stream
    wires = [p.server for p in pairs]
    for args, text in [(([], [], []), "n_wires is outside 1 .. max_batch"), ((wires, [], []), "n_wires is outside 1 .. max_batch"),
                       (([wires[0], wires[0]], [], []), "the same wire is given twice"),
                       ((wires[:2], [NM.net_key(1)], []), "n_keys or n_bias_r is not max_batch times what one image consumes"),
                       ((wires[:2], [], [5]), "n_keys or n_bias_r is not max_batch times what one image consumes")]:
        with pytest.raises(vpin_amd.VpinError) as e:
            server.serve(*args)
        assert e.value.code == EINVAL and "vpin_net_serve_multi: " + text in str(e.value), e.value
    L = capi.lib()
    ws = (C.c_void_p * 2)(wires[0].h, None)
    st = (capi.NetPeerStatus * 2)()
    out = C.c_void_p()
    for bad in ((server.h, ws, 2, None, 0, None, 0, st, C.byref(out)), (server.h, None, 1, None, 0, None, 0, st, C.byref(out)),
                (server.h, ws, 1, None, 0, None, 0, None, C.byref(out)), (None, ws, 1, None, 0, None, 0, st, C.byref(out))):
        assert L.vpin_net_serve_multi(*bad) == EINVAL and b"vpin_net_serve_multi: null argument" in L.vpin_last_error()
    for p in pairs:
        assert p.server.stats() == dict(bytes_sent=0, bytes_received=0, frames_sent=0, frames_received=0)
        assert p.client.stats()["bytes_received"] == 0
    assert server.stats()["calls"] == 0
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_server_create: max_batch is outside") as e:
        VN.Server(ctxs[0], cfg, 0)
    assert e.value.code == EINVAL
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_server_create: the last layer has no round"):
        VN.Server(ctxs[0], TM.device_config(small_model(has_round=False), []), 2)
    for p in pairs:
        p.close()
    server.free()
