"""GPU tests of images that leave a running batch (vpin_enc_last_refusals, vpin_net_infer_isolated with vpin_net_round_images and
vpin_net_round_drop_images, vpin_net_trace_layer_images, vpin_net_server_set_isolation).  The rule is that of a batch: an image
that stays is byte for byte its single run under its slot's keys and bias r, whoever else was in the batch and whenever they left.
The bad ciphertexts are written by hand: flag 1 with zero coordinates, on the wire wire_model.pack(None); the inputs are those of
tests/net_isolate_model.py, on which the models refuse only what is planted (tests/test_net_isolate_model.py).  The layers'
refusal lists; the two-round 8 -> 4 -> 2 network with an image refused at the first layer, at a later one, dropped by the
callback, all refused, and nobody refused (= vpin_net_infer_multi byte for byte); the small trained network with a survivor's
label proven; and three clients over socketpairs with one whose image a layer refuses, and one silent in round 0, isolation on and
off.  2^16 baby steps throughout."""
import numpy as np
import pytest

import elgamal_model as EL
import fcs_model as TM
import net_batch_model as BM
import net_isolate_model as IM
import wire_model as WM
from test_gpu_net_batch import SEED_C, SEED_P, assert_views_are, views
from test_gpu_net_multi import ShortPair, client_round, image_of, no_exception, packed_pair, run_all, status_is
from test_gpu_net_wire import Pair, assert_traffic, ints

pytestmark = pytest.mark.gpu

NB = 1 << 16
OK, EINVAL, ESHAPE, ECOMM = 0, -1, -5, -7
X_IS_IDENTITY = "vpin_enc_fc_signed: a multiplication operand X[k] is the identity (the witness format has no flag for it)"


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and one per client"""
    import vpin_amd
    out = [vpin_amd.Context(0) for _ in range(4)]
    yield out
    for c in reversed(out):
        c.close()


# ---- 1. the layers say which units refuse --------------------------------------------------------------------------------------------

def case_points(seed, n, identity):
    """vpin_synthetic_points(seed, n) with the identity (zero coordinates, flag 1) where `identity` says"""
    from vpin_amd import gadgets as G
    x, y = G.synthetic_points(seed, n)
    x, y = np.array(x, dtype=np.uint8).reshape(n, 32).copy(), np.array(y, dtype=np.uint8).reshape(n, 32).copy()
    f = np.array([1 if identity(i) else 0 for i in range(n)], dtype=np.uint8)
    x[f == 1] = 0
    y[f == 1] = 0
    return x, y, f


def refused(ctx, call, text):
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError) as e:
        call()
    assert e.value.code == ESHAPE and text in str(e.value), e.value
    return ctx.enc_last_refusals()


def test_the_layers_name_every_unit_that_refuses(ctxs):
    import vpin_amd
    from vpin_amd import gadgets as G
    ctx = ctxs[0]
    c = IM.FCS_CASE
    P, K, N = c["P"], c["K"], c["N"]
    x, y, f = case_points(c["seed"], P * K, lambda i: i // K in c["identity_rows"] and i % K == 0)
    bx, by = G.synthetic_points(c["seed"] + 0x1000, P * N)
    fcs = lambda: ctx.enc_fc_signed(x, y, f, P, K, c["W"], N, bx, by, None, IM.case_keys(P), c["prf_bytes"])
    assert refused(ctx, fcs, X_IS_IDENTITY) == [1, 3]
    # a VPIN_EINVAL leaves the list empty: a coordinate that is no point's
    off = x.copy()
    off[0] = np.frombuffer((5).to_bytes(32, "little"), dtype=np.uint8)
    with pytest.raises(vpin_amd.VpinError, match="is not on the curve E2") as e:
        ctx.enc_fc_signed(off, y, f, P, K, c["W"], N, bx, by, None, IM.case_keys(P), c["prf_bytes"])
    assert e.value.code == EINVAL and ctx.enc_last_refusals() == []
    assert refused(ctx, fcs, X_IS_IDENTITY) == [1, 3]
    # and so does a call that succeeds: row 0 alone
    tr = ctx.enc_fc_signed(x[:K], y[:K], f[:K], 1, K, c["W"], N, bx[:N], by[:N], None, IM.case_keys(1), c["prf_bytes"])
    assert ctx.enc_last_refusals() == []
    tr.free()

    c = IM.CONV_CASE
    per = c["H"] * c["W"]
    x, y, f = case_points(c["seed"], c["P"] * per, lambda i: i // per in c["identity_planes"])
    conv = lambda: ctx.enc_conv2d(x, y, f, c["P"], c["H"], c["W"], c["filt"], c["f"], c["f"], 0, 1, IM.case_keys(c["P"]), c["prf_bytes"])
    assert refused(ctx, conv, "vpin_enc_conv2d: a multiplication operand B'[k] is the identity") == [1]

    c = IM.POOL_CASE
    per = c["H"] * c["W"]
    x, y, f = case_points(c["seed"], c["P"] * per, lambda i: i // per in c["first_pixel_identity"] and i % per == 0)
    pool = lambda: ctx.enc_avgpool2d(x, y, f, c["P"], c["H"], c["W"], c["k"], c["k"], c["scale"])
    assert refused(ctx, pool, "vpin_enc_avgpool2d: an addition accumulator is the identity") == [2]

    c = IM.CONVMC_CASE
    per = c["C"] * c["H"] * c["W"]
    x, y, f = case_points(c["seed"], c["groups"] * per, lambda i: i // per in c["identity_groups"])
    w = np.array(c["w"]).reshape(c["n_out"], c["C"], c["f"], c["f"]).tolist()
    mc = lambda: ctx.enc_conv2d_mc(x, y, f, c["groups"], c["C"], c["n_out"], c["H"], c["W"], w, None, c["f"], c["f"], 0, 1,
                                   IM.case_keys(c["groups"] * c["n_out"]), c["prf_bytes"])
    assert refused(ctx, mc, "vpin_enc_conv2d_mc: a multiplication operand B'[c][k] is the identity") == [2]


# ---- 2 .. 6. in process, on two signed FC layers 8 -> 4 -> 2 with a round after each ----------------------------------------------------

def single_run(ctx, cfg, d, sk, b, giants):
    """slot b alone under the key sk, with the slot's keys, bias r and queue"""
    from vpin_amd import net as VN
    client = VN.Client(ctx, sk, NB, giants, d["client_r"][b])
    scores, rounds, trace = VN.infer(ctx, cfg, client, d["images"][b], d["image_r"][b], d["keys"][b], d["bias_r"][b])
    client.free()
    return dict(scores=scores, rounds=rounds, trace=trace)


@pytest.fixture(scope="module")
def two(ctxs):
    """the two-round network and the single runs: slot b < 3 under sks[b] (in process: a client per image), and slot 3 under sks[2]
    (over the wire the third client's)"""
    from vpin_amd import elgamal as E
    d = IM.two_round_inputs()
    cfg = TM.device_config(d["model"], [4, 4])
    refs = {b: single_run(ctxs[0], cfg, d, d["sks"][b], b, [4, 4]) for b in range(3)}
    refs[3] = single_run(ctxs[0], cfg, d, d["sks"][2], 3, [4, 4])
    base_g = E.BaseTable(ctxs[0])
    pubs = [E.keygen(base_g, sk) for sk in d["sks"]]
    yield dict(d, cfg=cfg, refs=refs, base_g=base_g, pubs=pubs)
    base_g.free()
    for r in refs.values():
        r["trace"].free()


def identity_at(c, index):
    """the ciphertext half c = (x, y, inf) with the identity at `index`"""
    x, y, f = (np.array(a).copy() for a in c)
    x[index] = 0
    y[index] = 0
    f[index] = 1
    return x, y, f


class InProcess:
    """three images, a client each, and the Python round function over whatever slots are at hand"""

    def __init__(self, ctxs, d, giants=(4, 4), reply=None, drop=None):
        from vpin_amd import net as VN
        self.d, self.reply, self.drop = d, reply, drop
        self.clients = [VN.Client(ctxs[1 + b], d["sks"][b], NB, list(giants), d["client_r"][b]) for b in range(3)]
        enc = [self.clients[b].encrypt(np.array(d["images"][b], dtype=np.int64), d["image_r"][b]) for b in range(3)]
        self.c1, self.c2 = (tuple(np.concatenate([e[h][j] for e in enc]) for j in range(3)) for h in range(2))
        self.seen, self.notes = [], []
        self.fn = VN.python_round(self.round)

    def round(self, rnd, relu, reencrypt, bits, r1, r2):
        from vpin_amd import net as VN
        slots = VN.round_images()
        self.seen.append((rnd, slots))
        n, flags = len(slots), (1 if relu else 0) | (2 if reencrypt else 0)
        outs = [client_round(self.clients[b], rnd, flags, bits, image_of(r1, at, n), image_of(r2, at, n)) for at, b in enumerate(slots)]
        if self.drop:
            self.drop(self, rnd, slots)
        if not reencrypt:
            return None
        if self.reply:
            outs = [self.reply(b, rnd, o) for b, o in zip(slots, outs)]
        return tuple(tuple(np.concatenate([o[h][j] for o in outs]) for j in range(3)) for h in range(2))

    def run(self, ctx, how):
        from vpin_amd import net as VN
        d = self.d
        args = (ctx, d["cfg"], d["base_g"].h, d["pubs"], [0, 1, 2], self.c1, self.c2, BM.flat(d["keys"][:3]), BM.flat(d["bias_r"][:3]), self.fn)
        return getattr(VN, how)(*args)

    def free(self):
        for c in self.clients:
            c.free()


def assert_slot_is_its_single_run(trace, b, ref, run=None, layers=None):
    """slot b in the batch's trace: every layer share, its label and, with the run, its client's values are its single run's"""
    layers = range(ref["trace"].n_layers) if layers is None else layers
    for i in layers:
        got, alone = trace.image_layer(b, i), ref["trace"].layer(i)
        assert (got.P, got.n_mult, got.n_add) == (alone.P, alone.n_mult, alone.n_add)
        assert_views_are(views(got), [views(alone)], "slot %d, layer %d" % (b, i))
    if run is not None:
        rounds = [run.clients[b].values(r) for r in range(len(ref["rounds"]))]
        assert ints(rounds) == ints(ref["rounds"]), "slot %d: the client's values" % b
    if len(layers) == ref["trace"].n_layers:
        got, alone = trace.image_label(b), ref["trace"].label()
        assert (got.n_mult, got.n_add) == (alone.n_mult, alone.n_add)
        assert_views_are(views(got, left=False), [views(alone, left=False)], "slot %d, the label" % b)


def assert_result_is(trace, survivors, refs):
    got = trace.result()
    for h in range(2):
        for j in range(3):
            exp = np.stack([np.asarray(refs[b]["trace"].result()[h][j]) for b in survivors])
            assert np.array_equal(np.asarray(got[h][j]).reshape(exp.shape), exp), "the result, half %d array %d" % (h, j)


@pytest.mark.timeout(120)
def test_an_image_the_first_layer_refuses_leaves_and_the_others_are_their_single_runs(ctxs, two):
    import vpin_amd
    run = InProcess(ctxs, two)
    run.c1 = identity_at(run.c1, 8 + 3)  # one identity c1 point of slot 1
    with pytest.raises(vpin_amd.VpinError) as e:
        run.run(ctxs[0], "infer_multi")
    assert e.value.code == ESHAPE and "vpin_net_infer_multi: layer 0 (fcs): " + X_IS_IDENTITY in str(e.value) and run.seen == []
    trace, status = run.run(ctxs[0], "infer_isolated")
    assert [s["code"] for s in status] == [OK, ESHAPE, OK] and (status[1]["layer"], status[1]["round"]) == (0, -1)
    assert status[1]["text"] == "vpin_net_infer_isolated: layer 0 (fcs): " + X_IS_IDENTITY and status[0]["text"] == ""
    assert trace.images == 3 and trace.n_layers == 2 and trace.layer(0).P == 4 and trace.layer(1).P == 4
    assert trace.layer_images(0) == [0, 2] and trace.layer_images(1) == [0, 2] and run.seen == [(0, [0, 2]), (1, [0, 2])]
    for b in (0, 2):
        assert_slot_is_its_single_run(trace, b, two["refs"][b], run)
    assert_result_is(trace, [0, 2], two["refs"])
    for i in range(2):
        with pytest.raises(vpin_amd.VpinError, match="vpin_net_trace_image_layer: image 1 left the batch at layer 0") as e:
            trace.image_layer(1, i)
        assert e.value.code == ESHAPE
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_trace_image_label: image 1 left the batch at layer 0"):
        trace.image_label(1)
    from vpin_amd import net as VN
    assert VN.last_isolation() == dict(refused=1, dropped=0, repeats=1)
    trace.free()
    run.free()


@pytest.mark.timeout(120)
def test_an_image_a_later_layer_refuses_was_there_before(ctxs, two):
    import vpin_amd

    def reply(b, rnd, out):
        return (identity_at(out[0], 0), out[1]) if (b, rnd) == (1, 0) else out  # slot 1's round-0 reply carries an identity c1

    run = InProcess(ctxs, two, reply=reply)
    trace, status = run.run(ctxs[0], "infer_isolated")
    assert [s["code"] for s in status] == [OK, ESHAPE, OK] and (status[1]["layer"], status[1]["round"]) == (1, -1)
    assert "layer 1 (fcs): " + X_IS_IDENTITY in status[1]["text"]
    assert trace.layer_images(0) == [0, 1, 2] and trace.layer_images(1) == [0, 2] and (trace.layer(0).P, trace.layer(1).P) == (6, 4)
    assert_slot_is_its_single_run(trace, 1, two["refs"][1], layers=[0])
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_trace_image_layer: image 1 left the batch at layer 1") as e:
        trace.image_layer(1, 1)
    assert e.value.code == ESHAPE
    for b in (0, 2):
        assert_slot_is_its_single_run(trace, b, two["refs"][b], run)
    assert_result_is(trace, [0, 2], two["refs"])
    trace.free()
    run.free()


@pytest.mark.timeout(120)
def test_the_callback_drops_images_and_the_next_layer_runs_without_them(ctxs, two):
    import vpin_amd
    from vpin_amd import net as VN

    def drop(run, rnd, slots):
        if rnd:
            return
        VN.round_drop_images([0], ECOMM, "slot 0 is gone")
        for bad in ([7], [0], [1, 1]):  # an unknown slot, a slot dropped already, a slot twice in one call
            with pytest.raises(vpin_amd.VpinError, match="is not in the batch, or is dropped twice") as e:
                VN.round_drop_images(bad, ECOMM, "x")
            run.notes.append(e.value.code)

    run = InProcess(ctxs, two, drop=drop)
    trace, status = run.run(ctxs[0], "infer_isolated")
    assert run.notes == [EINVAL] * 3 and run.fn.error is None
    assert status[0] == dict(code=ECOMM, layer=0, round=0, text="slot 0 is gone") and [s["code"] for s in status[1:]] == [OK, OK]
    assert trace.layer_images(0) == [0, 1, 2] and trace.layer_images(1) == [1, 2] and (trace.layer(0).P, trace.layer(1).P) == (6, 4)
    assert run.seen == [(0, [0, 1, 2]), (1, [1, 2])]
    assert_slot_is_its_single_run(trace, 0, two["refs"][0], layers=[0])
    for b in (1, 2):
        assert_slot_is_its_single_run(trace, b, two["refs"][b], run)
    assert_result_is(trace, [1, 2], two["refs"])
    assert VN.last_isolation() == dict(refused=0, dropped=1, repeats=0)
    trace.free()
    run.free()
    # outside an isolated run the callback may ask who is there, and may drop nobody
    run = InProcess(ctxs, two, drop=lambda run, rnd, slots: run.notes.append(pytest.raises(vpin_amd.VpinError, VN.round_drop_images, [0], ECOMM, "x").value.code))
    trace = run.run(ctxs[0], "infer_multi")
    assert run.notes == [EINVAL, EINVAL] and run.seen == [(0, [0, 1, 2]), (1, [0, 1, 2])]
    trace.free()
    run.free()


@pytest.mark.timeout(120)
def test_all_images_refused_is_no_image_left_with_every_status_written(ctxs, two):
    import vpin_amd
    run = InProcess(ctxs, two)
    for b in range(3):
        run.c1 = identity_at(run.c1, 8 * b + b)
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_infer_isolated: no image is left") as e:
        run.run(ctxs[0], "infer_isolated")
    assert e.value.code == ESHAPE and run.seen == []
    assert [(s["code"], s["layer"], s["round"]) for s in e.value.statuses] == [(ESHAPE, 0, -1)] * 3
    assert all(X_IS_IDENTITY in s["text"] for s in e.value.statuses)
    run.free()


@pytest.mark.timeout(120)
def test_when_nothing_refuses_the_isolated_run_is_infer_multi_byte_for_byte(ctxs, two):
    runs = [InProcess(ctxs, two), InProcess(ctxs, two)]
    ref = runs[0].run(ctxs[0], "infer_multi")
    trace, status = runs[1].run(ctxs[0], "infer_isolated")
    assert [s["code"] for s in status] == [OK] * 3 and all(s["text"] == "" for s in status)
    assert trace.images == ref.images == 3 and trace.n_layers == ref.n_layers == 2
    for i in range(2):
        assert trace.layer_images(i) == ref.layer_images(i) == [0, 1, 2]
        assert_views_are(views(trace.layer(i)), [views(ref.layer(i))], "layer %d" % i)
    assert_views_are(views(trace.label(), left=False), [views(ref.label(), left=False)], "the label")
    for b in range(3):
        assert ints([runs[1].clients[b].values(r) for r in range(2)]) == ints([runs[0].clients[b].values(r) for r in range(2)])
        assert_slot_is_its_single_run(trace, b, two["refs"][b], runs[1])
    for got, exp in zip(trace.result(), ref.result()):
        for u, v in zip(got, exp):
            assert np.array_equal(u, v)
    assert runs[0].seen == runs[1].seen
    trace.free()
    ref.free()
    for r in runs:
        r.free()


# ---- 4. the small trained network: biased convolutions, pooling, signed FC layers ---------------------------------------------------

@pytest.mark.timeout(240)
def test_the_trained_network_loses_an_all_identity_image_and_a_survivors_label_proves(ctxs):
    from vpin_amd import elgamal as E
    giants = [1 << 14] * 5
    d = dict(BM.trained_inputs(3), sks=IM.TWO_ROUND_SKS)
    d["cfg"] = TM.device_config(d["model"], giants)
    d["base_g"] = E.BaseTable(ctxs[0])
    d["pubs"] = [E.keygen(d["base_g"], sk) for sk in d["sks"]]
    refs = {b: single_run(ctxs[0], d["cfg"], d, d["sks"][b], b, giants) for b in (1, 2)}
    run = InProcess(ctxs, d, giants=giants)
    for i in range(100):  # slot 0: every c1 point the identity
        run.c1 = identity_at(run.c1, i)
    trace, status = run.run(ctxs[0], "infer_isolated")
    assert [s["code"] for s in status] == [ESHAPE, OK, OK] and (status[0]["layer"], status[0]["round"]) == (0, -1)
    assert "layer 0 (convmc): vpin_enc_conv2d_mc_bias: " in status[0]["text"]
    assert all(trace.layer_images(i) == [1, 2] for i in range(5)) and trace.n_layers == 5
    for b in (1, 2):
        assert_slot_is_its_single_run(trace, b, refs[b], run)
        plain = TM.net_plaintext(d["model"], np.array(d["images"][b]).reshape(1, 10, 10))
        assert [r[0] for r in ints([run.clients[b].values(r) for r in range(5)])] == plain[0]
    assert_result_is(trace, [1, 2], refs)
    assert (trace.image_label(2).n_mult, trace.image_label(2).n_add) == (130, 632)
    for g in trace.image_instances(2):
        assert g.is_sat()
        proof = g.snark_prove(SEED_C, SEED_P)
        assert ctxs[0].snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), proof)
        g.free()
    trace.free()
    run.free()
    d["base_g"].free()
    for r in refs.values():
        r["trace"].free()


# ---- the reference's LeNet as a list: channel sums, a repeat and the interleaved plane order in front of the refusing call -----------

@pytest.mark.timeout(240)
def test_the_tiny_lenet_loses_an_image_behind_sums_repeat_and_the_interleaved_order(ctxs):
    """tests/tiny_lenet.py, B = 3 under one key: slot 1 has an all-identity c1, so the first CONV (its planes handed over n1 times,
    interleaved) refuses slot 1's c1 planes alone; slots 0 and 2 are their own vpin_lenet_infer runs, label by label"""
    import tiny_lenet as TL
    from vpin_amd import elgamal as E
    from vpin_amd import lenet as VL
    from vpin_amd import net as VN
    ctx, giants = ctxs[0], [TL.GIANT] * 7
    lcfg = TL.make_cfg(VL)
    cfg = VN.from_lenet(lcfg)
    sk = IM.TWO_ROUND_SKS[1]
    refs = {}
    for b in (0, 2):
        client = VL.Client(ctx, sk, TL.NB, giants, TL.client_r(b))
        scores, rounds, trace = VL.infer(ctx, lcfg, client, TL.image(b), TL.image_r(b), TL.keys(b), TL.bias_r(b))
        client.free()
        refs[b] = dict(scores=scores, rounds=rounds, trace=trace)
    client = VN.Client(ctx, sk, TL.NB, giants, TL.batch_queue([0, 2]))
    c1, c2 = client.encrypt(np.array([v for b in range(3) for row in TL.image(b) for v in row], dtype=np.int64),
                            [r for b in range(3) for r in TL.image_r(b)])
    for i in range(TL.N_PIX):
        c1 = identity_at(c1, TL.N_PIX + i)
    base_g = E.BaseTable(ctx)
    trace, status = VN.infer_isolated(ctx, cfg, base_g.h, [E.keygen(base_g, sk)], [0, 0, 0], c1, c2, [k for b in range(3) for k in TL.keys(b)],
                                      [r for b in range(3) for r in TL.bias_r(b)], client.round_fn, client.user)
    assert [s["code"] for s in status] == [OK, ESHAPE, OK] and (status[1]["layer"], status[1]["round"]) == (0, -1)
    assert "layer 0 (conv): vpin_enc_conv2d: a multiplication operand B'[k] is the identity" in status[1]["text"]
    assert trace.n_layers == 7 and all(trace.layer_images(i) == [0, 2] for i in range(7))
    for b in (0, 2):
        for i, name in enumerate(VL.LABELS):
            got, alone = trace.image_layer(b, i), refs[b]["trace"].label(name)
            assert (got.P, got.oh, got.ow, got.n_mult, got.n_add) == (alone.P, alone.oh, alone.ow, alone.n_mult, alone.n_add), (b, name)
            assert_views_are(views(got), [views(alone)], "slot %d, %s" % (b, name))
    rounds = [client.values(r) for r in range(7)]
    for r in range(7):
        for j in range(2):
            assert np.array_equal(rounds[r][j], np.concatenate([refs[b]["rounds"][r][j] for b in (0, 2)])), "R%d" % (r + 1)
    assert_result_is(trace, [0, 2], refs)
    assert VN.last_isolation() == dict(refused=1, dropped=0, repeats=1)
    trace.free()
    client.free()
    base_g.free()
    for r in refs.values():
        r["trace"].free()


# ---- 7, 8. over the wire: three clients with B_i = (1, 2, 1), the middle one a peer by hand ---------------------------------------------

IMAGES_OF = [(0, 1), (1, 2), (3, 1)]  # per client (first_image, n_images)
BAD_SK = 0x55AA55AA55AA55AA55AA55AA % EL.ORDER


def wire_peer(ctxs, bad, pair, mode):
    """the middle client by hand: HELLO and an INPUT of two images.  "identity": the second image has an identity c1, and the peer
    waits for what the server tells it.  "silent": good ciphertexts, ROUND 0 is read and never answered"""
    ctx, w = ctxs[3], pair.client
    w.send(WM.HELLO, bytes(ctx.e2_pack(*ctx.e2_base_mul(bad.base_g, [BAD_SK])).reshape(-1)), cnt=1)
    c1, c2 = bad.encrypt(np.array(IM.TWO_ROUND_IMAGES[1] + IM.TWO_ROUND_IMAGES[2], dtype=np.int64), EL.splitmix_scalars(0x1630, 16))
    packed = packed_pair(ctx, c1, c2)
    if mode == "identity":
        packed = packed[:32 * 11] + WM.pack(None) + packed[32 * 12:]  # c1 point 3 of its second image
    w.send(WM.INPUT, packed, cnt=16)
    h, p = w.recv()
    if mode == "silent":
        assert (h["type"], h["round"], h["cnt"]) == (WM.ROUND, 0, 8)
        h, p = w.recv()  # says nothing: the server tells it so once its wire's time is up
    return h, p


def serve_three(ctxs, two, mode, isolation):
    """-> (server, the server's result, the three clients' results, the pairs, the good clients)"""
    from vpin_amd import net as VN
    server = VN.Server(ctxs[0], two["cfg"], 4, isolation=isolation)
    pairs = [Pair(), ShortPair() if mode == "silent" else Pair(), Pair()]
    good = {0: VN.Client(ctxs[1], two["sks"][0], NB, [4, 4], two["client_r"][0]), 2: VN.Client(ctxs[2], two["sks"][2], NB, [4, 4], two["client_r"][3])}
    bad = VN.Client(ctxs[3], BAD_SK, NB, [4, 4], EL.splitmix_scalars(0x1631, 64))
    sched = VN.schedule(two["cfg"])
    slot_of = {0: 0, 2: 3}
    client = lambda i: lambda: good[i].run(pairs[i].client, two["images"][slot_of[i]], two["image_r"][slot_of[i]], sched)
    res, got = run_all(lambda: server.serve([p.server for p in pairs], BM.flat(two["keys"]), BM.flat(two["bias_r"])),
                       [client(0), lambda: wire_peer(ctxs, bad, pairs[1], mode), client(2)])
    bad.free()
    return server, res, got, pairs, good, sched


def close_three(server, pairs, good):
    for c in good.values():
        c.free()
    for p in pairs:
        p.close()
    server.free()


def assert_survivors_are_their_single_runs(two, trace, statuses, got, pairs, sched):
    for i, slot in ((0, 0), (2, 3)):
        ref = two["refs"][slot]
        status_is(statuses[i], OK, -1, slot, 1)
        no_exception(got[i])
        scores, rounds = got[i]
        assert ints(rounds) == ints(ref["rounds"]) and [int(a) for a in scores] == [int(a) for a in ref["scores"]]
        assert_slot_is_its_single_run(trace, slot, ref)
        assert_traffic(8, sched, pairs[i].client.stats(), pairs[i].server.stats())
    assert_result_is(trace, [0, 3], two["refs"])


@pytest.mark.timeout(120)
def test_over_the_wire_a_client_whose_image_a_layer_refuses_is_dropped_alone(ctxs, two):
    import vpin_amd
    from vpin_amd import net as VN
    # isolation off: today's contract, everybody gets ERROR and the call returns the layer's code
    server, res, got, pairs, good, sched = serve_three(ctxs, two, "identity", False)
    text = "vpin_net_infer_multi: layer 0 (fcs): " + X_IS_IDENTITY
    assert isinstance(res, vpin_amd.VpinError) and res.code == ESHAPE and text in str(res), res
    for i, (first, n) in enumerate(IMAGES_OF):
        status_is(res.statuses[i], ESHAPE, VN.STAGE_SERVER, first, n, text)
    assert all(isinstance(got[i], vpin_amd.VpinError) and got[i].code == ECOMM for i in (0, 2)), got
    no_exception(got[1])
    assert got[1][0]["type"] == WM.ERROR and got[1][1][:4] == ESHAPE.to_bytes(4, "little", signed=True)
    assert server.stats_isolation() == dict(images_refused=0, images_compacted=0, layer_calls_repeated=0)
    close_three(server, pairs, good)
    # isolation on: the middle client is told the layer's text, the other two finish as if alone in their slots
    server, res, got, pairs, good, sched = serve_three(ctxs, two, "identity", True)
    no_exception(res)
    trace, statuses = res
    text = "vpin_net_infer_isolated: layer 0 (fcs): " + X_IS_IDENTITY
    status_is(statuses[1], ESHAPE, VN.STAGE_LAYER, 1, 2, text)
    no_exception(got[1])
    assert got[1][0]["type"] == WM.ERROR and got[1][1][:4] == ESHAPE.to_bytes(4, "little", signed=True) and text[:60].encode() in got[1][1]
    assert trace.images == 4 and trace.layer_images(0) == [0, 1, 3] and trace.layer_images(1) == [0, 3]
    assert_survivors_are_their_single_runs(two, trace, statuses, got, pairs, sched)
    assert server.stats_isolation() == dict(images_refused=2, images_compacted=0, layer_calls_repeated=1)
    assert server.stats() == dict(calls=1, clients_admitted=3, clients_served=2, images=4, base_tables_built=1)
    trace.free()
    close_three(server, pairs, good)


@pytest.mark.timeout(120)
def test_over_the_wire_a_silent_clients_images_are_compacted_away(ctxs, two):
    from vpin_amd import net as VN
    server, res, got, pairs, good, sched = serve_three(ctxs, two, "silent", True)
    no_exception(res, *got)
    trace, statuses = res
    status_is(statuses[1], ECOMM, 0, 1, 2, "round 0: vpin_wire: timed out after 300 ms waiting for the peer")
    assert got[1][0]["type"] == WM.ERROR
    assert trace.layer_images(0) == [0, 1, 2, 3] and trace.layer_images(1) == [0, 3] and (trace.layer(0).P, trace.layer(1).P) == (8, 4)
    assert_survivors_are_their_single_runs(two, trace, statuses, got, pairs, sched)
    assert server.stats_isolation() == dict(images_refused=0, images_compacted=2, layer_calls_repeated=0)
    trace.free()
    close_three(server, pairs, good)
    # isolation off holds today's contract: the silent client's images stay in every layer call
    server, res, got, pairs, good, sched = serve_three(ctxs, two, "silent", False)
    no_exception(res, *got)
    trace, statuses = res
    status_is(statuses[1], ECOMM, 0, 1, 2, "round 0: vpin_wire: timed out after 300 ms waiting for the peer")
    assert trace.layer_images(1) == [0, 1, 2, 3] and (trace.layer(0).P, trace.layer(1).P) == (8, 8)
    for i, slot in ((0, 0), (2, 3)):
        status_is(statuses[i], OK, -1, slot, 1)
        assert ints(got[i][1]) == ints(two["refs"][slot]["rounds"])
        assert_slot_is_its_single_run(trace, slot, two["refs"][slot])
    assert server.stats_isolation() == dict(images_refused=0, images_compacted=0, layer_calls_repeated=0)
    trace.free()
    close_three(server, pairs, good)
