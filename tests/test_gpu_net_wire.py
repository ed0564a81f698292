"""GPU test of the inference between two endpoints over a byte stream (vpin_net_serve, vpin_net_client_run, vpin_wire_round): the
small trained network of test_gpu_net_trained.py (five rounds, 130 multiplications, 632 additions, 2^16 baby steps) with the
server and the client as two threads over a socketpair and two contexts, and as two processes over an AF_UNIX socket, against the
in-process vpin_net_infer on the same key, image, randomness and PRF keys: every layer's output, the label's lists and every
round's (v, act) byte for byte, the scores the plaintext model's, and the bytes on the wire exactly what the schedule implies.
Then the refusals on a one-layer network of two ciphertexts: each ends both sides with an error return, and the same contexts run
the good inference again."""
import multiprocessing as mp
import os
import socket
import sys
import threading

import numpy as np
import pytest

import elgamal_model as EL
import fcs_model as TM
import net_model as NM
import wire_model as WM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 1 << 16
GIANTS = [1 << 14] * 5
SK = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))
WIRE_MS = 10000


def inputs():
    """the inputs of tests/test_gpu_net_trained.py"""
    model = TM.trained_config()
    image = [int(v) for v in TM.trained_image().reshape(-1)]
    counts = TM.net_counts(model)
    return dict(model=model, image=image, counts=counts, image_r=EL.splitmix_scalars(0x7A1, 100),
                bias_r=EL.splitmix_scalars(0x7A2, counts["bias_r"]), client_r=EL.splitmix_scalars(0x7A3, counts["encryptions"] - 100),
                keys=[NM.net_key(300 + i) for i in range(counts["prf_keys"])])


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and the client's"""
    import vpin_amd
    a, b = vpin_amd.Context(0), vpin_amd.Context(0)
    yield a, b
    b.close()
    a.close()


@pytest.fixture(scope="module")
def reference(ctxs):
    """the in-process inference, once"""
    from vpin_amd import net as VN
    d = inputs()
    cfg = TM.device_config(d["model"], GIANTS)
    client = VN.Client(ctxs[0], SK, NB, GIANTS, d["client_r"])
    scores, rounds, trace = VN.infer(ctxs[0], cfg, client, d["image"], d["image_r"], d["keys"], d["bias_r"])
    client.free()
    yield dict(d, cfg=cfg, scores=scores, rounds=rounds, trace=trace)
    trace.free()


def ints(rounds):
    return [([int(a) for a in v], [int(a) for a in act]) for v, act in rounds]


def assert_same_trace(got, ref):
    assert got.n_layers == ref.n_layers
    for i in range(ref.n_layers):
        for u, v in zip(got.layer(i).output(), ref.layer(i).output()):
            assert np.array_equal(u, v), "output of layer %d" % i
    gl, rl = got.label(), ref.label()
    assert (gl.n_mult, gl.n_add) == (rl.n_mult, rl.n_add) == (130, 632)
    assert gl.mults()[0] == rl.mults()[0]
    for u, v in zip(list(gl.mults()[1:]) + list(gl.adds()), list(rl.mults()[1:]) + list(rl.adds())):
        assert np.array_equal(u, v)


def assert_traffic(n_input, sched, client_stats, server_stats):
    frames_up, frames_down = 2 + len(sched), len(sched) + 1  # HELLO, INPUT, a REPLY per round; a ROUND per round, DONE
    up = 24 * frames_up + 64 * (n_input + sum(cnt for flags, _, cnt in sched if flags & 2)) + 32
    down = 24 * frames_down + 64 * sum(cnt for _, _, cnt in sched)
    assert WM.traffic(n_input, sched) == dict(up_bytes=up, up_frames=frames_up, down_bytes=down, down_frames=frames_down)
    assert client_stats == dict(bytes_sent=up, bytes_received=down, frames_sent=frames_up, frames_received=frames_down)
    assert server_stats == dict(bytes_sent=down, bytes_received=up, frames_sent=frames_down, frames_received=frames_up)


class Pair:
    """a socketpair with a Wire on each end"""

    def __init__(self):
        from vpin_amd import wire as W
        self.socks = socket.socketpair()
        self.server = W.Wire.from_fds(self.socks[0].fileno(), self.socks[0].fileno(), WIRE_MS)
        self.client = W.Wire.from_fds(self.socks[1].fileno(), self.socks[1].fileno(), WIRE_MS)

    def close(self):
        self.server.free()
        self.client.free()
        for s in self.socks:
            s.close()


def both(server_fn, client_fn):
    """server_fn in a thread, client_fn here -> (result or exception) of each; neither may hang"""
    out = {}

    def body():
        try:
            out["server"] = server_fn()
        except BaseException as e:  # noqa: BLE001
            out["server"] = e

    t = threading.Thread(target=body)
    t.start()
    try:
        out["client"] = client_fn()
    except BaseException as e:  # noqa: BLE001
        out["client"] = e
    t.join(3 * WIRE_MS / 1000)
    assert not t.is_alive(), "the server's side did not return"
    return out["server"], out["client"]


@pytest.mark.timeout(240)
def test_two_threads_one_socketpair_two_contexts(ctxs, reference):
    from vpin_amd import net as VN
    ref = reference
    sched = VN.schedule(ref["cfg"])
    assert sched == [(3, 28, 128), (2, 17, 32), (3, 20, 27), (3, 21, 4), (0, 0, 3)]
    client = VN.Client(ctxs[1], SK, NB, GIANTS, ref["client_r"])
    pair = Pair()
    trace, res = both(lambda: VN.serve(ctxs[0], ref["cfg"], pair.server, ref["keys"], ref["bias_r"]),
                      lambda: client.run(pair.client, ref["image"], ref["image_r"], sched))
    assert not isinstance(trace, BaseException), trace
    assert not isinstance(res, BaseException), res
    scores, rounds = res
    assert ints(rounds) == ints(ref["rounds"]) and len(rounds) == 5
    vs, acts = TM.net_plaintext(ref["model"], np.array(ref["image"]).reshape(1, 10, 10))
    assert [int(a) for a in scores] == acts[-1] and [r[0] for r in ints(rounds)] == vs
    assert_same_trace(trace, ref["trace"])
    assert_traffic(100, sched, pair.client.stats(), pair.server.stats())
    assert pair.server.timings(5)["unpack"] == 0.0 and pair.server.timings(1)["unpack"] > 0.0  # the last round encrypts nothing
    trace.free()
    client.free()
    pair.close()


def _client_process(path, q):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import vpin_amd
        from vpin_amd import net as VN
        from vpin_amd import wire as W
        d = inputs()
        s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        s.connect(path)
        with vpin_amd.Context(0) as ctx:
            client = VN.Client(ctx, SK, NB, GIANTS, d["client_r"])  # sk lives in this process alone
            wire = W.Wire.from_fds(s.fileno(), s.fileno(), 60000)
            scores, rounds = client.run(wire, d["image"], d["image_r"], VN.schedule(TM.device_config(d["model"], GIANTS)))
            st = wire.stats()
            wire.free()
            client.free()
        s.close()
        q.put(("ok", [int(a) for a in scores], ints(rounds), st))
    except BaseException as e:  # noqa: BLE001
        q.put(("error", repr(e), None, None))


@pytest.mark.timeout(300)
def test_two_processes_one_unix_socket(ctxs, reference, tmp_path):
    from vpin_amd import net as VN
    from vpin_amd import wire as W
    ref = reference
    path = str(tmp_path / "s")
    listener = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    listener.bind(path)
    listener.listen(1)
    listener.settimeout(120)
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    child = mpc.Process(target=_client_process, args=(path, q))
    child.start()
    conn = wire = trace = None
    try:
        conn, _ = listener.accept()
        wire = W.Wire.from_fds(conn.fileno(), conn.fileno(), 60000)
        trace = VN.serve(ctxs[0], ref["cfg"], wire, ref["keys"], ref["bias_r"])
        status, scores, rounds, client_stats = q.get(timeout=120)
        child.join(60)
        assert status == "ok", scores
        vs, acts = TM.net_plaintext(ref["model"], np.array(ref["image"]).reshape(1, 10, 10))
        assert scores == acts[-1], "the client that alone holds sk obtains the plaintext model's scores"
        assert rounds == ints(ref["rounds"])
        assert_same_trace(trace, ref["trace"])
        assert_traffic(100, VN.schedule(ref["cfg"]), client_stats, wire.stats())
        # the server's label from this run, proven and verified
        gm, ga = trace.instances()
        for g in (gm, ga):
            assert g.is_sat()
            got = g.snark_prove(SEED_C, SEED_P)
            assert ctxs[0].snark_verify(dict(inputs=g.inputs, num_inputs=g.num_inputs), got)
            g.free()
    finally:
        if child.is_alive():
            child.terminate()
            child.join(10)
        if trace is not None:
            trace.free()
        if wire is not None:
            wire.free()
        if conn is not None:
            conn.close()
        listener.close()


# ---- refusals, on a one-layer network of two ciphertexts -------------------------------------------------------------------
def small_model(has_round=True):
    """pooling 2 / 2 over 1 x 2 x 4: two outputs, no PRF key, no bias; its round applies ReLU and encrypts again"""
    layer = dict(kind="pool", k=2, stride=2, scale=1)
    if has_round:
        layer["round"] = dict(relu=1, shift_bits=0, reencrypt=True)
    return dict(C=1, H=2, W=4, prf_bytes=13, layers=[layer])


SMALL_IMAGE = [3, -50, 7, 9, 11, 13, 15, -17]
SMALL_R = EL.splitmix_scalars(0x7B1, 8)


@pytest.fixture(scope="module")
def small(ctxs):
    from vpin_amd import net as VN
    cfg = TM.device_config(small_model(), [4])
    client = VN.Client(ctxs[1], SK, NB, [4], EL.splitmix_scalars(0x7B2, 2 * 16))
    yield dict(cfg=cfg, client=client, sched=VN.schedule(cfg))
    client.free()


def good_small_run(ctxs, small):
    """the good inference on the same contexts and client: the plaintext model's values"""
    from vpin_amd import net as VN
    pair = Pair()
    trace, res = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], []),
                      lambda: small["client"].run(pair.client, SMALL_IMAGE, SMALL_R, small["sched"]))
    assert not isinstance(trace, BaseException), trace
    assert not isinstance(res, BaseException), res
    vs, acts = TM.net_plaintext(small_model(), np.array(SMALL_IMAGE).reshape(1, 2, 4))
    assert ints(res[1]) == [(vs[0], acts[0])] and vs[0] == [3 - 50 + 11 + 13, 7 + 9 + 15 - 17] and acts[0] == [0, 14]
    assert_traffic(8, small["sched"], pair.client.stats(), pair.server.stats())
    trace.free()
    pair.close()


@pytest.mark.timeout(60)
def test_the_small_network_runs(ctxs, small):
    assert small["sched"] == [(3, 0, 2)]
    good_small_run(ctxs, small)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("sched, text", [
    ([(3, 1, 2)], "round 0: the server asks for shift_bits 0, the schedule says 1"),
    ([(2, 0, 2)], r"round 0: the server asks for flags 3 \(relu 1, reencrypt 1\), the schedule says 2"),
    ([(3, 0, 3)], "round 0: the server sends 2 ciphertexts, the schedule says 3")], ids=["shift_bits", "relu", "cnt"])
def test_a_schedule_that_differs_is_refused_before_anything_is_decrypted(ctxs, small, sched, text):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    server, client = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], []),
                          lambda: small["client"].run(pair.client, SMALL_IMAGE, SMALL_R, sched))
    assert isinstance(client, vpin_amd.VpinError) and client.code == -5 and __import__("re").search(text, str(client)), client
    assert isinstance(server, vpin_amd.VpinError) and server.code == -7, server
    assert "the peer reported an error (-5)" in str(server) and __import__("re").search(text, str(server)), server
    pair.close()
    good_small_run(ctxs, small)


def hand_written_peer(ctxs, small, wire, answer):
    """a client by hand: HELLO and INPUT as the protocol says, then `answer(round header, payload)` instead of a reply"""
    ctx, client = ctxs[1], small["client"]
    hx, hy, hinf = ctx.e2_base_mul(client.base_g, [SK])
    wire.send(WM.HELLO, bytes(ctx.e2_pack(hx, hy, hinf).reshape(-1)), cnt=1)
    c1, c2 = client.encrypt(np.array(SMALL_IMAGE, dtype=np.int64), SMALL_R)
    both_halves = [np.concatenate([a, b]) for a, b in zip(c1, c2)]
    wire.send(WM.INPUT, bytes(ctx.e2_pack(*both_halves).reshape(-1)), cnt=8)
    if answer is None:
        return None
    h, p = wire.recv()
    assert (h["type"], h["round"], h["flags"], h["shift_bits"], h["cnt"]) == (WM.ROUND, 0, 3, 0, 2)
    answer(h, p)
    return wire.recv()  # what the server says to it


@pytest.mark.timeout(60)
def test_a_reply_with_a_non_square_x_is_einval_naming_the_index(ctxs, small):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    good = WM.pack(WM.G)

    def answer(h, p):
        pair.client.send(WM.REPLY, good + good + good + (5).to_bytes(32, "little"), round_=0, cnt=2)

    server, said = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], []), lambda: hand_written_peer(ctxs, small, pair.client, answer))
    assert isinstance(server, vpin_amd.VpinError) and server.code == -1, server
    assert "round 0" in str(server) and "vpin_e2_unpack: point 3: x is not on the curve E2" in str(server), server
    assert not isinstance(said, BaseException), said
    assert said[0]["type"] == WM.ERROR and said[1][:4] == (-1).to_bytes(4, "little", signed=True) and b"point 3" in said[1]
    pair.close()
    good_small_run(ctxs, small)


@pytest.mark.timeout(60)
def test_a_reply_for_the_wrong_round(ctxs, small):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    good = WM.pack(WM.G)
    server, said = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], []),
                        lambda: hand_written_peer(ctxs, small, pair.client, lambda h, p: pair.client.send(WM.REPLY, good * 4, round_=1, cnt=2)))
    assert isinstance(server, vpin_amd.VpinError) and server.code == -5 and "round 0: the reply is for round 1" in str(server), server
    assert not isinstance(said, BaseException) and said[0]["type"] == WM.ERROR and b"the reply is for round 1" in said[1], said
    pair.close()
    good_small_run(ctxs, small)


@pytest.mark.timeout(60)
def test_a_client_that_closes_after_input(ctxs, small):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()

    def peer():
        hand_written_peer(ctxs, small, pair.client, None)
        pair.socks[1].close()

    server, said = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], []), peer)
    assert not isinstance(said, BaseException), said
    assert isinstance(server, vpin_amd.VpinError) and server.code == -7 and "the peer closed the stream after 0 of 24 bytes" in str(server), server
    pair.close()
    good_small_run(ctxs, small)


@pytest.mark.timeout(60)
def test_a_last_layer_without_a_round_is_einval_before_anything_is_read(ctxs, small):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    cfg = TM.device_config(small_model(has_round=False), [])
    with pytest.raises(vpin_amd.VpinError, match="the last layer has no round") as e:
        VN.serve(ctxs[0], cfg, pair.server, [], [])
    assert e.value.code == -1 and pair.server.stats()["bytes_received"] == 0
    h, p = pair.client.recv()  # both sides end: the client is told
    assert h["type"] == WM.ERROR and b"the last layer has no round" in p
    pair.close()
    good_small_run(ctxs, small)
