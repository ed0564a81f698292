"""GPU tests of proofs over the wire (vpin_net_send_proofs, vpin_net_server_send_proofs, vpin_net_verifier_*, vpin_net_client_verify;
net.send_proofs, net.Server.send_proofs, net.Verifier, Client.verify): behind DONE the server proves each client's images and the
client verifies them on its own context under a computation commitment it derived itself.  The networks are the suite's smallest:
the small trained network of test_gpu_net_wire.py (its label is 130 multiplications and 632 additions), the one-layer network of
test_gpu_net_multi.py with three clients of B_i = (1, 2, 1), the tiny LeNet list of test_gpu_net_lenet.py for per-layer labels
and the two-round network of test_gpu_net_isolate.py with isolation on.  Every proof's seeds are derived here with hashlib, so a
record's bytes are compared with what the prover gives for the same instance and seeds.  2^16 baby steps throughout."""
import hashlib
import threading

import numpy as np
import pytest

import fcs_model as TM
import tiny_lenet as TL
from test_gpu_net_isolate import close_three, serve_three, two  # noqa: F401  (`two` is a fixture)
from test_gpu_net_multi import IMAGES_OF, SKS, no_exception, run_all, small_inputs, status_is
from test_gpu_net_wire import GIANTS, NB, SK, Pair, both, inputs, small_model
from test_proof_wire_model import SIZES

pytestmark = pytest.mark.gpu

OK, ESHAPE, EVERIFY, ECOMM = 0, -5, -6, -7
MASTER = bytes((7 * i + 1) % 256 for i in range(64))
SEED32 = bytes((5 * i + 2) % 256 for i in range(32))


def seeds(slot, label, is_mult):
    """seed_commit, seed_proof of one proof, as include/vpin_hip.h words them"""
    d = hashlib.shake_256(MASTER + b"vPIN/wire-proof" + slot.to_bytes(4, "little") + label.to_bytes(4, "little") + bytes([is_mult])).digest(128)
    return d[:64], d[64:]


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and one per client"""
    import vpin_amd
    out = [vpin_amd.Context(0) for _ in range(4)]
    yield out
    for c in reversed(out):
        c.close()


def read_records(wire):
    """the records up to END by hand -> ([(header, parts)], END's header)"""
    from vpin_amd import wire as W
    out = []
    while True:
        h, p = wire.recv_proof()
        if h["kind"] != W.PROOF:
            return out, h
        out.append((h, W.split_proof_payload(h, p)))


def assert_record_is_the_provers(rec, inst, slot, image, label, is_mult):
    """a record read by hand against the prover on the same instance with the seeds of (slot, label, is_mult)"""
    h, parts = rec
    want = inst.snark_prove(*seeds(slot, label, is_mult))
    n_ops = h["n_ops"]
    assert h == dict(kind=1, is_mult=is_mult, image=image, label=label, n_ops=n_ops, proof_len=len(want["proof"]), comm_len=len(want["comm"]))
    assert parts["proof"] == want["proof"] and parts["comm"] == want["comm"]
    assert parts["comm_para"] == bytes(want["comm_para"].reshape(-1)) and parts["comm_input"] == bytes(want["comm_input"].reshape(-1))


def record_bytes(records):
    return sum(40 + sum(len(v) for v in parts.values()) for _, parts in records)


# ---- 1, 2, 6: one client on the small trained network ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def honest(ctxs):
    """serve, send_proofs; Client.run, Client.verify -- and the same proofs sent once more and read by hand, record by record"""
    from vpin_amd import net as VN
    d = inputs()
    cfg = TM.device_config(d["model"], GIANTS)
    expect = VN.proof_expectation(cfg)
    assert expect == [(0, 1, 130), (0, 0, 632)]
    client = VN.Client(ctxs[1], SK, NB, GIANTS, d["client_r"])
    verifier = VN.Verifier(ctxs[1])
    pair = Pair()
    out = {}

    def server():
        trace = VN.serve(ctxs[0], cfg, pair.server, d["keys"], d["bias_r"])
        out["ms"] = VN.send_proofs(ctxs[0], trace, pair.server, master_seed=MASTER)
        VN.send_proofs(ctxs[0], trace, pair.server, master_seed=MASTER)
        return trace

    def peer():
        client.run(pair.client, d["image"], d["image_r"], VN.schedule(cfg))
        out["before"] = pair.client.stats()
        out["ok"] = client.verify(pair.client, verifier, 1, expect, SEED32)
        out["after"], out["stats"], out["timings"] = pair.client.stats(), verifier.stats(), verifier.timings()
        return read_records(pair.client)

    trace, res = both(server, peer)
    no_exception(trace, res)
    yield dict(out, cfg=cfg, expect=expect, trace=trace, records=res[0], end=res[1], verifier=verifier, client=client, pair=pair)
    trace.free()
    verifier.free()
    client.free()
    pair.close()


@pytest.mark.timeout(240)
def test_one_client_gets_the_proofs_of_its_image_and_verifies_them(ctxs, honest):
    h = honest
    assert h["ok"] == [[True, True]] and h["verifier"].last_text == ""
    assert h["stats"] == dict(shapes_derived=2, lookups=0, accepted=2, rejected=0)
    assert len(h["records"]) == 2 and h["end"] == dict(kind=2, is_mult=0, image=2, label=0, n_ops=0, proof_len=0, comm_len=0)
    insts = h["trace"].image_instances(0)
    for k, (is_mult, n_ops) in enumerate(((1, 130), (0, 632))):
        assert h["records"][k][0]["n_ops"] == n_ops
        assert_record_is_the_provers(h["records"][k], insts[k], 0, 0, 0, is_mult)
        insts[k].free()
    # on the wire: 40 bytes per record and the lengths; the second sending is byte for byte the first
    got = {k: h["after"][k] - h["before"][k] for k in h["after"]}
    assert got == dict(bytes_sent=0, bytes_received=record_bytes(h["records"]) + 40, frames_sent=0, frames_received=3)
    assert all(v >= 0.0 for v in h["ms"].values()) and h["ms"]["prove"] > 0.0
    t = h["timings"]
    assert t["recv"] > 0.0 and t["derive"] > 0.0 and t["verify"] > 0.0


@pytest.mark.timeout(240)
def test_the_derived_commitment_is_the_provers(ctxs, honest):
    """the client-side derivation stands on this equality: A, B, C depend on (is_mult, n_ops) alone, not on the witness"""
    from vpin_amd import capi, gadgets
    from vpin_amd import net as VN
    L = capi.lib()
    v = VN.Verifier(ctxs[2])

    def assert_shape_is(inst, is_mult, n_ops):
        decomm, comm = inst.spark_encode()
        decomm.free()
        got_comm, got_inputs = v.shape(is_mult, n_ops)
        assert got_comm == comm, "the commitment of %d %s" % (n_ops, "multiplications" if is_mult else "additions")
        assert got_inputs.shape == (inst.num_inputs, 4) == (is_mult, 4) and np.array_equal(got_inputs, inst.inputs)
        sizes = (int(L.vpin_dev_instance_comm_bytes(inst.h)), int(L.vpin_dev_instance_proof_max_bytes(inst.h)))
        assert sizes == (int(L.vpin_gadget_comm_bytes(is_mult, n_ops)), int(L.vpin_gadget_proof_max_bytes(is_mult, n_ops)))
        if (is_mult, n_ops) in SIZES:  # the literals of tests/test_proof_wire_model.py are the device instances' own
            assert sizes + (1 << ((inst.num_vars.bit_length() - 1) // 2),) == SIZES[is_mult, n_ops]
        inst.free()

    gm, ga = honest["trace"].image_instances(0)
    assert_shape_is(gm, 1, 130)
    assert_shape_is(ga, 0, 632)
    assert v.stats() == dict(shapes_derived=2, lookups=0, accepted=0, rejected=0)
    for is_mult, n_ops in ((1, 130), (0, 632)):  # a second request is a lookup, and the records' comm is this one
        assert v.shape(is_mult, n_ops)[0] == honest["records"][1 - is_mult][1]["comm"] == honest["verifier"].shape(is_mult, n_ops)[0]
    assert v.stats() == dict(shapes_derived=2, lookups=2, accepted=0, rejected=0)
    # the one-layer network's count: its pooling adds, and multiplies nothing
    cfg = TM.device_config(small_model(), [4])
    assert VN.proof_expectation(cfg) == [(0, 0, 12)] and VN.proof_expectation(cfg, per_layer=True) == [(1, 0, 12)]
    client = VN.Client(ctxs[2], SKS[0], NB, [4], small_inputs(0)[2])
    _, _, trace = VN.infer(ctxs[2], cfg, client, small_inputs(0)[0], small_inputs(0)[1], [], [])
    gm, ga = trace.instances()
    assert gm is None
    assert_shape_is(ga, 0, 12)
    trace.free()
    client.free()
    # one multiplication, on other points and another weight than the placeholders
    x, y = gadgets.synthetic_points(0xABCDEF, 1)
    assert_shape_is(ctxs[2].gadget_point_mult_dev([(1 << 127) + 12345], x, y), 1, 1)
    assert v.stats()["shapes_derived"] == 4
    v.free()


def hostile(ctxs, honest, server_fn, expect=None, n_images=1):
    """a server written here against Client.verify on a fresh pair -> (the server's result, the client's, the verifier's stats)"""
    from vpin_amd import net as VN
    pair = Pair()
    v = honest["verifier"]
    before = v.stats()
    server, client = both(lambda: server_fn(pair), lambda: honest["client"].verify(pair.client, v, n_images, expect or honest["expect"], SEED32))
    after = v.stats()
    received = pair.client.stats()["bytes_received"]
    pair.close()
    return server, client, {k: after[k] - before[k] for k in after}, received, VN


def send_record(wire, rec, **change):
    h, parts = rec
    parts = dict(parts, **{k: change.pop(k) for k in list(change) if k in parts})
    f = dict({k: h[k] for k in ("is_mult", "image", "label", "n_ops", "proof_len", "comm_len")}, **change)
    wire.send_proof(1, b"".join(parts[k] for k in ("proof", "comm", "comm_para", "comm_input")), **f)


def raw_header(pair, **f):
    """a header alone, as a server that goes on to write a payload would begin"""
    from vpin_amd import wire as W
    pair.socks[0].sendall(W.proof_header_encode(1, **f))


@pytest.mark.timeout(120)
def test_a_hostile_servers_honest_records_are_accepted(ctxs, honest):
    def server(pair):
        for rec in honest["records"]:
            send_record(pair.server, rec)
        pair.server.send_proof(2, image=2)

    s, ok, did, _, _ = hostile(ctxs, honest, server)
    no_exception(s, ok)
    assert ok == [[True, True]] and did == dict(shapes_derived=0, lookups=2, accepted=2, rejected=0)


@pytest.mark.timeout(120)
def test_one_flipped_bit_of_a_proof_is_everify_and_exactly_that_ok_is_zero(ctxs, honest):
    proof = bytearray(honest["records"][1][1]["proof"])
    proof[len(proof) // 2] ^= 0x10

    def server(pair):
        send_record(pair.server, honest["records"][0])
        send_record(pair.server, honest["records"][1], proof=bytes(proof))
        pair.server.send_proof(2, image=2)

    s, ok, did, _, _ = hostile(ctxs, honest, server)
    no_exception(s, ok)
    assert ok == [[True, False]] and did == dict(shapes_derived=0, lookups=2, accepted=1, rejected=1)
    assert "vpin_net_client_verify: image 0, label 0, additions: the proof is rejected" in honest["verifier"].last_text


@pytest.mark.timeout(120)
def test_the_commitment_of_another_shape_is_rejected_without_verification(ctxs, honest):
    from vpin_amd import net as VN
    other = VN.Verifier(ctxs[2])
    comm131 = other.shape(1, 131)[0]
    other.free()
    mine = honest["records"][0][1]["comm"]
    assert len(comm131) >= len(mine) and comm131[:len(mine)] != mine

    def server(pair):
        send_record(pair.server, honest["records"][0], comm=comm131[:len(mine)])
        send_record(pair.server, honest["records"][1])
        pair.server.send_proof(2, image=2)

    s, ok, did, _, _ = hostile(ctxs, honest, server)
    no_exception(s, ok)
    assert ok == [[False, True]] and did == dict(shapes_derived=0, lookups=2, accepted=1, rejected=1)
    assert "image 0, label 0, multiplications: the server's commitment is not the shape's commitment" in honest["verifier"].last_text


def assert_refused(res, text, received):
    """the client answered VPIN_ESHAPE with `text`, read `received` bytes, and the test's server got an ERROR record saying the same"""
    import vpin_amd
    s, client, did, got, _ = res
    no_exception(s)
    assert isinstance(client, vpin_amd.VpinError) and client.code == ESHAPE and text in str(client), client
    assert s[0]["kind"] == 3 and s[1][:4] == ESHAPE.to_bytes(4, "little", signed=True) and text.encode() in s[1]
    assert did == dict(shapes_derived=0, lookups=0, accepted=0, rejected=0) and got == received


@pytest.mark.timeout(120)
def test_another_n_ops_in_the_header_is_eshape_before_the_payload_is_read(ctxs, honest):
    from vpin_amd import wire as W
    h = honest["records"][0][0]

    def server(pair):
        raw_header(pair, is_mult=1, n_ops=131, proof_len=h["proof_len"], comm_len=W.gadget_sizes(1, 131)["comm"])
        return pair.server.recv_proof()

    assert_refused(hostile(ctxs, honest, server), "vpin_net_client_verify: image 0, label 0: the server proves 131 multiplications, the expectation says 130", 40)


@pytest.mark.timeout(120)
def test_two_records_in_the_other_order_are_eshape(ctxs, honest):
    h = honest["records"][1][0]

    def server(pair):
        raw_header(pair, is_mult=0, n_ops=632, proof_len=h["proof_len"], comm_len=h["comm_len"])
        return pair.server.recv_proof()

    assert_refused(hostile(ctxs, honest, server), "image 0, label 0: the server proves 632 additions, the expectation says 130 multiplications", 40)


@pytest.mark.timeout(120)
def test_end_after_the_first_record_and_a_wrong_count_are_eshape(ctxs, honest):
    def early(pair):
        send_record(pair.server, honest["records"][0])
        pair.server.send_proof(2, image=1)
        return pair.server.recv_proof()

    assert_refused(hostile(ctxs, honest, early), "vpin_net_client_verify: the server ends after 1 of 2 proofs", record_bytes(honest["records"][:1]) + 40)

    def miscounted(pair):
        for rec in honest["records"]:
            send_record(pair.server, rec)
        pair.server.send_proof(2, image=3)
        return pair.server.recv_proof()

    assert_refused(hostile(ctxs, honest, miscounted), "the server's END counts 3 proofs, 2 were sent", record_bytes(honest["records"]) + 40)

    def another_image(pair):
        raw_header(pair, image=1, **{k: honest["records"][0][0][k] for k in ("is_mult", "n_ops", "proof_len", "comm_len")})
        return pair.server.recv_proof()

    assert_refused(hostile(ctxs, honest, another_image), "the server sends image 1, label 0, the expectation says image 0, label 0 comes next", 40)


@pytest.mark.timeout(120)
def test_an_error_record_is_ecomm_with_its_text(ctxs, honest):
    import vpin_amd

    def server(pair):
        send_record(pair.server, honest["records"][0])
        pair.server.send_proof(3, EVERIFY.to_bytes(4, "little", signed=True) + b"the witness does not satisfy the gadget")

    s, client, did, _, _ = hostile(ctxs, honest, server)
    no_exception(s)
    assert isinstance(client, vpin_amd.VpinError) and client.code == ECOMM, client
    assert "vpin_net_client_verify: the peer reported an error (-6): the witness does not satisfy the gadget" in str(client)
    assert did == dict(shapes_derived=0, lookups=0, accepted=0, rejected=0)


# ---- 3, 4: three clients with B_i = (1, 2, 1) on the one-layer network ---------------------------------------------------------------
def three_clients(ctxs, closes=None):
    """Server.serve, then Server.send_proofs twice: every client verifies the first sending and reads the second by hand.  `closes`:
    that client closes its socket after DONE instead, and the server sends only once it has"""
    from vpin_amd import net as VN
    cfg = TM.device_config(small_model(), [4])
    expect = VN.proof_expectation(cfg)
    server = VN.Server(ctxs[0], cfg, 4)
    pairs = [Pair() for _ in range(3)]
    clients = [VN.Client(ctxs[1 + i], SKS[i], NB, [4], small_inputs(i)[2]) for i in range(3)]
    verifiers = [VN.Verifier(ctxs[1 + i]) for i in range(3)]
    closed = threading.Event()
    if closes is None:
        closed.set()

    def serve():
        wires = [p.server for p in pairs]
        trace, statuses = server.serve(wires, [], [])
        assert closed.wait(30)
        first = server.send_proofs(trace, wires, statuses, master_seed=MASTER)
        second = server.send_proofs(trace, wires, first, master_seed=MASTER)
        return trace, statuses, first, second

    def peer(i):
        n = IMAGES_OF[i][1]
        clients[i].run(pairs[i].client, small_inputs(i)[0], small_inputs(i)[1], VN.schedule(cfg, batch=n))
        if i == closes:
            pairs[i].socks[1].close()
            closed.set()
            return None
        ok = clients[i].verify(pairs[i].client, verifiers[i], n, expect, SEED32)
        return ok, read_records(pairs[i].client)

    res, got = run_all(serve, [lambda i=i: peer(i) for i in range(3)])

    def close():
        for x in verifiers + clients:
            x.free()
        for p in pairs:
            p.close()
        server.free()

    return res, got, verifiers, close


def assert_client_has_its_own_proofs(trace, i, got, verifier):
    first, n = IMAGES_OF[i]
    ok, (records, end) = got
    assert ok == [[True]] * n and end["image"] == n == len(records)
    assert verifier.stats() == dict(shapes_derived=1, lookups=n - 1, accepted=n, rejected=0)  # one shape, derived once
    for b in range(n):  # its own images only: `image` counts from its first, the seeds are its slot's
        gm, ga = trace.image_instances(first + b)
        assert gm is None
        assert_record_is_the_provers(records[b], ga, first + b, b, 0, 0)
        ga.free()


@pytest.mark.timeout(180)
def test_three_clients_each_verify_the_proofs_of_their_own_images(ctxs):
    res, got, verifiers, close = three_clients(ctxs)
    no_exception(res, *got)
    trace, statuses, first, second = res
    assert first == statuses == second
    for i, (slot, n) in enumerate(IMAGES_OF):
        status_is(second[i], OK, -1, slot, n)
        assert_client_has_its_own_proofs(trace, i, got[i], verifiers[i])
    assert [h["image"] for h, _ in got[1][1][0]] == [0, 1]
    trace.free()
    close()


@pytest.mark.timeout(180)
def test_a_client_that_closes_after_done_is_ecomm_at_the_proofs_stage_and_the_others_verify(ctxs):
    from vpin_amd import net as VN
    res, got, verifiers, close = three_clients(ctxs, closes=1)
    no_exception(res, *got)
    trace, statuses, first, second = res
    status_is(statuses[1], OK, -1, 1, 2)
    for st in (first, second):
        status_is(st[1], ECOMM, VN.STAGE_PROOFS, 1, 2, "vpin_net_server_send_proofs: vpin_net_send_proofs: vpin_wire: the peer closed the stream")
    assert VN.STAGE_PROOFS == -5 and got[1] is None
    for i in (0, 2):
        status_is(second[i], OK, -1, *IMAGES_OF[i])
        assert_client_has_its_own_proofs(trace, i, got[i], verifiers[i])
    trace.free()
    close()


# ---- 5: per-layer labels on the tiny LeNet list at B = 2 ---------------------------------------------------------------------------
@pytest.mark.timeout(240)
def test_per_layer_labels_of_the_tiny_lenet_at_two_images(ctxs):
    from vpin_amd import lenet as VL
    from vpin_amd import net as VN
    cfg = VN.from_lenet(TL.make_cfg(VL))
    expect = VN.proof_expectation(cfg, per_layer=True)
    assert expect == [(1 + i, is_mult, n) for i, (m, a) in enumerate(TL.COUNTS["labels"]) for is_mult, n in ((1, m), (0, a)) if n]
    assert sorted({label for label, _, _ in expect}) == [1, 2, 3, 4, 5, 6, 7] and len(expect) == 12
    assert [label for label, is_mult, _ in expect if is_mult] == [1, 3, 5, 6, 7], "the pooling layers are without a multiplication record"
    client = VN.Client(ctxs[1], SKS[0], TL.NB, [TL.GIANT] * 7, TL.batch_queue(range(2)))
    verifier = VN.Verifier(ctxs[1])
    pair = Pair()
    flat = lambda f, n: [v for b in range(n) for v in f(b)]

    def server():
        trace = VN.serve(ctxs[0], cfg, pair.server, flat(TL.keys, 3), flat(TL.bias_r, 3), max_batch=3)
        VN.send_proofs(ctxs[0], trace, pair.server, per_layer=True, master_seed=MASTER)
        return trace

    def peer():
        client.run(pair.client, [v for b in range(2) for row in TL.image(b) for v in row], flat(TL.image_r, 2), VN.schedule(cfg, batch=2))
        before = pair.client.stats()["frames_received"]
        return client.verify(pair.client, verifier, 2, expect, SEED32), pair.client.stats()["frames_received"] - before

    trace, res = both(server, peer)
    no_exception(trace, res)
    # the client takes a record only as the next of its own list: 24 accepted records are those labels, in that order, per image
    assert res == ([[True] * 12] * 2, 25)
    assert verifier.stats() == dict(shapes_derived=len({(m, n) for _, m, n in expect}), lookups=24 - len({(m, n) for _, m, n in expect}), accepted=24, rejected=0)
    trace.free()
    verifier.free()
    client.free()
    pair.close()


# ---- 7: isolation on, one client refused by the first layer ------------------------------------------------------------------------
@pytest.mark.timeout(180)
def test_with_isolation_the_survivors_get_their_proofs_and_the_refused_client_none(ctxs, two):  # noqa: F811
    from vpin_amd import net as VN
    server, res, got, pairs, good, sched = serve_three(ctxs, two, "identity", True)
    no_exception(res)
    trace, statuses = res
    status_is(statuses[1], ESHAPE, VN.STAGE_LAYER, 1, 2, "vpin_net_infer_isolated: layer 0 (fcs)")
    expect = VN.proof_expectation(two["cfg"])
    assert expect == [(0, 1, 24), (0, 0, 32)]
    sent_to_refused = pairs[1].server.stats()
    verifiers = {i: VN.Verifier(ctxs[1 + i // 2]) for i in (0, 2)}
    after, oks = run_all(lambda: server.send_proofs(trace, [p.server for p in pairs], statuses, master_seed=MASTER),
                         [lambda i=i: good[i].verify(pairs[i].client, verifiers[i], 1, expect, SEED32) for i in (0, 2)])
    no_exception(after, *oks)
    assert after == statuses and oks == [[[True, True]], [[True, True]]]
    assert pairs[1].server.stats() == sent_to_refused, "the refused client gets no record"
    for v in verifiers.values():
        assert v.stats() == dict(shapes_derived=2, lookups=0, accepted=2, rejected=0)
        v.free()
    trace.free()
    close_three(server, pairs, good)
