"""The full-size encrypted inference of one of the reference's networks A .. E on its image and weights (vpin_net_infer against
the ready-made client, vpin_amd.net):  python tools/time_net.py A|B|C|D|E|lenet5|lenet5max|resnet [--reps R] [--nb LOG2] [--no-proofs] [--wire]
[--batch 1,2,4,..] [--clients 1,2,4,..] [--isolation] [--refuse 1] [--proofs]
lenet5 is the architecture of the reference's src/accuracy/train_test_lenet5.py (net.lenet5_config: two biased trained convolutions,
three signed fully connected layers) on the same image under seeded signed weights |w| < 2^4 (tests/fcs_model.py); no trained
weights exist here.
lenet5max is lenet5 under the same weights with both average poolings and their rounds removed and max pooling (2, 2) inside the
rounds behind the two convolutions (tests/maxpool_model.py; net.Config.round(maxpool=)): five layers and five rounds instead of
seven and seven; in process, --wire and --batch (the multi-client server does not serve a round that pools).
resnet is a small residual network on the same image under seeded weights of that kind (tests/residual_model.py, built through
net.Config.residual_block): CONVMC 1 -> 8 (3 x 3), a block 8 -> 8, a block 8 -> 16 at stride 2 with the 1 x 1 projection, pooling
over the whole plane, FCS 16 -> 10; its ADD layers (vpin_enc_add) have rounds of their own.
It prints its fixed seeds, checks the scores and every round's values against the plaintext model (tests/net_model.py) and the
label's counts against the model's, and then the median / minimum / maximum in ms over R warm runs (after one warm-up run) of
every layer and every round (the library's host clock, vpin_net_last_timings), of the whole inference, and of the whole
inference followed by the two proofs of its one label (vpin_snark_prove_dev on the trace's device instances).  The baby-step
table has 2^nb entries (default 24).
--wire: the same inference in process and between two endpoints over a socketpair (vpin_net_serve in a thread on a context of
its own, vpin_net_client_run here), the two modes alternating in this one process, R = 11 warm runs by default after one warm-up
pair.  Per round it prints the bytes on the wire each way and the ms of pack, unpack and socket (send and the receive of
payloads), both sides added up (vpin_wire_timings), beside that round's own time in process and over the wire (the server's host
clock: the round as the driver sees it, the client's work and the wire included).
--batch 1,2,4,..: per B a batch of B images through ONE inference (vpin_net_infer_batch; image b is the reference's image rolled by
b % 8 rows and b // 8 columns, under keys and r of its own), every B warmed as a shape of its own by one run and then timed over
R = 11 warm runs by default: ms per inference and per image, and per layer and per round the median (minimum .. maximum).  The
first run of every B is checked against the plaintext model, image by image.  With --wire every B also runs between two endpoints
over a socketpair (vpin_net_serve_batch, vpin_net_client_run), the two modes alternating.  No proofs in this mode.
--clients 1,2,4,..: per K, K clients of one image each, every one with a key and a context of its own, as threads of this one
process over socketpairs (at most 8 clients: 9 contexts), three ways that alternate run by run: (a) ONE inference over all of them
(vpin_net_serve_multi on a vpin_net_server that keeps its table of G), (b) one client with K images through vpin_net_serve_batch,
(c) K times vpin_net_serve, one connection after the other.  Per way the ms per image of the whole exchange (from the first
endpoint's start to the last one's return: the connection's set-up in, the clients' own tables and the server object out) and of
every layer and every round (the server's host clock): median (minimum .. maximum) of R = 11 warm runs by default.  Every client's
values of the first run are checked against the plaintext model.  Then two side timings: vpin_e2_base_create of G and of an H,
and vpin_e2_encrypt_keyed against vpin_e2_encrypt with a ready table at cnt = 236, 944 and 7552.  No proofs in this mode.
--isolation: way (a)'s server with vpin_net_server_set_isolation on (nothing refuses: the cost of the slot bookkeeping alone).
--clients 2,4,.. --refuse 1: what a refusal costs.  Per K two runs of way (a) on an isolating server alternate: all K clients good,
and the LAST client a peer by hand whose c1 points are all the identity, so that the first layer refuses its image, runs again over K - 1
images, and the client is dropped at round 0 while the others finish (their values are checked against the plaintext model).
Printed: the whole exchange and the first layer's time of both, ms per call, median (minimum .. maximum)."""
import os
import socket
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpin_amd  # noqa: E402
from vpin_amd import net as VN  # noqa: E402
import elgamal_model as EL  # noqa: E402
import fcs_model as TM  # noqa: E402
import maxpool_model as MM  # noqa: E402
import net_model as NM  # noqa: E402
import residual_model as RM  # noqa: E402


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


VERSION = sys.argv[1]
WIRE = "--wire" in sys.argv
BATCH = [int(b) for b in sys.argv[sys.argv.index("--batch") + 1].split(",")] if "--batch" in sys.argv else None
CLIENTS = [int(b) for b in sys.argv[sys.argv.index("--clients") + 1].split(",")] if "--clients" in sys.argv else None
WIRE_PROOFS = "--proofs" in sys.argv
REPS, NB_LOG = opt("--reps", 3 if WIRE_PROOFS else 11 if WIRE or BATCH or CLIENTS else 5), opt("--nb", 24)
PROOFS = "--no-proofs" not in sys.argv
ISOLATION, REFUSE = "--isolation" in sys.argv, opt("--refuse", 0)
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER
SEEDS = dict(image_r=0xCA1, bias_r=0xCA2, client_r=0xCA3, keys="sha256('net/key/<i>'), i = 0 ..")
SEED_C, SEED_P = bytes(range(64)), bytes((11 * i + 5) % 256 for i in range(64))
KINDS = {VN.CONV: "conv", VN.POOL: "pool", VN.FC: "fc", VN.CONVMC: "convmc", VN.FCS: "fcs", VN.ADD: "add"}


def stats(xs):
    return "%9.2f %9.2f %9.2f" % (statistics.median(xs), min(xs), max(xs))


def main():
    assert VERSION in VN.VERSIONS + ("lenet5", "lenet5max", "resnet"), "time_net.py A|B|C|D|E|lenet5|lenet5max|resnet"
    print("network", VERSION, "seeds:", SEEDS, "sk: fixed", "nb = 2^%d" % NB_LOG, "reps =", REPS)
    image = NM.reference_image()
    plain = RM.net_plaintext if VERSION == "resnet" else TM.net_plaintext if VERSION == "lenet5" else MM.net_plaintext if VERSION == "lenet5max" else NM.plaintext
    if VERSION == "resnet":
        model = RM.resnet_model_config()
        vs, acts = plain(model, image)
        giant = max(1, (1 << 31) >> NB_LOG)  # the client's range per round: +-2^31
        assert all(abs(v) < giant << NB_LOG for r in vs for v in r), "the shifts do not keep a round inside the client's range"
        cfg = RM.resnet_device_config([giant] * RM.RESNET_ROUNDS, model)
        want = RM.net_counts(model)
    elif VERSION == "lenet5max":
        assert not CLIENTS and not WIRE_PROOFS, "lenet5max: in process, --wire or --batch"
        model = MM.lenet5max_model_config()
        vs, acts = MM.net_plaintext(model, image)
        giant = max(1, (1 << 31) >> NB_LOG)  # the client's range per round: +-2^31
        assert all(abs(v) < giant << NB_LOG for r in vs for v in r), "the shifts do not keep a round inside the client's range"
        cfg = MM.device_config(model, [giant] * 5)
        want = MM.net_counts(model)
    elif VERSION == "lenet5":
        model = TM.lenet5_model_config()
        vs, acts = TM.net_plaintext(model, image)
        giant = max(1, (1 << 31) >> NB_LOG)  # the client's range per round: +-2^31
        assert all(abs(v) < giant << NB_LOG for r in vs for v in r), "the shifts do not keep a round inside the client's range"
        cfg = TM.lenet5_device_config([giant] * 7)
        want = TM.net_counts(model)
    else:
        model = NM.cnn_config(VERSION)
        vs, acts = NM.plaintext(model, image)
        cfg = VN.cnn_config(VERSION, nb_log=NB_LOG)
        want = NM.counts(model)
    ctx = vpin_amd.Context(0)
    counts, giants = cfg.counts(), cfg.max_giants()
    assert counts == dict(want, rounds=len(giants))
    if WIRE_PROOFS:
        assert (WIRE or CLIENTS) and not BATCH and not REFUSE, "--proofs goes with --wire or with --clients"
        proofs_mode(ctx, cfg, model, counts, giants, image, plain)
        ctx.close()
        return
    if BATCH or CLIENTS:
        (refuse_mode if CLIENTS and REFUSE else clients_mode if CLIENTS else batch_mode)(ctx, cfg, model, counts, giants, image, plain)
        ctx.close()
        return
    keys = [NM.net_key(i) for i in range(counts["prf_keys"])]
    if VERSION in ("lenet5", "lenet5max"):  # 2 * 6 + 2 * 16 keys of the two convolutions in front
        fcs = [l for l in model["layers"] if l["kind"] == "fcs"]
        assert all(TM.folded_fit_signed(l["w"], l["N"], keys[44 + 2 * j + i], model["prf_bytes"]) for j, l in enumerate(fcs) for i in range(2))
    elif VERSION == "resnet":  # its one FCS layer is the last: the last two keys
        assert all(TM.folded_fit_signed(model["layers"][-1]["w"], 10, k, model["prf_bytes"]) for k in keys[-2:])
    else:
        assert all(NM.keys_fit(model, keys)), "a folded weight does not fit 128 bits under these keys"
    image_rs = EL.splitmix_scalars(SEEDS["image_r"], image.size)
    bias_rs = EL.splitmix_scalars(SEEDS["bias_r"], counts["bias_r"])
    client_rs = EL.splitmix_scalars(SEEDS["client_r"], counts["encryptions"] - image.size)
    n = len(cfg.layers)
    if WIRE:
        wire_mode(ctx, cfg, counts, giants, image, image_rs, keys, bias_rs, client_rs, vs, acts)
        ctx.close()
        return
    layers, rounds, whole, proved = [], [], [], []
    for rep in range(REPS + 1):
        client = VN.Client(ctx, SK, 1 << NB_LOG, giants, client_rs).set_pools(VN.pool_schedule(cfg))
        t0 = time.perf_counter()
        scores, values, trace = VN.infer(ctx, cfg, client, image, image_rs, keys, bias_rs)
        t1 = time.perf_counter()
        if PROOFS:
            for g in trace.instances():
                if g is not None:
                    g.snark_prove(SEED_C, SEED_P)
                    g.free()
        t2 = time.perf_counter()
        if rep == 0:
            for r in range(len(giants)):
                assert [int(a) for a in values[r][0]] == vs[r] and [int(a) for a in values[r][1]] == acts[r], "round %d" % r
            label = trace.label()
            assert (label.n_mult, label.n_add) == (counts["n_mult"], counts["n_add"])
            print("scores:", [int(a) for a in scores], "class", int(np.argmax(scores)), "(the plaintext model's, every round checked)")
            print("label: %d multiplications, %d additions" % (label.n_mult, label.n_add))
        else:
            tm = VN.timings(n)
            layers.append(tm["layers"])
            rounds.append(tm["rounds"])
            whole.append((t1 - t0) * 1e3)
            proved.append((t2 - t0) * 1e3)
        trace.free()
        client.free()
    print("%-34s %9s %9s %9s" % ("ms, warm", "median", "min", "max"))
    rnd = 0
    for i, l in enumerate(cfg.layers):
        m, a = counts["layers"][i]
        print("%-34s %s" % ("layer %d (%s, %d + %d ops)" % (i, KINDS[l.kind], m, a), stats([x[i] for x in layers])))
        if l.has_round:
            name = "round %d (client, %d values%s)" % (rnd, counts["per_round"][rnd], ", max pooled" if l.round_pool_k else "")
            print("%-34s %s" % (name, stats([x[i] for x in rounds])))
            rnd += 1
    print("%-34s %s" % ("inference (image encryption in)", stats(whole)))
    if PROOFS:
        print("%-34s %s" % ("inference + 2 proofs", stats(proved)))
    ctx.close()


def wire_mode(ctx, cfg, counts, giants, image, image_rs, keys, bias_rs, client_rs, vs, acts):
    from vpin_amd import wire as W
    ctx2 = vpin_amd.Context(0)  # the client's
    sched, n, nr = VN.schedule(cfg), len(cfg.layers), len(giants)
    at = [i for i, l in enumerate(cfg.layers) if l.has_round]  # the layer each round follows
    inproc, wired, whole_in, whole_wire, infer_in, infer_wire = [], [], [], [], [], []
    parts = []  # per run, per slot (0: HELLO and INPUT, 1 + r: round r): pack, unpack, socket ms, both sides added
    stats = None
    for rep in range(REPS + 1):
        client = VN.Client(ctx2, SK, 1 << NB_LOG, giants, client_rs).set_pools(VN.pool_schedule(cfg))
        t0 = time.perf_counter()
        scores, values, trace = VN.infer(ctx, cfg, client, image, image_rs, keys, bias_rs)
        t1 = time.perf_counter()
        tm = VN.timings(n)
        trace.free()
        client.free()
        client = VN.Client(ctx2, SK, 1 << NB_LOG, giants, client_rs).set_pools(VN.pool_schedule(cfg))
        a, b = socket.socketpair()
        ws, wc = W.Wire.from_fds(a.fileno(), a.fileno(), 600000), W.Wire.from_fds(b.fileno(), b.fileno(), 600000)
        out = {}

        def server():
            try:
                tr = VN.serve(ctx, cfg, ws, keys, bias_rs)
                out["tm"] = VN.timings(n)  # this thread's
                tr.free()
            except BaseException as e:  # noqa: BLE001
                out["error"] = e

        th = threading.Thread(target=server)
        t2 = time.perf_counter()
        th.start()
        wscores, wvalues = client.run(wc, image, image_rs, sched)
        th.join()
        t3 = time.perf_counter()
        assert "error" not in out, out.get("error")
        for r in range(nr):
            assert np.array_equal(wvalues[r][0], values[r][0]) and np.array_equal(wvalues[r][1], values[r][1]), "round %d over the wire" % r
        if rep == 0:
            for r in range(nr):
                assert [int(v) for v in values[r][0]] == vs[r] and [int(v) for v in values[r][1]] == acts[r], "round %d" % r
            print("scores:", [int(v) for v in wscores], "class", int(np.argmax(wscores)), "(over the wire; the plaintext model's, every round checked in both modes)")
            stats = (wc.stats(), ws.stats())
        else:
            inproc.append([tm["rounds"][i] for i in at])
            wired.append([out["tm"]["rounds"][i] for i in at])
            whole_in.append((t1 - t0) * 1e3)
            whole_wire.append((t3 - t2) * 1e3)
            infer_in.append(tm["total"])
            infer_wire.append(out["tm"]["total"])
            run = []
            for slot in range(nr + 1):
                s, c = ws.timings(slot), wc.timings(slot)
                run.append((s["pack"] + c["pack"], s["unpack"] + c["unpack"], s["send"] + c["send"] + s["recv"] + c["recv"]))
            parts.append(run)
        ws.free(); wc.free()
        a.close(); b.close()
        client.free()
    med = lambda xs: statistics.median(xs)
    rng = lambda xs: "%8.2f (%7.2f .. %7.2f)" % (med(xs), min(xs), max(xs))
    print("bytes on the wire: client -> server %d in %d frames, server -> client %d in %d frames" %
          (stats[0]["bytes_sent"], stats[0]["frames_sent"], stats[1]["bytes_sent"], stats[1]["frames_sent"]))
    print("ms, warm, median (min .. max) over %d runs, the two modes alternating" % REPS)
    print("%-26s %9s %9s  %-28s %-28s %-28s %-28s %-28s" % ("", "B down", "B up", "round in process", "round over the wire", "pack", "unpack", "socket"))
    col = lambda k, slot: rng([p[slot][k] for p in parts])
    print("%-26s %9d %9d  %-28s %-28s %-28s %-28s %-28s" % ("HELLO and INPUT", 0, 2 * 24 + 32 + 64 * image.size, "", "", col(0, 0), col(1, 0), col(2, 0)))
    replies = [o[0] * o[1] * o[2] for l, (_, _, o) in zip(cfg.layers, VN.shapes(cfg)) if l.has_round]  # the pooled count of a round that pools
    for r, (flags, _, cnt) in enumerate(sched):
        print("%-26s %9d %9d  %-28s %-28s %-28s %-28s %-28s" % (
            "round %d (%d values)" % (r, cnt), 24 + 64 * cnt, 24 + (64 * replies[r] if flags & VN.REENCRYPT else 0), rng([x[r] for x in inproc]),
            rng([x[r] for x in wired]), col(0, 1 + r), col(1, 1 + r), col(2, 1 + r)))
    tot = lambda k: [sum(p[slot][k] for slot in range(nr + 1)) for p in parts]
    print("%-26s %9d %9d  %-28s %-28s %-28s %-28s %-28s" % ("in all", stats[1]["bytes_sent"], stats[0]["bytes_sent"], rng(whole_in), rng(whole_wire),
                                                             rng(tot(0)), rng(tot(1)), rng(tot(2))))
    print("%-26s %9s %9s  %-28s %-28s" % ("vpin_net_infer alone", "", "", rng(infer_in), rng(infer_wire)))
    print("(in all: from the image's encryption to the last value; over the wire it also holds the connection's set-up, the server's two "
          "window tables of G and H built by vpin_e2_base_create, which the run in process takes ready-made from its client)")
    share = [100.0 * (a + b + c) / w for a, b, c, w in zip(tot(0), tot(1), tot(2), whole_wire)]
    print("pack + unpack + socket are %.2f %% of an inference over the wire (median; %.2f .. %.2f); unpack alone %.2f %%" %
          (med(share), min(share), max(share), med([100.0 * b / w for b, w in zip(tot(1), whole_wire)])))
    print("the inference over the wire takes %.3f x the inference in process (medians)" % (med(whole_wire) / med(whole_in)))
    ctx2.close()


def batch_mode(ctx, cfg, model, counts, giants, image, plain):
    from vpin_amd import wire as W
    ctx2 = vpin_amd.Context(0) if WIRE else ctx  # the client's
    n, nr, size = len(cfg.layers), len(giants), image.size
    at = [i for i, l in enumerate(cfg.layers) if l.has_round]
    k, r_bias, r_client = counts["prf_keys"], counts["bias_r"], counts["encryptions"] - size
    top = max(BATCH)
    images = [np.roll(image, (b % 8, b // 8), axis=(0, 1)) for b in range(top)]
    expect = [plain(model, im) for im in images]
    bound = max(g << NB_LOG for g in giants)
    assert all(abs(v) < bound for vs, _ in expect for r in vs for v in r), "an image leaves the client's range"
    keys = [[NM.net_key(k * b + i) for i in range(k)] for b in range(top)]
    image_rs = [EL.splitmix_scalars(SEEDS["image_r"] + 0x1000 * b, size) for b in range(top)]
    bias_rs = [EL.splitmix_scalars(SEEDS["bias_r"] + 0x1000 * b, r_bias) for b in range(top)]
    client_rs = [EL.splitmix_scalars(SEEDS["client_r"] + 0x1000 * b, r_client) for b in range(top)]
    # per image, per round that encrypts again, what it encrypts: the pooled count of a round that pools
    stage = [o[0] * o[1] * o[2] for l, (_, _, o) in zip(cfg.layers, VN.shapes(cfg)) if l.has_round and l.reencrypt]
    med = statistics.median
    rng = lambda xs, d=1: "%9.2f (%8.2f .. %8.2f)" % (med(xs) / d, min(xs) / d, max(xs) / d)
    summary = []
    for B in BATCH:
        queue, pos = [], 0
        for c in stage:  # stage after stage the r of all images
            for b in range(B):
                queue += client_rs[b][pos:pos + c]
            pos += c
        flat = lambda per: [v for one in per[:B] for v in one]
        sched = VN.schedule(cfg, batch=B)
        layers, rounds, whole, wired_rounds, wired_whole = [], [], [], [], []
        for rep in range(REPS + 1):
            client = VN.Client(ctx2, SK, 1 << NB_LOG, giants, queue).set_pools(VN.pool_schedule(cfg))
            t0 = time.perf_counter()
            scores, values, trace = VN.infer_batch(ctx, cfg, client, images[:B], image_rs[:B], keys[:B], bias_rs[:B])
            t1 = time.perf_counter()
            tm = VN.timings(n)
            if rep == 0:
                for r in range(nr):
                    for i in range(2):
                        assert [int(a) for a in values[r][i]] == [v for e in expect[:B] for v in e[i][r]], "B = %d round %d" % (B, r)
                label = trace.label()
                assert (label.n_mult, label.n_add) == (B * counts["n_mult"], B * counts["n_add"]) and trace.images == B
                assert all(trace.layer(i).n_add == B * counts["layers"][i][1] for i in range(n)), "every layer is one call over the batch"
            trace.free()
            client.free()
            if WIRE:
                client = VN.Client(ctx2, SK, 1 << NB_LOG, giants, queue).set_pools(VN.pool_schedule(cfg))
                a, b = socket.socketpair()
                ws, wc = W.Wire.from_fds(a.fileno(), a.fileno(), 600000), W.Wire.from_fds(b.fileno(), b.fileno(), 600000)
                out = {}

                def server():
                    try:
                        tr = VN.serve(ctx, cfg, ws, flat(keys), flat(bias_rs), max_batch=None if B == 1 else B)
                        out["tm"] = VN.timings(n)  # this thread's
                        tr.free()
                    except BaseException as e:  # noqa: BLE001
                        out["error"] = e

                th = threading.Thread(target=server)
                t2 = time.perf_counter()
                th.start()
                _, wvalues = client.run(wc, np.concatenate([im.reshape(-1) for im in images[:B]]), flat(image_rs), sched)
                th.join()
                t3 = time.perf_counter()
                assert "error" not in out, out.get("error")
                for r in range(nr):
                    assert np.array_equal(wvalues[r][0], values[r][0]) and np.array_equal(wvalues[r][1], values[r][1]), "round %d over the wire" % r
                ws.free(); wc.free()
                a.close(); b.close()
                client.free()
            if rep:
                layers.append(tm["layers"])
                rounds.append([tm["rounds"][i] for i in at])
                whole.append((t1 - t0) * 1e3)
                if WIRE:
                    wired_rounds.append([out["tm"]["rounds"][i] for i in at])
                    wired_whole.append((t3 - t2) * 1e3)
        print("B = %d: every round of every image is the plaintext model's; ms, warm, median (min .. max) over %d runs" % (B, REPS))
        print("%-40s %-32s %12s" % ("", "the batch", "per image"))
        rnd = 0
        for i, l in enumerate(cfg.layers):
            m, a = counts["layers"][i]
            xs = [x[i] for x in layers]
            print("%-40s %-32s %12.3f" % ("layer %d (%s, %d + %d ops)" % (i, KINDS[l.kind], B * m, B * a), rng(xs), med(xs) / B))
            if l.has_round:
                xs = [x[rnd] for x in rounds]
                name = "round %d (client, %d values%s)" % (rnd, sched[rnd][2], ", max pooled" if l.round_pool_k else "")
                print("%-40s %-32s %12.3f" % (name, rng(xs), med(xs) / B))
                if WIRE:
                    xs = [x[rnd] for x in wired_rounds]
                    print("%-40s %-32s %12.3f" % ("round %d over the wire" % rnd, rng(xs), med(xs) / B))
                rnd += 1
        print("%-40s %-32s %12.3f" % ("inference (image encryption in)", rng(whole), med(whole) / B))
        if WIRE:
            print("%-40s %-32s %12.3f" % ("inference over the wire (set-up in)", rng(wired_whole), med(wired_whole) / B))
        summary.append((B, med(whole), med([sum(x) for x in layers]), med([sum(x) for x in rounds]), med(wired_whole) if WIRE else 0.0))
    print("ms per image (medians): the whole inference, the layers, the rounds" + (", the whole inference over the wire" if WIRE else ""))
    for B, w, ls, rs, ww in summary:
        print("B = %-4d %10.3f %10.3f %10.3f" % (B, w / B, ls / B, rs / B) + ("%10.3f" % (ww / B) if WIRE else ""))
    if WIRE:
        ctx2.close()


def threads(fns):
    """every fn in a thread of its own -> their results in order; the first exception is raised here"""
    out = [None] * len(fns)

    def body(i):
        try:
            out[i] = fns[i]()
        except BaseException as e:  # noqa: BLE001
            out[i] = e

    ts = [threading.Thread(target=body, args=(i,)) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for o in out:
        if isinstance(o, BaseException):
            raise o
    return out


def clients_mode(ctx, cfg, model, counts, giants, image, plain):
    from vpin_amd import elgamal as E
    from vpin_amd import wire as W
    top = max(CLIENTS)
    assert top <= 8, "at most 8 clients: a context each beside the server's"
    cctx = [vpin_amd.Context(0) for _ in range(top)]
    sks = [(SK + 977 * k) % EL.ORDER for k in range(top)]
    n, nr, size = len(cfg.layers), len(giants), image.size
    at = [i for i, l in enumerate(cfg.layers) if l.has_round]
    k_keys, r_bias, r_client = counts["prf_keys"], counts["bias_r"], counts["encryptions"] - size
    images = [np.roll(image, (b % 8, b // 8), axis=(0, 1)) for b in range(top)]
    expect = [plain(model, im) for im in images]
    bound = max(g << NB_LOG for g in giants)
    assert all(abs(v) < bound for vs, _ in expect for r in vs for v in r), "an image leaves the client's range"
    keys = [[NM.net_key(k_keys * b + i) for i in range(k_keys)] for b in range(top)]
    image_rs = [EL.splitmix_scalars(SEEDS["image_r"] + 0x1000 * b, size) for b in range(top)]
    bias_rs = [EL.splitmix_scalars(SEEDS["bias_r"] + 0x1000 * b, r_bias) for b in range(top)]
    client_rs = [EL.splitmix_scalars(SEEDS["client_r"] + 0x1000 * b, r_client) for b in range(top)]
    stage = [c for c, l in zip(counts["per_round"], [cfg.layers[i] for i in at]) if l.reencrypt]
    sched1 = VN.schedule(cfg)
    med = statistics.median
    rng = lambda xs, d: "%8.2f (%7.2f .. %7.2f)" % (med(xs) / d, min(xs) / d, max(xs) / d)

    class Conn:
        def __init__(self):
            self.a, self.b = socket.socketpair()
            self.ws, self.wc = W.Wire.from_fds(self.a.fileno(), self.a.fileno(), 600000), W.Wire.from_fds(self.b.fileno(), self.b.fileno(), 600000)

        def close(self):
            self.ws.free(); self.wc.free()
            self.a.close(); self.b.close()

    def checked(values, who):  # per client k its rounds
        for k, vals in enumerate(values):
            for r in range(nr):
                for i in range(2):
                    assert [int(a) for a in vals[r][i]] == expect[who[k]][i][r], "client %d round %d" % (who[k], r)

    summary = []
    for K in CLIENTS:
        flat = lambda per: [v for one in per[:K] for v in one]
        queue, pos = [], 0
        for c in stage:  # one client with K images: stage after stage the r of all images
            for b in range(K):
                queue += client_rs[b][pos:pos + c]
            pos += c
        schedK = VN.schedule(cfg, batch=K)
        server = VN.Server(ctx, cfg, K, isolation=ISOLATION)
        ways = {w: dict(whole=[], layers=[], rounds=[]) for w in "abc"}
        for rep in range(REPS + 1):
            # (a) one inference over K clients
            cl = [VN.Client(cctx[k], sks[k], 1 << NB_LOG, giants, client_rs[k]) for k in range(K)]
            conns = [Conn() for _ in range(K)]
            t0 = time.perf_counter()
            res = threads([lambda: (server.serve([c.ws for c in conns], flat(keys), flat(bias_rs)), VN.timings(n))] +
                          [lambda k=k: cl[k].run(conns[k].wc, images[k].reshape(-1), image_rs[k], sched1) for k in range(K)])
            ta = (time.perf_counter() - t0) * 1e3
            (trace, statuses), tma = res[0]
            assert all(s["code"] == 0 and s["stage"] == VN.STAGE_DONE for s in statuses) and trace.images == K
            if rep == 0:
                checked([r[1] for r in res[1:]], list(range(K)))
            trace.free()
            for c in cl + conns:
                c.free() if hasattr(c, "free") else c.close()
            # (b) one client with K images
            client = VN.Client(cctx[0], sks[0], 1 << NB_LOG, giants, queue)
            conn = Conn()
            t0 = time.perf_counter()
            res = threads([lambda: (VN.serve(ctx, cfg, conn.ws, flat(keys), flat(bias_rs), max_batch=None if K == 1 else K), VN.timings(n)),
                           lambda: client.run(conn.wc, np.concatenate([im.reshape(-1) for im in images[:K]]), flat(image_rs), schedK)])
            tb = (time.perf_counter() - t0) * 1e3
            res[0][0].free()
            tmb = res[0][1]
            client.free()
            conn.close()
            # (c) K connections, one after the other
            cl = [VN.Client(cctx[k], sks[k], 1 << NB_LOG, giants, client_rs[k]) for k in range(K)]
            conns = [Conn() for _ in range(K)]
            tmc = dict(layers=[0.0] * n, rounds=[0.0] * n)
            t0 = time.perf_counter()
            for k in range(K):
                res = threads([lambda: (VN.serve(ctx, cfg, conns[k].ws, keys[k], bias_rs[k]), VN.timings(n)),
                               lambda: cl[k].run(conns[k].wc, images[k].reshape(-1), image_rs[k], sched1)])
                res[0][0].free()
                for key in ("layers", "rounds"):
                    tmc[key] = [x + y for x, y in zip(tmc[key], res[0][1][key])]
                if rep == 0:
                    checked([res[1][1]], [k])
            tc = (time.perf_counter() - t0) * 1e3
            for c in cl + conns:
                c.free() if hasattr(c, "free") else c.close()
            if rep:
                for w, whole, tm in (("a", ta, tma), ("b", tb, tmb), ("c", tc, tmc)):
                    ways[w]["whole"].append(whole)
                    ways[w]["layers"].append(tm["layers"])
                    ways[w]["rounds"].append([tm["rounds"][i] for i in at])
        assert server.stats()["base_tables_built"] == 1 and server.stats()["calls"] == REPS + 1
        server.free()
        print("K = %d clients of one image each; ms PER IMAGE, warm, median (min .. max) over %d runs, the three ways alternating" % (K, REPS))
        print("%-34s %-30s %-30s %-30s" % ("", "(a) vpin_net_serve_multi", "(b) one client, serve_batch", "(c) K x vpin_net_serve"))
        rnd = 0
        for i, l in enumerate(cfg.layers):
            print("%-34s %-30s %-30s %-30s" % (("layer %d (%s)" % (i, KINDS[l.kind]),) + tuple(rng([x[i] for x in ways[w]["layers"]], K) for w in "abc")))
            if l.has_round:
                print("%-34s %-30s %-30s %-30s" % (("round %d (%d values per image)" % (rnd, sched1[rnd][2]),) +
                                                   tuple(rng([x[rnd] for x in ways[w]["rounds"]], K) for w in "abc")))
                rnd += 1
        print("%-34s %-30s %-30s %-30s" % (("the whole exchange",) + tuple(rng(ways[w]["whole"], K) for w in "abc")))
        summary.append((K,) + tuple(med(ways[w]["whole"]) / K for w in "abc"))
    print("ms per image (medians) of the whole exchange: (a), (b), (c)")
    for row in summary:
        print("K = %-3d %10.3f %10.3f %10.3f" % row)
    # the side timings: the table builds, and the keyed encryption against the table form
    base_g = E.BaseTable(ctx)
    H = E.keygen(base_g, SK)
    pubs = [E.keygen(base_g, sk) for sk in sks]
    tg, th = [], []
    for rep in range(REPS + 1):
        for xs, point in ((tg, None), (th, H)):
            t0 = time.perf_counter()
            b = E.BaseTable(ctx, point)
            xs.append((time.perf_counter() - t0) * 1e3)
            b.free()
    print("vpin_e2_base_create, ms: of G %s, of an H %s" % (rng(tg[1:], 1), rng(th[1:], 1)))
    base_h = E.BaseTable(ctx, H)
    for cnt in (236, 944, 7552):
        msgs = [int(v) % (1 << 30) - (1 << 29) for v in EL.splitmix_scalars(0xCB1, cnt)]
        rs = EL.splitmix_scalars(0xCB2, cnt)
        key_of = [i * len(pubs) // cnt for i in range(cnt)]  # runs of elements under one key, as the images of a batch
        tt, tk, t1 = [], [], []
        for rep in range(REPS + 1):
            for xs, fn in ((tt, lambda: E.encrypt(base_g, base_h, msgs, rs)), (tk, lambda: E.encrypt_keyed(base_g, pubs, key_of, msgs, rs)),
                           (t1, lambda: E.encrypt_keyed(base_g, [H], [0] * cnt, msgs, rs))):
                t0 = time.perf_counter()
                out = fn()
                xs.append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                ref = E.encrypt(base_g, base_h, msgs, rs)
                assert all(np.array_equal(u, v) for a, b in zip(out, ref) for u, v in zip(a, b)), "keyed under H is the table form"
        print("cnt = %-5d ms (with the Python marshalling): vpin_e2_encrypt with a ready table %s, vpin_e2_encrypt_keyed under %d keys %s, under one key %s" %
              (cnt, rng(tt[1:], 1), len(pubs), rng(tk[1:], 1), rng(t1[1:], 1)))
    base_h.free()
    base_g.free()
    for c in cctx:
        c.close()


def proofs_mode(ctx, cfg, model, counts, giants, image, plain):
    """--wire --proofs (one client through vpin_net_serve and vpin_net_send_proofs) and --clients .. --proofs (K clients through
    vpin_net_serve_multi and vpin_net_server_send_proofs): what the proofs behind DONE cost either side, per image"""
    from vpin_amd import wire as W
    top = max(CLIENTS) if CLIENTS else 1
    assert top <= 8, "at most 8 clients: a context each beside the server's"
    cctx = [vpin_amd.Context(0) for _ in range(top)]
    sks = [(SK + 977 * k) % EL.ORDER for k in range(top)]
    nr, size = len(giants), image.size
    k_keys, r_bias, r_client = counts["prf_keys"], counts["bias_r"], counts["encryptions"] - size
    images = [np.roll(image, (b % 8, b // 8), axis=(0, 1)) for b in range(top)]
    expect_values = [plain(model, im) for im in images]
    keys = [[NM.net_key(k_keys * b + i) for i in range(k_keys)] for b in range(top)]
    image_rs = [EL.splitmix_scalars(SEEDS["image_r"] + 0x1000 * b, size) for b in range(top)]
    bias_rs = [EL.splitmix_scalars(SEEDS["bias_r"] + 0x1000 * b, r_bias) for b in range(top)]
    client_rs = [EL.splitmix_scalars(SEEDS["client_r"] + 0x1000 * b, r_client) for b in range(top)]
    sched, expect = VN.schedule(cfg), VN.proof_expectation(cfg)
    master, seed32 = bytes((7 * i + 1) % 256 for i in range(64)), bytes(range(32))
    print("per image the server proves:", ", ".join("%d %s" % (n, "multiplications" if m else "additions") for _, m, n in expect))
    rng = lambda xs: "%9.2f (%8.2f .. %8.2f)" % (statistics.median(xs), min(xs), max(xs)) if xs else "not measured"
    for K in CLIENTS or [1]:
        flat = lambda per: [v for one in per[:K] for v in one]
        server = VN.Server(ctx, cfg, K) if CLIENTS else None
        verifiers = [VN.Verifier(cctx[k]) for k in range(K)]  # kept across the runs: a returning client
        rows = dict(build=[], prove=[], send=[], server=[], recv=[], verify=[], derive_first=[], derive_again=[], client=[])
        per_image = 0
        for rep in range(REPS + 1):
            cl = [VN.Client(cctx[k], sks[k], 1 << NB_LOG, giants, client_rs[k]) for k in range(K)]
            socks = [socket.socketpair() for _ in range(K)]
            ws = [W.Wire.from_fds(a.fileno(), a.fileno(), 600000) for a, _ in socks]
            wc = [W.Wire.from_fds(b.fileno(), b.fileno(), 600000) for _, b in socks]

            def serve():
                if CLIENTS:
                    trace, statuses = server.serve(ws, flat(keys), flat(bias_rs))
                    t0 = time.perf_counter()
                    after = server.send_proofs(trace, ws, statuses, master_seed=master)
                    assert all(s["code"] == 0 and s["stage"] == VN.STAGE_DONE for s in after)
                    ms = dict(whole=(time.perf_counter() - t0) * 1e3)
                else:
                    trace = VN.serve(ctx, cfg, ws[0], keys[0], bias_rs[0])
                    t0 = time.perf_counter()
                    ms = VN.send_proofs(ctx, trace, ws[0], master_seed=master)
                    ms["whole"] = (time.perf_counter() - t0) * 1e3
                trace.free()
                return ms

            def peer(k):
                _, values = cl[k].run(wc[k], images[k].reshape(-1), image_rs[k], sched)
                before = wc[k].stats()["bytes_received"]
                t0 = time.perf_counter()
                ok = cl[k].verify(wc[k], verifiers[k], 1, expect, seed32)
                whole = (time.perf_counter() - t0) * 1e3
                assert ok == [[True] * len(expect)], verifiers[k].last_text
                return values, verifiers[k].timings(), whole, wc[k].stats()["bytes_received"] - before

            res = threads([serve] + [lambda k=k: peer(k) for k in range(K)])
            if rep == 0:
                for k in range(K):
                    for r in range(nr):
                        for i in range(2):
                            assert [int(a) for a in res[1 + k][0][r][i]] == expect_values[k][i][r], "client %d round %d" % (k, r)
                per_image = res[1][3]
            for key in ("build", "prove", "send"):
                if rep and key in res[0]:
                    rows[key].append(res[0][key])
            if rep:
                rows["server"].append(res[0]["whole"] / K)
            for k in range(K):
                t = res[1 + k][1]
                rows["derive_first" if rep == 0 else "derive_again"].append(t["derive"])
                if rep:
                    rows["recv"].append(t["recv"])
                    rows["verify"].append(t["verify"])
                    rows["client"].append(res[1 + k][2])
            for x in cl + ws + wc:
                x.free()
            for a, b in socks:
                a.close(); b.close()
        stats_v = verifiers[0].stats()
        assert stats_v["shapes_derived"] == len({(m, n) for _, m, n in expect}) and stats_v["rejected"] == 0
        for v in verifiers:
            v.free()
        if server:
            server.free()
        print("K = %d client(s) of one image each; ms PER IMAGE, median (min .. max) over %d warm runs; all %d proofs accepted" %
              (K, REPS, stats_v["accepted"] * K))
        print("  the server: instance build %s, prove %s, send %s; the whole call %s" % (rng(rows["build"]), rng(rows["prove"]), rng(rows["send"]), rng(rows["server"])))
        print("  the client: derive, first call %s, again %s; receive (waits for the prover) %s; verify %s; the whole call %s" %
              (rng(rows["derive_first"]), rng(rows["derive_again"]), rng(rows["recv"]), rng(rows["verify"]), rng(rows["client"])))
        print("  bytes of the records per image: %d (%d records and END)" % (per_image, len(expect)))
    for c in cctx:
        c.close()


def refuse_mode(ctx, cfg, model, counts, giants, image, plain):
    """--clients .. --refuse 1: way (a) on an isolating server, all clients good against the last one refused by the first layer"""
    import wire_model as WM
    from vpin_amd import wire as W
    assert REFUSE == 1 and min(CLIENTS) >= 2 and max(CLIENTS) <= 8, "--refuse 1 with 2 .. 8 clients: somebody has to be left"
    top = max(CLIENTS)
    cctx = [vpin_amd.Context(0) for _ in range(top)]
    sks = [(SK + 977 * k) % EL.ORDER for k in range(top)]
    n, nr, size = len(cfg.layers), len(giants), image.size
    k_keys, r_bias, r_client = counts["prf_keys"], counts["bias_r"], counts["encryptions"] - size
    images = [np.roll(image, (b % 8, b // 8), axis=(0, 1)) for b in range(top)]
    expect = [plain(model, im) for im in images]
    keys = [NM.net_key(k_keys * b + i) for b in range(top) for i in range(k_keys)]
    image_rs = [EL.splitmix_scalars(SEEDS["image_r"] + 0x1000 * b, size) for b in range(top)]
    bias_rs = [r for b in range(top) for r in EL.splitmix_scalars(SEEDS["bias_r"] + 0x1000 * b, r_bias)]
    client_rs = [EL.splitmix_scalars(SEEDS["client_r"] + 0x1000 * b, r_client) for b in range(top)]
    sched1 = VN.schedule(cfg)
    rng = lambda xs: "%9.2f (%8.2f .. %8.2f)" % (statistics.median(xs), min(xs), max(xs))

    def peer(k, client, wire):  # HELLO, an INPUT whose every c1 point is the identity, then whatever the server says
        c = cctx[k]
        wire.send(W.HELLO, bytes(c.e2_pack(*c.e2_base_mul(client.base_g, [sks[k]])).reshape(-1)), cnt=1)
        c1, c2 = client.encrypt(images[k].reshape(-1).astype(np.int64), image_rs[k])
        packed = bytes(c.e2_pack(*[np.concatenate([a, b]) for a, b in zip(c1, c2)]).reshape(-1))
        wire.send(W.INPUT, WM.pack(None) * size + packed[32 * size:], cnt=size)
        return wire.recv()

    for K in CLIENTS:
        server = VN.Server(ctx, cfg, K, isolation=True)
        runs = {w: dict(whole=[], layer0=[]) for w in ("good", "refused")}
        for rep in range(REPS + 1):
            for way in ("good", "refused"):
                cl = [VN.Client(cctx[k], sks[k], 1 << NB_LOG, giants, client_rs[k]) for k in range(K)]
                socks = [socket.socketpair() for _ in range(K)]
                ws = [W.Wire.from_fds(a.fileno(), a.fileno(), 600000) for a, _ in socks]
                wc = [W.Wire.from_fds(b.fileno(), b.fileno(), 600000) for _, b in socks]
                last = (lambda: peer(K - 1, cl[K - 1], wc[K - 1])) if way == "refused" else (
                    lambda: cl[K - 1].run(wc[K - 1], images[K - 1].reshape(-1), image_rs[K - 1], sched1))
                t0 = time.perf_counter()
                res = threads([lambda: (server.serve(ws, keys[:K * k_keys], bias_rs[:K * r_bias]), VN.timings(n))] +
                              [lambda k=k: cl[k].run(wc[k], images[k].reshape(-1), image_rs[k], sched1) for k in range(K - 1)] + [last])
                ms = (time.perf_counter() - t0) * 1e3
                (trace, statuses), tm = res[0]
                good = K - 1 if way == "refused" else K
                assert [s["stage"] for s in statuses] == [VN.STAGE_DONE] * good + [VN.STAGE_LAYER] * (K - good), statuses
                assert trace.layer_images(0) == list(range(good))
                if rep == 0:
                    for k in range(good):
                        for r in range(nr):
                            assert [int(a) for a in res[1 + k][1][r][0]] == expect[k][0][r], "client %d round %d" % (k, r)
                else:
                    runs[way]["whole"].append(ms)
                    runs[way]["layer0"].append(tm["layers"][0])
                trace.free()
                for o in cl + ws + wc:
                    o.free()
                for a, b in socks:
                    a.close(); b.close()
        st = server.stats_isolation()
        assert st == dict(images_refused=REPS + 1, images_compacted=0, layer_calls_repeated=REPS + 1), st
        server.free()
        print("K = %d clients on an isolating server; ms PER CALL, warm, median (min .. max) over %d runs, the two alternating" % (K, REPS))
        print("%-44s %-34s %-34s" % ("", "all K good", "the last one refused at layer 0"))
        print("%-44s %-34s %-34s" % ("layer 0 (with its repeat over K - 1 images)", rng(runs["good"]["layer0"]), rng(runs["refused"]["layer0"])))
        print("%-44s %-34s %-34s" % ("the whole exchange", rng(runs["good"]["whole"]), rng(runs["refused"]["whole"])))
    for c in cctx:
        c.close()


if __name__ == "__main__":
    main()
