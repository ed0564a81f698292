"""The full-size encrypted LeNet inference on the reference's image and weights (vpin_lenet_infer against the ready-made
client, vpin_amd.lenet):  python tools/time_lenet.py [--reps R] [--nb LOG2] [--no-proofs]
It prints its fixed seeds, checks the scores and every round's values against the plaintext model (tests/lenet_model.py) and the
label counts against the LENET table, and then the median / minimum / maximum in ms over R warm runs (after one warm-up run) of
every label L1 .. L7 and every round R1 .. R7 (the library's host clock, vpin_lenet_last_timings), of the whole inference, and of
the whole inference followed by the 12 proofs of its labels (vpin_snark_prove_dev on the trace's device instances; the two
pooling labels have no multiplication list).  The baby-step table has 2^nb entries (default 24); R6 and R7 get the giant steps
for +-2^39, the other rounds for +-2^35.

The same network as a batch (vpin_lenet_as_net through vpin_net_infer_batch; vpin_amd.net.from_lenet, vpin_amd.lenet.infer_batch):
    python tools/time_lenet.py --batch 1,2,4,8 [--reps R] [--nb LOG2] [--wire] [--clients K] [--stages]
    python tools/time_lenet.py --sums
--batch: per B a batch of B images through ONE inference (image b is the reference's image rolled by b % 8 rows and b // 8
columns, under keys and r of its own), every B warmed as a shape of its own by one run and then timed over R = 11 warm runs by default: ms per
inference and per image, and per label L1 .. L7 and round R1 .. R7 the median (minimum .. maximum) of the library's host clock
(vpin_net_last_timings; a label's time holds its channel sums).  The first run of every B is checked against the plaintext model
(tests/lenet_model.py), image by image and round by round.  At B = 1 vpin_lenet_infer itself runs beside the layer list, the two
alternating.  The baby-step table has 2^nb entries (default 24).  No proofs.
--wire: every B also between two endpoints over a socketpair (vpin_net_serve_batch in a thread on a context of its own,
vpin_net_client_run here), the modes alternating.
--clients K: every B that K divides also as K clients of B / K images each, every one with a key and a context of its own, as
threads over socketpairs through ONE inference (vpin_net_serve_multi); K <= 8.
--stages: per B one more pass whose round callback reads the stages of the layer call before it (vpin_enc_conv_last_timings:
validate, the layer's compute, PRF, RLC sums, host tail) and then hands the round to the ready-made client: per label the median
of each stage.  The callback is Python: this pass's rounds and totals are not the figures above.
--sums: the channel-sum stage alone at B = 8: ONE vpin_e2_plane_sums_batch call over the 16 groups against sixteen
vpin_e2_plane_sums calls, for the shapes in front of L3 (6 planes of 14 x 14 by the 16-row table) and L5 (16 planes of 5 x 5, all)."""
import ctypes as C
import hashlib
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
from vpin_amd import capi  # noqa: E402
from vpin_amd import gadgets as VG  # noqa: E402
from vpin_amd import lenet as VL  # noqa: E402
from vpin_amd import net as VN  # noqa: E402
import elgamal_model as EL  # noqa: E402
import lenet_model as LM  # noqa: E402


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


BATCH = [int(b) for b in opt("--batch", "0").split(",")]
REPS, NB_LOG, CLIENTS = int(opt("--reps", 11)), int(opt("--nb", 24)), int(opt("--clients", 0))
WIRE, STAGES, SUMS = "--wire" in sys.argv, "--stages" in sys.argv, "--sums" in sys.argv
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER
SEEDS = dict(image_r=0xDA1, bias_r=0xDA2, client_r=0xDA3, keys="sha256('lenet/batch/<b>/<i>')")
SINGLE_REPS, PROOFS = int(opt("--reps", 5)), "--no-proofs" not in sys.argv
SINGLE_SEEDS = dict(image_r=0x1E1, bias_r=0x1E2, client_r=0x1E3, keys="sha256('lenet/key/<i>')")
SEED_C, SEED_P = bytes(range(64)), bytes((11 * i + 5) % 256 for i in range(64))
STAGE_NAMES = ("validate", "conv", "prf", "rlc", "host_tail")
med = statistics.median
rng = lambda xs: "%9.2f (%8.2f .. %8.2f)" % (med(xs), min(xs), max(xs))


class Conn:
    def __init__(self):
        from vpin_amd import wire as W
        self.a, self.b = socket.socketpair()
        self.ws, self.wc = W.Wire.from_fds(self.a.fileno(), self.a.fileno(), 600000), W.Wire.from_fds(self.b.fileno(), self.b.fileno(), 600000)

    def close(self):
        self.ws.free(); self.wc.free()
        self.a.close(); self.b.close()


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


def staged_round(client, sink):
    """a round callback that notes the stages of the layer call just made and hands the round to the ready-made client"""
    fwd = capi.lib().vpin_net_client_round

    def cb(user, rnd, flags, bits, *rest):
        sink.append(vpin_amd.Context.enc_conv_timings())
        args = [C.c_void_p(p) for p in rest[:6]] + [C.c_size_t(rest[6])] + [C.c_void_p(p) for p in rest[7:]]
        return fwd(C.c_void_p(client.h.value), C.c_int(rnd), C.c_int(flags), C.c_int(bits), *args)

    return capi.LENET_ROUND_FN(cb)


def sums_alone(ctx):
    table = LM.default_config()["connect"]
    for what, n_in, side, connect in (("in front of L3", 6, 14, table), ("in front of L5", 16, 5, [[1] * 16])):
        groups, hw = 16, side * side
        n = groups * n_in * hw
        x, y, inf = VG.synthetic_points(VG.SEED + 0xDB0 + n_in, n) + (np.zeros(n, np.uint8),)
        one, many = [], []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            got = ctx.e2_plane_sums_batch(x, y, inf, groups, n_in, side, side, connect)
            t1 = time.perf_counter()
            per = n_in * hw
            parts = [ctx.e2_plane_sums(x[g * per:(g + 1) * per], y[g * per:(g + 1) * per], inf[g * per:(g + 1) * per], n_in, side, side, connect)
                     for g in range(groups)]
            t2 = time.perf_counter()
            assert all(np.array_equal(got[j][g], parts[g][j]) for g in range(groups) for j in range(3))
            if rep:
                one.append((t1 - t0) * 1e3)
                many.append((t2 - t1) * 1e3)
        print("channel sums %s, B = 8 (16 groups of %d planes of %d x %d -> %d): ms with the Python marshalling, one batched call %s, "
              "sixteen single calls %s, equal bytes" % (what, n_in, side, side, len(connect), rng(one), rng(many)))


def stats(xs):
    return "%9.2f %9.2f %9.2f" % (statistics.median(xs), min(xs), max(xs))


def single_mode():
    print("seeds:", SINGLE_SEEDS, "sk: fixed", "nb = 2^%d" % NB_LOG, "reps =", SINGLE_REPS)
    model = LM.default_config()
    image, w1, b1, w2, b2 = LM.reference_model()
    vs, acts = LM.plaintext(model, image, w1.tolist(), b1.tolist(), w2.tolist(), b2.tolist())
    giants = [max(1, (1 << (39 if r >= 5 else 35)) >> NB_LOG) for r in range(7)]
    ctx = vpin_amd.Context(0)
    cfg = VL.default_config(w1, b1, w2, b2)
    cfg.set_rounds(max_giant=giants)
    counts = cfg.counts()
    assert counts["labels"] == [(VG.CONFIGS[l]["n_mult"], VG.CONFIGS[l]["n_add"]) for l in VG.LENET]
    keys = [hashlib.sha256(b"lenet/key/%d" % i).digest() for i in range(counts["prf_keys"])]
    image_rs = EL.splitmix_scalars(SINGLE_SEEDS["image_r"], image.size)
    bias_rs = EL.splitmix_scalars(SINGLE_SEEDS["bias_r"], counts["bias_r"])
    client_rs = EL.splitmix_scalars(SINGLE_SEEDS["client_r"], counts["encryptions"] - image.size)
    labels, rounds, whole, proved = [], [], [], []
    for rep in range(SINGLE_REPS + 1):
        client = VL.Client(ctx, SK, 1 << NB_LOG, giants, client_rs)
        t0 = time.perf_counter()
        scores, values, trace = VL.infer(ctx, cfg, client, image, image_rs, keys, bias_rs)
        t1 = time.perf_counter()
        if PROOFS:
            for name in VL.LABELS:
                for g in trace.instances(name):
                    if g is not None:
                        g.snark_prove(SEED_C, SEED_P)
                        g.free()
        t2 = time.perf_counter()
        if rep == 0:
            for r in range(7):
                assert [int(a) for a in values[r][0]] == vs[r] and [int(a) for a in values[r][1]] == acts[r], "R%d" % (r + 1)
            for i, name in enumerate(VL.LABELS):
                t = trace.label(name)
                assert (t.n_mult, t.n_add) == counts["labels"][i]
            print("scores:", [int(a) for a in scores], "class", int(np.argmax(scores)), "(the plaintext model's, every round checked)")
        else:
            tm = VL.timings()
            labels.append(tm["labels"])
            rounds.append(tm["rounds"])
            whole.append((t1 - t0) * 1e3)
            proved.append((t2 - t0) * 1e3)
        trace.free()
        client.free()
    print("%-28s %9s %9s %9s" % ("ms, warm", "median", "min", "max"))
    for i in range(7):
        print("%-28s %s" % ("L%d (server)" % (i + 1), stats([l[i] for l in labels])))
        print("%-28s %s" % ("R%d (client, %d values)" % (i + 1, counts["per_round"][i]), stats([r[i] for r in rounds])))
    print("%-28s %s" % ("inference (image encryption in)", stats(whole)))
    if PROOFS:
        print("%-28s %s" % ("inference + 12 proofs", stats(proved)))
    ctx.close()


def batch_mode():
    print("LeNet, seeds:", SEEDS, "sk: fixed", "nb = 2^%d" % NB_LOG, "reps =", REPS)
    full = LM.default_config()
    image, w1, b1, w2, b2 = LM.reference_model()
    lcfg = VL.default_config(w1, b1, w2, b2)
    cfg = VN.from_lenet(lcfg)
    counts, giants = cfg.counts(), cfg.max_giants()
    assert counts["layers"] == lcfg.counts()["labels"] and counts["prf_keys"] == lcfg.counts()["prf_keys"]
    ctx = vpin_amd.Context(0)
    if SUMS:
        sums_alone(ctx)
        ctx.close()
        return
    top, size = max(BATCH), image.size
    images = [np.roll(image, (b % 8, b // 8), axis=(0, 1)) for b in range(top)]
    expect = [LM.plaintext(full, im, w1.tolist(), b1.tolist(), w2.tolist(), b2.tolist()) for im in images]
    assert all(abs(v) < giants[r] << NB_LOG for vs, _ in expect for r in range(7) for v in vs[r]), "an image leaves the client's range"
    k, r_client = counts["prf_keys"], counts["encryptions"] - size
    keys = [[hashlib.sha256(b"lenet/batch/%d/%d" % (b, i)).digest() for i in range(k)] for b in range(top)]
    image_rs = [EL.splitmix_scalars(SEEDS["image_r"] + 0x1000 * b, size) for b in range(top)]
    bias_rs = [EL.splitmix_scalars(SEEDS["bias_r"] + 0x1000 * b, counts["bias_r"]) for b in range(top)]
    client_rs = [EL.splitmix_scalars(SEEDS["client_r"] + 0x1000 * b, r_client) for b in range(top)]

    def queue_of(bs):  # round after round the r of the images bs
        out, pos = [], 0
        for c in counts["per_round"][:-1]:
            for b in bs:
                out += client_rs[b][pos:pos + c]
            pos += c
        return out

    def checked(values, bs, what):
        for r in range(7):
            for i in range(2):
                assert [int(a) for a in values[r][i]] == [v for b in bs for v in expect[b][i][r]], "%s, R%d" % (what, r + 1)

    ctx2 = vpin_amd.Context(0) if WIRE else ctx
    cctx = [vpin_amd.Context(0) for _ in range(CLIENTS)]
    assert CLIENTS <= 8, "at most 8 clients: a context each beside the server's"
    summary = []
    for B in BATCH:
        bs = list(range(B))
        flat = lambda per: [v for one in per[:B] for v in one]
        sched = VN.schedule(cfg, batch=B)
        multi = CLIENTS and B % CLIENTS == 0
        runs = dict(batch=[], lenet=[], wire=[], multi=[])  # per mode and run: (whole ms, the library's timings)
        for rep in range(REPS + 1):
            client = VL.Client(ctx2, SK, 1 << NB_LOG, giants, queue_of(bs))
            t0 = time.perf_counter()
            _, values, trace = VL.infer_batch(ctx, lcfg, client, images[:B], image_rs[:B], keys[:B], bias_rs[:B])
            t1 = time.perf_counter()
            tm = VN.timings(7)
            if rep == 0:
                checked(values, bs, "B = %d" % B)
                assert trace.images == B and all(trace.layer(i).n_add == B * counts["layers"][i][1] for i in range(7)), "every label is one call over the batch"
            else:
                runs["batch"].append(((t1 - t0) * 1e3, tm))
            trace.free()
            client.free()
            if B == 1:  # vpin_lenet_infer itself, alternating with the layer list
                client = VL.Client(ctx2, SK, 1 << NB_LOG, giants, client_rs[0])
                t0 = time.perf_counter()
                _, values, trace = VL.infer(ctx, lcfg, client, images[0], image_rs[0], keys[0], bias_rs[0])
                t1 = time.perf_counter()
                tl = VL.timings()
                if rep == 0:
                    checked(values, [0], "vpin_lenet_infer")
                else:
                    runs["lenet"].append(((t1 - t0) * 1e3, dict(layers=tl["labels"], rounds=tl["rounds"], total=tl["total"])))
                trace.free()
                client.free()
            if WIRE:
                client = VL.Client(ctx2, SK, 1 << NB_LOG, giants, queue_of(bs))
                conn = Conn()
                t0 = time.perf_counter()
                res = threads([lambda: (VN.serve(ctx, cfg, conn.ws, flat(keys), flat(bias_rs), max_batch=None if B == 1 else B), VN.timings(7)),
                               lambda: client.run(conn.wc, np.concatenate([im.reshape(-1) for im in images[:B]]), flat(image_rs), sched)])
                t1 = time.perf_counter()
                res[0][0].free()
                if rep == 0:
                    checked(res[1][1], bs, "B = %d over the wire" % B)
                else:
                    runs["wire"].append(((t1 - t0) * 1e3, res[0][1]))
                client.free()
                conn.close()
            if multi:
                per = B // CLIENTS
                mine = [bs[i * per:(i + 1) * per] for i in range(CLIENTS)]
                server = VN.Server(ctx, cfg, B)
                cl = [VL.Client(cctx[i], (SK + 977 * i) % EL.ORDER, 1 << NB_LOG, giants, queue_of(mine[i])) for i in range(CLIENTS)]
                conns = [Conn() for _ in range(CLIENTS)]
                sched_i = VN.schedule(cfg, batch=per)
                t0 = time.perf_counter()
                res = threads([lambda: (server.serve([c.ws for c in conns], flat(keys), flat(bias_rs)), VN.timings(7))] +
                              [lambda i=i: cl[i].run(conns[i].wc, np.concatenate([images[b].reshape(-1) for b in mine[i]]),
                                                     [r for b in mine[i] for r in image_rs[b]], sched_i) for i in range(CLIENTS)])
                t1 = time.perf_counter()
                (trace, statuses), tmm = res[0]
                assert all(s["code"] == 0 and s["stage"] == VN.STAGE_DONE for s in statuses) and trace.images == B
                if rep == 0:
                    for i in range(CLIENTS):
                        checked(res[1 + i][1], mine[i], "B = %d, client %d of %d" % (B, i, CLIENTS))
                else:
                    runs["multi"].append(((t1 - t0) * 1e3, tmm))
                trace.free()
                for c in cl:
                    c.free()
                for c in conns:
                    c.close()
                server.free()
        names = [("batch", "vpin_net_infer_batch"), ("lenet", "vpin_lenet_infer"), ("wire", "over the wire"), ("multi", "%d clients, serve_multi" % CLIENTS)]
        names = [(key, title) for key, title in names if runs[key]]
        print("B = %d: every round of every image is the plaintext model's; ms, warm, median (min .. max) over %d runs, the modes alternating" % (B, REPS))
        print("%-30s" % "" + "".join(" %-32s" % title for _, title in names) + " %10s" % "per image")
        for i in range(7):
            m, a = counts["layers"][i]
            for kind, label in (("layers", "L%d (%d + %d ops)" % (i + 1, B * m, B * a)), ("rounds", "R%d (%d values)" % (i + 1, sched[i][2]))):
                cols = [[tm[kind][i] for _, tm in runs[key]] for key, _ in names]
                print("%-30s" % label + "".join(" %-32s" % rng(xs) for xs in cols) + " %10.3f" % (med(cols[0]) / B))
        cols = [[w for w, _ in runs[key]] for key, _ in names]
        print("%-30s" % "the whole (encryption in)" + "".join(" %-32s" % rng(xs) for xs in cols) + " %10.3f" % (med(cols[0]) / B))
        first = runs["batch"]
        summary.append((B, med(cols[0]) / B, med([sum(tm["layers"]) for _, tm in first]) / B, med([sum(tm["rounds"]) for _, tm in first]) / B) +
                       tuple(med(c) / B for (key, _), c in zip(names, cols) if key in ("wire", "multi")))
        if STAGES:
            per_label = [[] for _ in range(7)]
            for rep in range(3):
                client = VL.Client(ctx2, SK, 1 << NB_LOG, giants, queue_of(bs))
                sink = []
                c1, c2 = client.encrypt(np.concatenate([im.reshape(-1) for im in images[:B]]).astype(np.int64), flat(image_rs))
                VN.run(ctx, cfg, c1, c2, client.base_g, client.base_h, flat(keys), flat(bias_rs), staged_round(client, sink), batch=None if B == 1 else B).free()
                client.free()
                if rep:
                    for i in range(7):
                        per_label[i].append(sink[i])
            print("B = %d: the stages of every label's layer call, ms, median of 2 warm runs: %s" % (B, ", ".join(STAGE_NAMES)))
            for i in range(7):
                print("L%d" % (i + 1) + "".join(" %10.3f" % (1e3 * med([s[n] for s in per_label[i]])) for n in STAGE_NAMES))
    print("ms per image (medians): the whole inference, the labels, the rounds" + (", then the other modes' whole" if WIRE or CLIENTS else ""))
    for row in summary:
        print("B = %-4d" % row[0] + "".join(" %10.3f" % v for v in row[1:]))
    for c in cctx + ([ctx2] if WIRE else []) + [ctx]:
        c.close()


if __name__ == "__main__":
    batch_mode() if "--batch" in sys.argv or SUMS else single_mode()
