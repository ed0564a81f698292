"""The full-size encrypted LeNet inference on the reference's image and weights (vpin_lenet_infer against the ready-made
client, vpin_amd.lenet):  python tools/time_lenet.py [--reps R] [--nb LOG2] [--no-proofs]
It prints its fixed seeds, checks the scores and every round's values against the plaintext model (tests/lenet_model.py) and the
label counts against the LENET table, and then the median / minimum / maximum in ms over R warm runs (after one warm-up run) of
every label L1 .. L7 and every round R1 .. R7 (the library's host clock, vpin_lenet_last_timings), of the whole inference, and of
the whole inference followed by the 12 proofs of its labels (vpin_snark_prove_dev on the trace's device instances; the two
pooling labels have no multiplication list).  The baby-step table has 2^nb entries (default 24); R6 and R7 get the giant steps
for +-2^39, the other rounds for +-2^35."""
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpin_amd  # noqa: E402
from vpin_amd import gadgets as VG  # noqa: E402
from vpin_amd import lenet as VL  # noqa: E402
import elgamal_model as EL  # noqa: E402
import lenet_model as LM  # noqa: E402


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS, NB_LOG = opt("--reps", 5), opt("--nb", 24)
PROOFS = "--no-proofs" not in sys.argv
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER
SEEDS = dict(image_r=0x1E1, bias_r=0x1E2, client_r=0x1E3, keys="sha256('lenet/key/<i>')")
SEED_C, SEED_P = bytes(range(64)), bytes((11 * i + 5) % 256 for i in range(64))


def stats(xs):
    return "%9.2f %9.2f %9.2f" % (statistics.median(xs), min(xs), max(xs))


def main():
    print("seeds:", SEEDS, "sk: fixed", "nb = 2^%d" % NB_LOG, "reps =", REPS)
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
    image_rs = EL.splitmix_scalars(SEEDS["image_r"], image.size)
    bias_rs = EL.splitmix_scalars(SEEDS["bias_r"], counts["bias_r"])
    client_rs = EL.splitmix_scalars(SEEDS["client_r"], counts["encryptions"] - image.size)
    labels, rounds, whole, proved = [], [], [], []
    for rep in range(REPS + 1):
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


if __name__ == "__main__":
    main()
