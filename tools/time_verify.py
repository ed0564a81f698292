"""Verification time per instance of a trace (vpin_snark_verify, steady state), and of the whole trace in one batch call:
python tools/time_verify.py [trace] [label-kind] [--batch] [--traces K]
  --batch      also verify the trace's proofs in one vpin_snark_verify_batch call
  --traces K   ... and K copies of the trace's proofs in one call (distinct seeds per call); implies --batch
Prints the per-proof steady times, their sum, the batch time and the ratio.  VPIN_VERIFY_TRACE=1 prints the spans of every
verification on stderr."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpin_amd  # noqa: E402
from vpin_amd import gadgets as G  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = sys.argv[1:]
traces = 0
if "--traces" in flags:
    traces = int(flags[flags.index("--traces") + 1])
    args = [a for a in args if a != flags[flags.index("--traces") + 1]]
batch = "--batch" in flags or traces > 0
trace = args[0] if len(args) > 0 else "lenet"
only = args[1] if len(args) > 1 else None
labels = list(G.LENET) if trace == "lenet" else [trace]
SEED_C, SEED_P = bytes(range(64)), bytes((7 * i + 3) % 256 for i in range(64))
REPEATS = 5  # steady state: the minimum of the passes after the first
total = 0.0
items = []
with vpin_amd.Context(0) as ctx:
    for lab in labels:
        for kind in ("mult", "add"):
            inp = G.synthetic_mult_inputs(lab) if kind == "mult" else G.synthetic_add_inputs(lab)
            if inp is None or (only and f"{lab}-{kind}" != only):
                continue
            g = ctx.gadget_point_mult_dev(*inp) if kind == "mult" else ctx.gadget_point_add_dev(*inp)
            dec, comm = g.spark_encode()
            r = ctx.snark_prove_resident(g.r1cs, dec, g.vars_para, g.vars_input, g.vars, g.inputs, SEED_C, SEED_P)
            meta = {"inputs": np.array(g.inputs, copy=True), "num_inputs": g.num_inputs}
            ts = []
            for it in range(3):
                t0 = time.perf_counter()
                ok = ctx.snark_verify(meta, dict(r, comm=comm))
                ts.append(time.perf_counter() - t0)
                if os.environ.get("VPIN_VERIFY_TRACE"):
                    print(f"-- {lab}-{kind} pass {it}: {ts[-1] * 1e3:.2f} ms", file=sys.stderr)
            print(f"{lab}-{kind}: ok={bool(ok)} first {ts[0] * 1e3:.1f} ms, steady {min(ts[1:]) * 1e3:.1f} ms")
            total += min(ts[1:])
            items.append((meta, dict(r, comm=comm)))
            dec.free()
            g.free()
    print(f"trace {trace}: {total * 1e3:.1f} ms steady")
    if batch:
        # the per-proof path again, as one loop over the trace (what a caller without the batch call runs), in the same session
        loop = []
        for it in range(REPEATS + 1):
            t0 = time.perf_counter()
            oks = [ctx.snark_verify(m, r) for m, r in items]
            loop.append(time.perf_counter() - t0)
        per_proof = min(loop[1:])
        print(f"per-proof loop, {len(items)} calls: ok={all(oks)} steady {per_proof * 1e3:.1f} ms")
        for k in ([1] if not traces else [1, traces]):
            many = items * k
            ts = []
            for it in range(REPEATS + 1):
                seed = bytes([it, k] + [0] * 30)
                t0 = time.perf_counter()
                oks = ctx.snark_verify_batch(many, seed)
                ts.append(time.perf_counter() - t0)
            b = min(ts[1:])
            print(f"batch of {k} trace(s), {len(many)} proofs in one call: ok={all(oks)} first {ts[0] * 1e3:.1f} ms, steady {b * 1e3:.1f} ms"
                  f" = {b / k * 1e3:.1f} ms per trace; per-proof / batch = {per_proof * k / b:.2f}")
