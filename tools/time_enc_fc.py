"""Time per stage of the encrypted fully connected layer and of the encrypted average pooling (vpin_enc_fc,
vpin_enc_fc_signed, vpin_enc_avgpool2d + vpin_conv_trace_instances), warm:
python tools/time_enc_fc.py fc P K N [--runs R] [--prf-bytes B]
python tools/time_enc_fc.py fcs P K N [--runs R] [--prf-bytes B] [--against-fc]   (the same weights with alternating signs)
python tools/time_enc_fc.py pool P H W k stride [--runs R]
Points are vpin_synthetic_points; the weights are 14-bit values (with the default 13-byte PRF the folded weights stay inside
128 bits, as in the reference's LeNet), the pooling scale is 2^10 / k^2.  One cold run, then R warm ones (default 11): per stage
the median, the minimum and the maximum in ms -- validate (upload + range / curve checks, for fc the bias too), layer (fc: the
matrix-vector product, its normalisation and out = C + bias; pool: the accumulators and the scaled outputs), PRF and RLC (fc
only: HMAC-SHA256 on the host team, the left sum), host tail (fc: folded weights, the K multiplications and the chain's prefixes
on the device, the checks and the equation; pool: the second operands of the list), instance build (the vpin_gadget_point_*_dev
calls).
--against-fc prints, for orientation only, vpin_enc_fc_signed and vpin_enc_fc on the SAME non-negative weights, alternating in
one process: the two compute the same trace, so any difference is the signed product kernel's."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpin_amd  # noqa: E402
from vpin_amd import gadgets as G  # noqa: E402


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


kind = sys.argv[1]
pos = []
skip = False
for a in sys.argv[2:]:
    if skip:
        skip = False
    elif a == "--against-fc":
        pass
    elif a.startswith("--"):
        skip = True
    else:
        pos.append(int(a))
runs, prf_bytes = opt("--runs", 11), opt("--prf-bytes", 13)
against_fc = "--against-fc" in sys.argv
if kind in ("fc", "fcs"):
    P, K, N = pos
    x, y = G.synthetic_points(G.SEED + 9, P * (K + N))
    W = [[(2654435761 * (k * N + j + 1) >> 7) % 2**14 for j in range(N)] for k in range(K)]
    Ws = [[w if (k * N + j) % 2 else -w for j, w in enumerate(row)] for k, row in enumerate(W)]
    keys = [bytes((17 * p + i) % 256 for i in range(32)) for p in range(P)]
    args = lambda w: (x[:P * K], y[:P * K], None, P, K, w, N, x[P * K:], y[P * K:], None, keys, prf_bytes)
    call = (lambda ctx: ctx.enc_fc(*args(W))) if kind == "fc" else (lambda ctx: ctx.enc_fc_signed(*args(Ws)))
    head = f"{kind} P={P} K={K} N={N} prf_bytes={prf_bytes}"
    STAGES = ("validate", "layer", "prf", "rlc", "host_tail", "total", "instances")
else:
    assert kind == "pool", "fc P K N | fcs P K N | pool P H W k stride"
    P, H, W_, k, stride = pos
    x, y = G.synthetic_points(G.SEED + 9, P * H * W_)
    call = lambda ctx: ctx.enc_avgpool2d(x, y, None, P, H, W_, k, stride, 2**10 // (k * k))
    head = f"pool P={P} {H}x{W_} k={k} stride={stride}"
    STAGES = ("validate", "layer", "host_tail", "total", "instances")
samples = {s: [] for s in STAGES}
with vpin_amd.Context(0) as ctx:
    for it in range(runs + 1):
        tr = call(ctx)
        tm = ctx.enc_conv_timings()
        tm["layer"] = tm.pop("conv")
        t0 = time.perf_counter()
        insts = tr.instances()
        ctx.sync()
        tm["instances"] = time.perf_counter() - t0
        if it == 0:
            print(f"{head}: outputs {tr.P}x{tr.oh}x{tr.ow}, {tr.n_mult} multiplications, {tr.n_add} additions; "
                  f"cold run {tm['total'] * 1e3:.1f} ms + instances {tm['instances'] * 1e3:.1f} ms")
        else:
            for s in STAGES:
                samples[s].append(tm[s] * 1e3)
        for g in insts:
            if g is not None:
                g.free()
        tr.free()
    if against_fc and kind == "fcs":
        both = {"vpin_enc_fc": {s: [] for s in STAGES[:-1]}, "vpin_enc_fc_signed": {s: [] for s in STAGES[:-1]}}
        for it in range(2 * (runs + 1)):
            name = ("vpin_enc_fc", "vpin_enc_fc_signed")[it % 2]
            tr = (ctx.enc_fc if it % 2 == 0 else ctx.enc_fc_signed)(*args(W))
            tm = ctx.enc_conv_timings()
            tm["layer"] = tm.pop("conv")
            tr.free()
            if it >= 2:
                for s in STAGES[:-1]:
                    both[name][s].append(tm[s] * 1e3)


def report(title, samples, names):
    print(title)
    for s in names:
        v = samples[s]
        print(f"  {s:10s} {statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]")


report(f"warm runs: {runs}; ms per stage: median [min .. max]", samples, STAGES)
if against_fc and kind == "fcs":
    for name, v in both.items():
        report(f"for orientation, {name} on the same non-negative weights, alternating, {runs} warm runs each", v, STAGES[:-1])
