"""Time per stage of the encrypted convolution layer (vpin_enc_conv2d + vpin_conv_trace_instances), warm:
python tools/time_enc_conv.py H W f pad stride [--planes P] [--runs N] [--prf-bytes B]
Pixels are vpin_synthetic_points; the filter is the reference's 3 x 3 {1,0,1,2,0,2,1,0,1} or, for other sizes, its pattern of
small weights with zeros.  One cold run, then N warm ones (default 11): per stage the median, the minimum and the maximum in
ms -- validate (upload + range / curve checks), conv (+ normalisation, outputs to the host), PRF (HMAC-SHA256 on the host
team), RLC (the f^2 + 1 sums), host tail (f^2 multiplications, the additions, the equation, the lists), instance build (the two
vpin_gadget_point_*_dev calls)."""
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


pos = []
skip = False
for a in sys.argv[1:]:
    if skip:
        skip = False
    elif a.startswith("--"):
        skip = True
    else:
        pos.append(int(a))
H, W, f, pad, stride = pos
P, runs, prf_bytes = opt("--planes", 2), opt("--runs", 11), opt("--prf-bytes", 16)
filt = [1, 0, 1, 2, 0, 2, 1, 0, 1] if f == 3 else [1 + (k % 2) if k % 8 == 0 else 0 for k in range(f * f)]
keys = [bytes((17 * p + i) % 256 for i in range(32)) for p in range(P)]
x, y = G.synthetic_points(G.SEED + 7, P * H * W)
STAGES = ("validate", "conv", "prf", "rlc", "host_tail", "total", "instances")
samples = {s: [] for s in STAGES}
with vpin_amd.Context(0) as ctx:
    for it in range(runs + 1):
        tr = ctx.enc_conv2d(x, y, None, P, H, W, filt, f, f, pad, stride, keys, prf_bytes)
        tm = ctx.enc_conv_timings()
        t0 = time.perf_counter()
        gm, ga = tr.instances()
        ctx.sync()
        tm["instances"] = time.perf_counter() - t0
        if it == 0:
            print(f"{H}x{W} f={f} pad={pad} stride={stride} planes={P} prf_bytes={prf_bytes}: outputs {tr.oh}x{tr.ow} per plane, "
                  f"{tr.n_mult} multiplications, {tr.n_add} additions; cold run {tm['total'] * 1e3:.1f} ms + instances {tm['instances'] * 1e3:.1f} ms")
        else:
            for s in STAGES:
                samples[s].append(tm[s] * 1e3)
        gm.free()
        if ga is not None:
            ga.free()
        tr.free()
print(f"warm runs: {runs}; ms per stage: median [min .. max]")
for s in STAGES:
    v = samples[s]
    print(f"  {s:10s} {statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]")
