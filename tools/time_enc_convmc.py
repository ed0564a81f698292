"""Time per stage of the trained convolution layer (vpin_enc_conv2d_mc + vpin_conv_trace_instances), warm:
python tools/time_enc_convmc.py groups C n_out H W f pad stride [--runs N] [--prf-bytes B] [--bits K] [--plane-sum-route]
                                [--no-instances]   (leave the instance build out: 2 * 120 * 16 * 25 multiplications are a 10 GB witness)
                                [--bias]           (vpin_enc_conv2d_mc_bias under groups * n_out synthetic bias points: the bias
                                                    addition is part of the conv stage)
Pixels are vpin_synthetic_points; the weights are signed pseudo-random values of up to K bits (default 16: the reference's
fixed point), every pair connected, the first weight of every chain non-zero.  One cold run, then N warm ones (default 11): per
stage the median, the minimum and the maximum in ms -- validate (upload + range / curve checks), conv (+ normalisation, outputs
to the host), PRF (HMAC-SHA256 on the host team), RLC (the sums, their negation and normalisation), tail (the chain on the
device, the equation, the lists), instance build (the two vpin_gadget_point_*_dev calls).
--plane-sum-route prints, for orientation only, the existing route over the same planes in the same process: vpin_e2_plane_sums
per group under the all-ones table, then vpin_enc_conv2d over the groups * n_out sums under ONE non-negative filter.  It computes
something simpler (no per-pair filters, no signs, the sums unproven), so no ratio is meaningful."""
import os
import statistics
import sys
import time

import numpy as np

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
    elif a in ("--plane-sum-route", "--no-instances", "--bias"):
        pass
    elif a.startswith("--"):
        skip = True
    else:
        pos.append(int(a))
groups, C, n_out, H, W, f, pad, stride = pos
runs, prf_bytes, bits = opt("--runs", 11), opt("--prf-bytes", 16), opt("--bits", 16)
no_inst, with_bias = "--no-instances" in sys.argv, "--bias" in sys.argv
bx, by = G.synthetic_points(G.SEED + 8, groups * n_out)
rng = np.random.default_rng(0x4D43)
w = rng.integers(-(1 << bits) + 1, 1 << bits, size=(n_out, C, f, f), dtype=np.int64)
w[:, 0, 0, 0] = np.where(w[:, 0, 0, 0] == 0, 1, w[:, 0, 0, 0])
keys = [bytes((17 * p + i) % 256 for i in range(32)) for p in range(groups * n_out)]
x, y = G.synthetic_points(G.SEED + 7, groups * C * H * W)
STAGES = ("validate", "conv", "prf", "rlc", "host_tail", "total", "instances")


def report(samples, names):
    print(f"warm runs: {runs}; ms per stage: median [min .. max]")
    for s in names:
        v = samples[s]
        print(f"  {s:10s} {statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]")


samples = {s: [] for s in STAGES}
with vpin_amd.Context(0) as ctx:
    for it in range(runs + 1):
        if with_bias:
            tr = ctx.enc_conv2d_mc_bias(x, y, None, groups, C, n_out, H, W, w, None, f, f, pad, stride, bx, by, None, keys, prf_bytes)
        else:
            tr = ctx.enc_conv2d_mc(x, y, None, groups, C, n_out, H, W, w, None, f, f, pad, stride, keys, prf_bytes)
        tm = ctx.enc_conv_timings()
        t0 = time.perf_counter()
        gm, ga = (None, None) if no_inst else tr.instances()
        ctx.sync()
        tm["instances"] = time.perf_counter() - t0
        if it == 0:
            print(f"convmc{' + bias' if with_bias else ''} groups={groups} C={C} n_out={n_out} {H}x{W} f={f} pad={pad} stride={stride} prf_bytes={prf_bytes} |w| < 2^{bits}: "
                  f"outputs {tr.P}x{tr.oh}x{tr.ow}, {tr.n_mult} multiplications, {tr.n_add} additions; cold run {tm['total'] * 1e3:.1f} ms "
                  f"+ instances {tm['instances'] * 1e3:.1f} ms")
        else:
            for s in STAGES:
                samples[s].append(tm[s] * 1e3)
        for g in (gm, ga):
            if g is not None:
                g.free()
        tr.free()
    report(samples, STAGES[:-1] if no_inst else STAGES)
    if "--plane-sum-route" in sys.argv:
        filt = [int(abs(v)) or 1 for v in w[0, 0].reshape(-1)]
        table = np.ones((n_out, C), dtype=np.uint8)
        xs, ys = x.reshape(groups, C * H * W, 32), y.reshape(groups, C * H * W, 32)
        route = {"plane_sums": [], "one_filter": [], "total": []}
        for it in range(runs + 1):
            t0 = time.perf_counter()
            sums = [ctx.e2_plane_sums(xs[g], ys[g], None, C, H, W, table) for g in range(groups)]
            t1 = time.perf_counter()
            sx, sy, si = (np.concatenate([s[i] for s in sums]) for i in range(3))
            tr = ctx.enc_conv2d(sx, sy, si, groups * n_out, H, W, filt, f, f, pad, stride, keys, prf_bytes)
            t2 = time.perf_counter()
            if it:
                route["plane_sums"].append((t1 - t0) * 1e3)
                route["one_filter"].append((t2 - t1) * 1e3)
                route["total"].append((t2 - t0) * 1e3)
            else:
                print(f"for orientation, plane sums + one filter over the same planes (all-ones table, filter |w[0][0]|): {tr.n_mult} multiplications, "
                      f"{tr.n_add} additions")
            tr.free()
        report(route, ("plane_sums", "one_filter", "total"))
