#!/usr/bin/env python3
"""tools/ab_msm_var_bucket.py -- the variable-base MSM two ways on the same scalars and compressed points (run on the GPU box):

  lane    vpin_msm: one lane per term, decompression and double-and-add (msm_var.hip msm_var_kernel)
  bucket  vpin_msm_bucket: signed windows, buckets, running-sum reduction (msm_var.hip bkt_*_kernel)

at n = 2^10 .. 2^17 full-width scalars.  Per size: the minimum and the median wall time of a call (copies of the inputs
included: that is what the batch verifier pays) over --loops calls after --warmup, the two results compared byte for byte.
One text table to stdout: the source of profiles/r07_ab_msm_var_bucket.txt and of kBucketMinTerms in verify.cpp.

  python3 tools/ab_msm_var_bucket.py [--loops 10] [--warmup 3] [--max-log 17]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpin_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-log", type=int, default=10)
    ap.add_argument("--max-log", type=int, default=17)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    print(f"# ab_msm_var_bucket: {time.strftime('%Y-%m-%d %H:%M:%S')}  --loops {a.loops} --warmup {a.warmup}  wall ms per call, min / median")
    print(f"# {'n':>8} {'lane min':>10} {'lane med':>10} {'bucket min':>11} {'bucket med':>11} {'lane/bucket':>12}  bytes")
    with vpin_amd.Context(0) as ctx:
        # points: 2^max-log distinct group elements, multiples of the basepoint, made on the device
        nmax = 1 << a.max_log
        # from the basepoint's encoding by repeated row-wise additions
        seed_pt = np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), dtype=np.uint8)  # RFC 9496 A.1: B
        pts = np.zeros((nmax, 32), dtype=np.uint8)
        pts[0] = seed_pt
        filled = 1
        while filled < nmax:  # doubling: pts[filled + i] = pts[i] + pts[filled - 1]
            take = min(filled, nmax - filled)
            pts[filled:filled + take] = ctx.points_add(pts[:take], np.tile(pts[filled - 1], (take, 1)))
            filled += take
        for lg in range(a.min_log, a.max_log + 1):
            n = 1 << lg
            s = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
            s[:, 3] &= np.uint64((1 << 60) - 1)  # below 2^252 < q: the Montgomery image of some full-width scalar
            res, t = {}, {}
            for name, fn in (("lane", ctx.msm), ("bucket", ctx.msm_bucket)):
                ts = []
                for it in range(a.warmup + a.loops):
                    t0 = time.perf_counter()
                    out = fn(s, pts[:n])
                    if it >= a.warmup:
                        ts.append((time.perf_counter() - t0) * 1e3)
                res[name], t[name] = bytes(out), ts
            same = "same" if res["lane"] == res["bucket"] else "DIFFERENT"
            print(f"  {n:>8} {min(t['lane']):>10.3f} {statistics.median(t['lane']):>10.3f} {min(t['bucket']):>11.3f} "
                  f"{statistics.median(t['bucket']):>11.3f} {min(t['lane']) / min(t['bucket']):>12.2f}  {same}", flush=True)


if __name__ == "__main__":
    main()
