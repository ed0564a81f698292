#!/usr/bin/env python3
"""sweep_row_min.py -- one row commitment alone, the multi-window walk (VPIN_MSM_ROW_TABLE=0) against the row-table kernels
(VPIN_MSM_ROW_MIN=0), over the provers' table pair of a long stream (16-bit row table beside the 8-bit multi-window table), on a
whole-chip context and on one confined to 8 CUs per XCD (bench.py's layout for the small lanes).  The break-even of
row_table_min_scalars (msm.hip) is read from its output: profiles/r20_row_min_sweep.txt.

Shapes: the Hyrax shape of a polynomial of 2^n scalars (L = 2^(n/2) rows of R = 2^(n - n/2), one blind column), and the derefs
shape (the first 3/4 of the rows, no blind column).  Full-width random scalars.  Per point: the `msm` class of the HIP-event
profile (kernels only; the walk's chunk-sum kernel lies outside it) and the host clock around the whole call (compression and
copies included, the same on both paths), medians over --reps calls after one warm-up call.
usage: python tools/sweep_row_min.py [--lo 14] [--hi 24] [--reps 5] [--ell 26]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Handle:
    def __init__(self, h):
        self.h = h


def cus(per_xcd_from, per_xcd_to):
    return [x + 8 * ((n // 8) + 4 * (n % 8)) for x in range(8) for n in range(per_xcd_from, per_xcd_to)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lo", type=int, default=14)
    ap.add_argument("--hi", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ell", type=int, default=26, help="the SPARK view asked for: R = 2^(ell - ell/2) generators and two more")
    args = ap.parse_args()
    os.environ.setdefault("VPIN_TABLE_SLOT", "128")            # bench.py's settings for a single-GPU run
    os.environ.setdefault("VPIN_SPARK_GENS_BUDGET_GB", "100")
    for k in ("VPIN_MSM_ROW_MIN", "VPIN_MSM_ROW_TABLE", "VPIN_ROW_TABLE_C", "VPIN_ROW_TABLE", "VPIN_MSM_ROW_WIN_CHUNKS"):
        os.environ.pop(k, None)
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_spark_gens_view.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.vpin_gens_layout.argtypes = [C.c_void_p, C.c_void_p]
    L.vpin_gens_row_layout.argtypes = [C.c_void_p, C.c_void_p]
    L.vpin_hyrax_commit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
    rng = np.random.default_rng(20)
    n_max = 1 << args.hi
    Z = rng.integers(0, 2**63, size=(n_max, 4), dtype=np.uint64)
    Z[:, 3] &= np.uint64((1 << 59) - 1)   # below q; as Montgomery images just other uniformly random scalars
    for name, mask in (("whole chip", None), ("8 CUs per XCD", cus(24, 32))):
        ctx = vpin_amd.Context(0, cu_mask=mask)
        gv, Lv, Rv = C.c_void_p(), C.c_size_t(), C.c_size_t()
        t0 = time.perf_counter()
        assert L.vpin_spark_gens_view(ctx.h, args.ell, C.byref(gv), C.byref(Lv), C.byref(Rv)) == 0
        g = Handle(gv)
        lay, row = (C.c_size_t * 6)(), (C.c_size_t * 4)()
        assert L.vpin_gens_layout(gv, lay) == 0 and L.vpin_gens_row_layout(gv, row) == 0
        print(f"## {name}: {ctx.device_props()[0]} CUs; multi-window table c = {lay[0]} W = {lay[1]}, row table c = {row[0]} W = {row[1]} "
              f"over {row[2]} generators ({time.perf_counter() - t0:.1f} s)", flush=True)
        assert row[0], "no row table was built: nothing to compare"
        tZ = ctx.upload(Z)
        print("log2  shape          blind   walk: msm ms  call ms    row table: msm ms  call ms    call ms saved", flush=True)
        for n in range(args.lo, args.hi + 1):
            Ls, Rs = 1 << (n // 2), 1 << (n - n // 2)
            if Rs + 2 > row[2]:
                continue
            sub = ctx.wrap(tZ.device_ptr, Ls * Rs)
            for blind in (True, False):
                rows = Ls if blind else 3 * Ls // 4
                blinds = np.ascontiguousarray(Z[:rows]) if blind else None
                out = np.zeros((rows, 32), dtype=np.uint8)

                def call():
                    assert L.vpin_hyrax_commit_rows(ctx.h, g.h, sub.h, Ls, 0, rows, blinds.ctypes.data_as(C.c_void_p) if blind else None,
                                                    Rs + 1, out.ctypes.data_as(C.c_void_p)) == 0

                res, outs = {}, {}
                for path, kv in (("walk", {"VPIN_MSM_ROW_TABLE": "0"}), ("row", {"VPIN_MSM_ROW_MIN": "0"})):
                    os.environ.update(kv)
                    try:
                        taken0 = ctx.row_table_rows()
                        call()
                        assert (ctx.row_table_rows() - taken0 == rows) == (path == "row"), path
                        walls = []
                        ctx.prof_reset(); ctx.prof_enable(True)
                        for _ in range(args.reps):
                            t0 = time.perf_counter()
                            call()
                            walls.append((time.perf_counter() - t0) * 1e3)
                        st = ctx.prof_read()["msm"]
                        ctx.prof_enable(False)
                    finally:
                        for k in kv:
                            del os.environ[k]
                    res[path] = (st["ms"] / args.reps, statistics.median(walls))
                    outs[path] = out.copy()
                assert np.array_equal(outs["walk"], outs["row"]), "the two paths' bytes differ"
                (wm, ww), (rm, rw) = res["walk"], res["row"]
                print(f"{n:4d}  {rows:5d} x {Rs:5d}  {'yes' if blind else 'no ':5s}  {wm:12.3f} {ww:8.3f}    {rm:17.3f} {rw:8.3f}    "
                      f"{ww - rw:+9.3f} ({100 * (rw - ww) / ww:+.0f} %)", flush=True)
            sub.free()
        tZ.free()
        ctx.close()


if __name__ == "__main__":
    main()
