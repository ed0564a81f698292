"""Warm timings of the client side on E2 (vpin_e2_base_*, vpin_e2_encrypt, vpin_e2_mul256, vpin_e2_dlog_*, vpin_e2_decrypt):
python tools/time_e2_client.py [--reps R] [--nb LOG2 ...] [--widths W ...]
For cnt in {1024, 4704} (LeNet's image and its largest activation plane set) it prints the median / minimum / maximum in ms,
over R calls after a warm-up call, of
  the table builds          base tables at every width, baby-step tables at every nb (and the device bytes they hold)
  fixed-base multiplication at every width, and the same scalars through the variable-base kernel with the base replicated
  encryption                vpin_e2_encrypt
  sk * c1                   the variable-base kernel with the key replicated
  the walk                  vpin_e2_dlog_solve over values uniform in +-2^35 at every nb, max_giant = 2^35 / nb
  a client round            decrypt cnt, encrypt cnt again, at the default nb
Every timed call ends in a stream synchronise inside the library; the clock is the host's, around the C call alone (the
arrays are prepared before).  The variants of one comparison alternate inside every repetition."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpin_amd  # noqa: E402
from vpin_amd import elgamal as E  # noqa: E402
from vpin_amd.capi import _chk, lib  # noqa: E402


def opt(name, default):
    if name not in sys.argv:
        return default
    out = []
    for a in sys.argv[sys.argv.index(name) + 1:]:
        if a.startswith("--"):
            break
        out.append(int(a))
    return out


REPS = opt("--reps", [7])[0]
NBS = [1 << k for k in opt("--nb", [20, 24, 26])]
WIDTHS = opt("--widths", [4, 6, 8, 10, 12])
COUNTS = (1024, 4704)
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % E.ORDER
RANGE = 1 << 35
p = lambda a: a.ctypes.data_as(C.c_void_p)


def clock(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def report(name, ts):
    print(f"{name:<58s} median {statistics.median(ts):10.3f} ms   min {min(ts):10.3f}   max {max(ts):10.3f}   ({len(ts)} calls)", flush=True)


def alternate(variants):
    """variants: [(name, fn)]; one warm-up call each, then REPS rounds that visit every variant in turn"""
    for _, fn in variants:
        fn()
    ts = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, fn in variants:
            ts[name].append(clock(fn))
    for name, _ in variants:
        report(name, ts[name])
    return {name: statistics.median(v) for name, v in ts.items()}


def scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x07  # below 2^251, so below the group order
    s[:, 0] |= 1
    return s


def outs(n, k=1):
    return [a for _ in range(k) for a in (np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8))]


def main():
    L = lib()
    rng = np.random.default_rng(0xE2C1)
    with vpin_amd.Context(0) as ctx:
        print(f"# reps {REPS}, widths {WIDTHS}, nb {[int(np.log2(v)) for v in NBS]} (log2)")
        print("## table builds")
        bases = {}
        for w in WIDTHS:
            ts = []
            for i in range(REPS + 1):
                h = C.c_void_p()
                t = clock(lambda: _chk(L.vpin_e2_base_create_w(ctx.h, None, None, w, C.byref(h)), "vpin_e2_base_create_w"))
                if i:
                    ts.append(t)
                if i < REPS:
                    L.vpin_e2_base_free(h)
            bases[w] = h
            nwin = (252 + w - 1) // w
            report(f"base table of G, w = {w} ({nwin * (2**w - 1) * 64 / 1e6:.2f} MB)", ts)
        tables = {}
        for nb in NBS:
            ts = []
            for i in range(3):
                h = C.c_void_p()
                t = clock(lambda: _chk(L.vpin_e2_dlog_create(ctx.h, nb, C.byref(h)), "vpin_e2_dlog_create"))
                if i:
                    ts.append(t)
                if i < 2:
                    L.vpin_e2_dlog_free(h)
            tables[nb] = h
            report(f"baby-step table, nb = 2^{int(np.log2(nb))} ({ctx.e2_dlog_info(h)[1] / 1e6:.1f} MB on the device)", ts)

        base_g = ctx.e2_base_create()  # the library's default width
        hx, hy, hinf = ctx.e2_base_mul(base_g, [SK])
        base_h = ctx.e2_base_create(int.from_bytes(bytes(hx[0]), "little"), int.from_bytes(bytes(hy[0]), "little"))
        gx, gy, _ = ctx.e2_base_mul(base_g, [1])

        for cnt in COUNTS:
            print(f"## cnt = {cnt}")
            s = scalars(rng, cnt)
            o = {w: outs(cnt) for w in WIDTHS}
            rx, ry, rinf = np.tile(gx, (cnt, 1)), np.tile(gy, (cnt, 1)), np.zeros(cnt, np.uint8)
            variants = [(f"fixed base, w = {w}", (lambda b, q: lambda: _chk(L.vpin_e2_base_mul(ctx.h, b, p(s), cnt, p(q[0]), p(q[1]), p(q[2])),
                                                                          "vpin_e2_base_mul"))(bases[w], o[w])) for w in WIDTHS]
            o2 = outs(cnt)
            variants.append(("variable base (252-bit double-and-add), G replicated",
                             lambda: _chk(L.vpin_e2_mul256(ctx.h, p(s), p(rx), p(ry), p(rinf), cnt, p(o2[0]), p(o2[1]), p(o2[2])), "vpin_e2_mul256")))
            alternate(variants)
            for w in WIDTHS:
                assert all(np.array_equal(a, b) for a, b in zip(o[w], o2)), f"fixed base at w = {w} and variable base disagree"

            vals = rng.integers(-RANGE, RANGE + 1, size=cnt, dtype=np.int64)
            r = scalars(rng, cnt)
            ct = outs(cnt, 2)
            enc = lambda: _chk(L.vpin_e2_encrypt(ctx.h, base_g, base_h, p(vals), p(r), cnt, *[p(a) for a in ct]), "vpin_e2_encrypt")
            alternate([("encryption (r G, msg G + r H)", enc)])
            sk = np.tile(np.frombuffer(SK.to_bytes(32, "little"), np.uint8), (cnt, 1)).copy()
            t_o = outs(cnt)
            alternate([("sk * c1 (variable base)",
                        lambda: _chk(L.vpin_e2_mul256(ctx.h, p(sk), p(ct[0]), p(ct[1]), p(ct[2]), cnt, p(t_o[0]), p(t_o[1]), p(t_o[2])), "vpin_e2_mul256"))])

            vs = np.frombuffer(b"".join((int(v) % E.ORDER).to_bytes(32, "little") for v in vals), np.uint8).reshape(cnt, 32).copy()
            pts = outs(cnt)
            _chk(L.vpin_e2_base_mul(ctx.h, base_g, p(vs), cnt, p(pts[0]), p(pts[1]), p(pts[2])), "vpin_e2_base_mul")
            got, found = np.zeros(cnt, np.int64), np.zeros(cnt, np.uint8)
            walks = []
            for nb in NBS:
                mg = (RANGE + nb - 1) // nb
                walks.append((f"walk, +-2^35, nb = 2^{int(np.log2(nb))}, max_giant = {mg}",
                              (lambda h, m: lambda: _chk(L.vpin_e2_dlog_solve(ctx.h, h, p(pts[0]), p(pts[1]), p(pts[2]), cnt, m, p(got), p(found)),
                                                         "vpin_e2_dlog_solve"))(tables[nb], mg)))
            alternate(walks)
            assert found.all() and np.array_equal(got, vals), "the walk missed a value"

            nb = E.DEFAULT_NB if E.DEFAULT_NB in tables else NBS[-1]
            mg = (RANGE + nb - 1) // nb
            key = np.frombuffer(SK.to_bytes(32, "little"), np.uint8).copy()
            ct2 = outs(cnt, 2)

            def client_round():
                _chk(L.vpin_e2_decrypt(ctx.h, tables[nb], p(key), *[p(a) for a in ct], cnt, mg, p(got), p(found)), "vpin_e2_decrypt")
                _chk(L.vpin_e2_encrypt(ctx.h, base_g, base_h, p(got), p(r), cnt, *[p(a) for a in ct2]), "vpin_e2_encrypt")

            alternate([(f"client round: decrypt {cnt} + encrypt {cnt}, nb = 2^{int(np.log2(nb))}", client_round)])
            assert found.all() and np.array_equal(got, vals), "the round trip lost a message"
            assert all(np.array_equal(a, b) for a, b in zip(ct, ct2)), "the same r and message encrypt to the same ciphertext"

        for h in tables.values():
            L.vpin_e2_dlog_free(h)
        ctx.e2_base_free(base_h)
        ctx.e2_base_free(base_g)
        for h in bases.values():
            L.vpin_e2_base_free(h)


if __name__ == "__main__":
    main()
