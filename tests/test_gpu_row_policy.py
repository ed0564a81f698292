"""Which row commitments go to the row-table kernels (row_table_use / row_table_min_scalars in msm.hip): at the threshold a
commitment of n - 1 scalars keeps the multi-window walk and one of n takes the row table, with and without a blind column and for
the derefs shape with hot columns; both give the CPU oracle's bytes.  vpin_ctx_row_table_rows proves which path ran.  The
library's own default is read through vpin_msm_row_min_scalars in a fresh process with no override set, and whole SNARKs are
proven over a forced row table with the default deciding.

The row tables are forced tiny (VPIN_ROW_TABLE_C, read per table build) as in test_gpu_row_table.py: c = 5 -> 51 windows,
c = 13 -> 20 windows.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import pymodel as M

pytestmark = pytest.mark.gpu
Q = M.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 514  # generators: rows of up to 512 scalars, the blind base behind them
N_MIN = 4096


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(ctx):
    """width -> (table with a forced row table, oracle generators)"""
    xyzt, og = O.gens_stream_xyzt(NB)
    out = {}
    for c in (5, 13):
        os.environ["VPIN_ROW_TABLE_C"] = str(c)
        try:
            out[c] = (ctx.gens_shared(f"test_row_policy_c{c}", xyzt, 1), og)
        finally:
            del os.environ["VPIN_ROW_TABLE_C"]
    return out


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def full(rng):
    return int.from_bytes(rng.bytes(32), "little") % Q


def mix(rng, n):
    k = rng.random(n)
    return [0 if k[i] < 0.2 else int(rng.integers(0, 2)) if k[i] < 0.3 else Q - 1 - int(rng.integers(0, 3)) if k[i] < 0.35 else full(rng)
            for i in range(n)]


def committed(ctx, call, n_min, rows, takes):
    """call() under VPIN_MSM_ROW_MIN = n_min: its bytes, after checking that the row-table kernels took `rows` rows or none"""
    taken0 = ctx.row_table_rows()
    with env(VPIN_MSM_ROW_MIN=n_min):
        assert ctx.msm_row_min_scalars() == n_min
        got = call()
    assert ctx.row_table_rows() - taken0 == (rows if takes else 0), (n_min, rows, takes)
    return got


@pytest.mark.parametrize("c", [5, 13])
def test_without_a_blind_column_n_minus_1_walks_and_n_takes_the_row_table(ctx, tables, c):
    """15 x 273 = 4095 scalars against 16 x 256 = 4096 under VPIN_MSM_ROW_MIN = 4096; then the second shape once more with the
    threshold one above it"""
    g, og = tables[c]
    rng = np.random.default_rng(40 + c)
    for rows, ncols, n_min, takes in ((15, 273, N_MIN, False), (16, 256, N_MIN, True), (16, 256, N_MIN + 1, False)):
        assert (rows * ncols >= n_min) == takes
        Z = M.ints_to_table(mix(rng, rows * ncols))
        exp = O.hyrax_commit(Z, rows, np.zeros((rows, 4), dtype=np.uint64), og, ncols + 1)
        got = committed(ctx, lambda: ctx.gens_msm(g, Z, rows, ncols), n_min, rows, takes)
        assert np.array_equal(got, exp), (rows, ncols, n_min)


@pytest.mark.parametrize("c", [5, 13])
def test_with_a_blind_column_the_blinds_count(ctx, tables, c):
    """64 rows of 64 scalars and a blind each are 64 x 65 = 4160 scalars: the row table from a threshold of 4160, the walk from 4161
    -- and from 4097, which the 4096 scalars without the blinds would not reach"""
    g, og = tables[c]
    rng = np.random.default_rng(50 + c)
    rows = ncols = 64
    Z = M.ints_to_table(mix(rng, rows * ncols))
    b = M.ints_to_table([full(rng) for _ in range(rows)])
    exp = O.hyrax_commit(Z, rows, b, og, ncols + 1)
    dZ = ctx.upload(Z)
    try:
        for n_min, takes in ((4160, True), (4161, False), (4097, True)):
            got = committed(ctx, lambda: ctx.hyrax_commit(g, dZ, b, ncols + 1), n_min, rows, takes)
            assert np.array_equal(got, exp), n_min
    finally:
        dZ.free()


@pytest.mark.parametrize("c", [5, 13])
def test_derefs_shape_with_hot_columns(ctx, tables, c):
    """8 rows of R = N = 512 (4096 scalars): three row-derefs rows, the col-derefs rows of three matrices -- a hot column with 40 %
    of the entries, none, a rare one -- and two rows of zeros; the row table at a threshold of 4096, the walk at 4097"""
    g, og = tables[c]
    rng = np.random.default_rng(60 + c)
    R = N = 512
    ncol = 700
    e_ry = [full(rng) for _ in range(ncol)]
    e_ry[7] = 0
    col = rng.integers(0, ncol, size=(3, N), dtype=np.uint32)
    hot = [11, None, 123]
    col[0][rng.random(N) < 0.4] = 11
    col[2][[3, 250]] = 123
    vals = [full(rng) for _ in range(3 * N)] + [e_ry[int(col[m][i])] for m in range(3) for i in range(N)] + [0] * (2 * N)
    Z = M.ints_to_table(vals)
    exp = O.hyrax_commit(Z, 8, np.zeros((8, 4), dtype=np.uint64), og, R + 1)
    dZ, dE = ctx.upload(Z), ctx.upload(M.ints_to_table(e_ry + [0] * (1024 - ncol)))
    try:
        for n_min, takes in ((N_MIN, True), (N_MIN + 1, False)):
            got = committed(ctx, lambda: ctx.hyrax_commit_derefs(g, dZ, 8, N, col, hot, dE), n_min, 8, takes)
            assert np.array_equal(got, exp), n_min
    finally:
        dZ.free()
        dE.free()


DEFAULT_SCRIPT = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import vpin_amd
import oracle_lib as O
L = vpin_amd.lib()
L.vpin_hyrax_commit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
R = 256
xyzt, _ = O.gens_stream_xyzt(R + 2)
rng = np.random.default_rng(3)
with vpin_amd.Context(0) as ctx:
    g = ctx.gens_shared("test_row_policy_default", xyzt, 1)
    n_min = ctx.msm_row_min_scalars()
    above = n_min // (R + 1) + 1          # rows of R scalars and a blind: just above the threshold
    below = max(1, n_min // (8 * (R + 1)))  # an eighth of it
    Ls = 1
    while Ls < above:
        Ls *= 2
    Z = rng.integers(0, 2**63, size=(Ls * R, 4), dtype=np.uint64)
    Z[:, 3] &= np.uint64((1 << 59) - 1)    # below q: as Montgomery images, uniformly random scalars
    dZ = ctx.upload(Z)
    blinds = np.ascontiguousarray(Z[:above])
    def commit(rows):
        out = np.zeros((rows, 32), dtype=np.uint8)
        t0 = ctx.row_table_rows()
        assert L.vpin_hyrax_commit_rows(ctx.h, g.h, dZ.h, Ls, 0, rows, blinds.ctypes.data_as(C.c_void_p), R + 1, out.ctypes.data_as(C.c_void_p)) == 0
        return out, ctx.row_table_rows() - t0
    got_above, taken_above = commit(above)
    got_below, taken_below = commit(below)
    os.environ["VPIN_MSM_ROW_TABLE"] = "0"
    walk_above, walk_taken = commit(above)
    dZ.free()
print(json.dumps(dict(n_min=n_min, above=above, below=below, taken_above=taken_above, taken_below=taken_below, walk_taken=walk_taken,
                      same=bool(np.array_equal(got_above, walk_above)), same_below=bool(np.array_equal(got_below, walk_above[:below])))))
"""


def test_the_library_default_decides_in_a_fresh_process():
    """no override set, a 13-bit row table forced over 258 generators: rows of 256 scalars and a blind, just above
    vpin_msm_row_min_scalars() they take the row table, at an eighth of it they keep the walk; the bytes are the walk's"""
    e = dict(os.environ, VPIN_ROW_TABLE_C="13")
    for k in ("VPIN_MSM_ROW_MIN", "VPIN_MSM_ROW_TABLE", "VPIN_ROW_TABLE", "VPIN_MSM_ROW_WIN_CHUNKS", "VPIN_MSM_STRIP", "VPIN_MSM_STRIP_MIN",
              "VPIN_MSM_PIPPENGER"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", DEFAULT_SCRIPT % dict(root=ROOT)], capture_output=True, text=True, env=e, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["n_min"] > 0
    assert res["above"] * 257 >= res["n_min"] > (res["above"] - 1) * 257
    assert res["taken_above"] == res["above"], res
    assert res["taken_below"] == 0 and res["walk_taken"] == 0, res
    assert res["same"] and res["same_below"], res


CONTEXTS_SCRIPT = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import vpin_amd
import oracle_lib as O
L = vpin_amd.lib()
L.vpin_hyrax_commit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
R = 256
xyzt, _ = O.gens_stream_xyzt(R + 2)
rng = np.random.default_rng(4)
quarter = [x + 8 * ((n // 8) + 4 * (n %% 8)) for x in range(8) for n in range(24, 32)]   # CUs 24..31 of every XCD
with vpin_amd.Context(0) as ctx, vpin_amd.Context(0, cu_mask=quarter) as small:
    g = ctx.gens_shared("test_row_policy_contexts", xyzt, 1)
    gs = small.gens_shared("test_row_policy_contexts", xyzt, 1)
    n_min, n_small, n_pair = ctx.msm_row_min_scalars(), small.msm_row_min_scalars(), ctx.msm_row_min_scalars(part_short=True)
    Lp = 1
    while Lp * R < n_pair:
        Lp *= 2                              # the smallest pair of Lp x R scalars each that reaches the witness threshold
    Z = rng.integers(0, 2**63, size=(Lp * R, 4), dtype=np.uint64)
    Z[:, 3] &= np.uint64((1 << 59) - 1)      # below q: as Montgomery images, uniformly random scalars
    dZ = ctx.upload(Z)
    between = n_small // (R + 1) + 1         # rows of R scalars and a blind: just above the small context's threshold
    blinds = np.ascontiguousarray(Z[:Lp])
    def rows(cx, gg, n):
        out = np.zeros((n, 32), dtype=np.uint8)
        t0 = cx.row_table_rows()
        assert L.vpin_hyrax_commit_rows(cx.h, gg.h, dZ.h, Lp, 0, n, blinds.ctypes.data_as(C.c_void_p), R + 1, out.ctypes.data_as(C.c_void_p)) == 0
        return out, cx.row_table_rows() - t0
    def pair(n):
        sub = ctx.wrap(dZ.device_ptr, n * R)
        t0 = ctx.row_table_rows()
        outs = ctx.hyrax_commit_pair_split(g, sub, sub, blinds[:n], blinds[:n], R + 1)
        taken = ctx.row_table_rows() - t0
        sub.free()
        return np.concatenate(outs), taken
    out_small, taken_small = rows(small, gs, between)
    out_whole, taken_whole = rows(ctx, g, between)
    pair_at, taken_pair_at = pair(Lp)
    pair_half, taken_pair_half = pair(Lp // 2)
    os.environ["VPIN_MSM_ROW_TABLE"] = "0"
    walk_rows, t1 = rows(ctx, g, between)
    walk_at, t2 = pair(Lp)
    walk_half, t3 = pair(Lp // 2)
    dZ.free()
print(json.dumps(dict(n_min=n_min, n_small=n_small, n_pair=n_pair, Lp=Lp, between=between, taken_small=taken_small, taken_whole=taken_whole,
                      taken_pair_at=taken_pair_at, taken_pair_half=taken_pair_half, walk_taken=t1 + t2 + t3,
                      same=bool(np.array_equal(out_small, walk_rows) and np.array_equal(out_whole, walk_rows) and
                                np.array_equal(pair_at, walk_at) and np.array_equal(pair_half, walk_half)))))
"""


def test_the_default_by_context_and_for_the_witness_pair():
    """no override set, a 13-bit row table forced over 258 generators.  A context on 8 CUs per XCD has a default of its own: rows just
    above it take the row table there and, where the whole chip's default is higher, keep the walk on a whole-chip context.  The
    provers' witness pair (vpin_hyrax_commit_pair_split) follows vpin_msm_row_min_scalars(ctx, 1): both polynomials on the row table
    at the smallest power of two of scalars that reaches it, none at half of that where that lies below it.  Bytes: the walk's."""
    e = dict(os.environ, VPIN_ROW_TABLE_C="13")
    for k in ("VPIN_MSM_ROW_MIN", "VPIN_MSM_ROW_TABLE", "VPIN_ROW_TABLE", "VPIN_MSM_ROW_WIN_CHUNKS", "VPIN_MSM_STRIP", "VPIN_MSM_STRIP_MIN",
              "VPIN_MSM_PIPPENGER"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", CONTEXTS_SCRIPT % dict(root=ROOT)], capture_output=True, text=True, env=e, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert 0 < res["n_small"] <= res["n_min"] <= res["n_pair"], res
    scalars = res["between"] * 257
    assert res["taken_small"] == res["between"], res
    assert res["taken_whole"] == (res["between"] if scalars >= res["n_min"] else 0), res
    assert res["taken_pair_at"] == 2 * res["Lp"], res
    assert res["taken_pair_half"] == (res["Lp"] if res["Lp"] // 2 * 256 >= res["n_pair"] else 0), res
    assert res["walk_taken"] == 0 and res["same"], res


SNARK_SCRIPT = r"""
import hashlib, json, sys
sys.path.insert(0, %(root)r)
import vpin_amd
from vpin_amd import gadgets as G
SEED_C, SEED_P = bytes(range(64)), bytes((7 * i + 3) %% 256 for i in range(64))
out = {}
with vpin_amd.Context(0) as ctx:
    for key in ("3_32-mult", "A-mult"):
        label, kind = key.split("-")
        d = ctx.gadget_point_mult_dev(*G.synthetic_mult_inputs(label))
        r = d.snark_prove(SEED_C, SEED_P)
        out[key] = hashlib.sha256(r["proof"]).hexdigest()
        d.free()
    out["rows"] = ctx.row_table_rows()
    out["n_min"] = ctx.msm_row_min_scalars()
print(json.dumps(out))
"""


def test_whole_snarks_over_a_forced_row_table_with_the_default_threshold():
    """3_32-mult and A-mult with every table of the process carrying a 13-bit row table and no VPIN_MSM_ROW_MIN: whichever
    commitments the default sends to the row table, the golden SNARK digests"""
    with open(os.path.join(ROOT, "tests", "golden", "config_digests.json")) as f:
        gold = json.load(f)["cases"]
    e = dict(os.environ, VPIN_ROW_TABLE_C="13")
    for k in ("VPIN_MSM_ROW_MIN", "VPIN_MSM_STRIP", "VPIN_MSM_STRIP_MIN", "VPIN_MSM_ROW_TABLE", "VPIN_ROW_TABLE"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", SNARK_SCRIPT % dict(root=ROOT)], capture_output=True, text=True, env=e, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    for key in ("3_32-mult", "A-mult"):
        assert res[key] == gold[key]["snark_sha256"], key
