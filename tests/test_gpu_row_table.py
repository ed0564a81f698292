"""GPU parity of the row-table commitment (msm_rows_win_kernel + msm_rows_finish_kernel): one window per generator,
T1[j][k] = (k+1) g_j, one accumulator per lane and window, the powers of two applied once per row.  Every case compares the
bytes of the new kernels with the CPU oracle's MSM AND with the multi-window row walk (VPIN_MSM_ROW_TABLE=0) over the same table
object, and checks through vpin_ctx_row_table_rows that the path under test is the one that ran.

The window width is forced small (VPIN_ROW_TABLE_C, read per table build) so that several windows, LDS segments and carries
occur at a few hundred generators:
    c = 5  -> W = 51 windows (does not divide 256), 480 columns per segment
    c = 8  -> W = 32, 768 columns per segment
    c = 13 -> W = 20 (does not divide 256), 1228 columns per segment
and once at c = 16 (W = 16, 1536 columns per segment), the width production uses and the only one at which the 16-bit digit words
are tight: magnitude - 1 fills 15 bits and 0xffff, the no-digit marker, must never be a digit.
"""
import ctypes as C
import hashlib
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
NB = {5: 514, 8: 771, 13: 300, 16: 300}  # generators per forced width: R + gens_1 base + h
SEG = {5: 480, 8: 768, 13: 1228, 16: 1536}


def windows(c):
    return (253 + c - 1) // c


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(ctx):
    """width -> (table with a forced row table, oracle generators); one build per width for the whole module"""
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_gens_row_layout.argtypes = [C.c_void_p, C.c_void_p]
    xyzt, og = O.gens_stream_xyzt(max(NB.values()))
    out = {}
    for c, nb in NB.items():
        os.environ["VPIN_ROW_TABLE_C"] = str(c)
        try:
            g = ctx.gens_shared(f"test_row_table_c{c}", xyzt[:nb], 1)
        finally:
            del os.environ["VPIN_ROW_TABLE_C"]
        lay = (C.c_size_t * 4)()
        assert L.vpin_gens_row_layout(g.h, lay) == 0
        assert list(lay) == [c, windows(c), nb, SEG[c]], list(lay)
        out[c] = (g, og)
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


def check_commit(ctx, g, og, vals, Ls, blinds=None, chunks=None):
    """new kernels == multi-window walk == oracle, for Ls rows of len(vals) / Ls scalars (+ blinds on the last generator of the row's
    stream prefix when given)"""
    Rs = len(vals) // Ls
    Z = M.ints_to_table(vals)
    zero_blinds = np.zeros((Ls, 4), dtype=np.uint64)
    b = zero_blinds if blinds is None else M.ints_to_table(blinds)
    exp = O.hyrax_commit(Z, Ls, b, og, Rs + 1)
    kv = dict(VPIN_MSM_ROW_MIN=0)
    if chunks:
        kv["VPIN_MSM_ROW_WIN_CHUNKS"] = chunks
    dZ = ctx.upload(Z) if blinds is not None else None   # a device table holds a power of two of scalars; without blinds
    try:                                                  # the scalars go up with the call (vpin_gens_msm)
        taken0 = ctx.row_table_rows()
        with env(**kv):
            got = ctx.hyrax_commit(g, dZ, b, Rs + 1) if blinds is not None else ctx.gens_msm(g, Z, Ls, Rs)
        taken1 = ctx.row_table_rows()
        assert taken1 == taken0 + Ls, "the row-table kernels did not take the commitment"
        with env(VPIN_MSM_ROW_TABLE=0):
            walk = ctx.hyrax_commit(g, dZ, b, Rs + 1) if blinds is not None else ctx.gens_msm(g, Z, Ls, Rs)
        assert ctx.row_table_rows() == taken1, "VPIN_MSM_ROW_TABLE=0 must keep the multi-window walk"
    finally:
        if dZ is not None:
            dZ.free()
    assert np.array_equal(walk, exp), "multi-window walk against the oracle"
    assert np.array_equal(got, exp), "row-table kernels against the oracle"


def edge_scalars(c):
    W, half = windows(c), 1 << (c - 1)
    all_half = sum(half << (c * w) for w in range(W - 1))            # every digit exactly 2^(c-1), the top one zero
    all_half1 = sum((half + 1) << (c * w) for w in range(W - 1))     # every digit 2^(c-1)+1: the carry ripples to the top
    assert all_half1 < (1 << 251)
    return [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2,                 # the two sides of the fold
            all_half, all_half1, Q - all_half, Q - all_half1,        # and the same digits behind the fold
            (1 << 251) - 1, 1 << 251,                                # the largest top window: unfolded, and folded (q - 2^251)
            (1 << 251) + 1, half, half + 1, (1 << c) - 1, 1 << c]


@pytest.mark.parametrize("c", [5, 8, 13, 16])
def test_digit_edge_cases_one_row_each(ctx, tables, c):
    g, og = tables[c]
    rng = np.random.default_rng(c)
    for s in edge_scalars(c):
        # the scalar alone, then among bits, 128-bit values and full-width scalars inside one wave
        check_commit(ctx, g, og, [s] + [0] * 63, 1)
        mixed = [int(rng.integers(0, 2)) if k % 3 == 0 else int.from_bytes(rng.bytes(16), "little") if k % 3 == 1 else full(rng)
                 for k in range(64)]
        mixed[17] = s
        check_commit(ctx, g, og, mixed, 1, blinds=[full(rng)])


@pytest.mark.parametrize("c,ncols", [(5, 300), (5, 480), (5, 481), (5, 512), (8, 100), (8, 256), (8, 767), (8, 768), (8, 769), (13, 298), (16, 298)])
def test_shapes_around_a_segment(ctx, tables, c, ncols):
    """below one segment, exactly one, one plus 1, not a multiple of 256 / W; 1 row, and 9 rows in 3 column chunks"""
    g, og = tables[c]
    rng = np.random.default_rng(1000 * c + ncols)

    def mix(n):
        k = rng.random(n)
        return [0 if k[i] < 0.3 else int(rng.integers(0, 2)) if k[i] < 0.4 else Q - 1 - int(rng.integers(0, 3)) if k[i] < 0.45
                else full(rng) for i in range(n)]
    check_commit(ctx, g, og, mix(ncols), 1)
    check_commit(ctx, g, og, mix(9 * ncols), 9, chunks=3)
    if ncols & (ncols - 1) == 0:   # with blinds on generator ncols + 1: an extra column behind the row's own
        check_commit(ctx, g, og, mix(8 * ncols), 8, blinds=[full(rng) for _ in range(8)], chunks=3)


@pytest.mark.parametrize("c", [5, 8])
def test_constant_nearly_constant_and_zero_rows(ctx, tables, c):
    g, og = tables[c]
    rng = np.random.default_rng(77 + c)
    R = 512
    s = full(rng)
    nearly = [s] * R
    nearly[R // 3] = full(rng)
    rows = [s] * R + nearly + [0] * R + [1] * R + [full(rng) for _ in range(R)]
    check_commit(ctx, g, og, rows, 5)
    rows += [Q - 1] * R + [full(rng) for _ in range(R)] + [2] * (R - 1) + [3]   # eight rows: a device table is a power of two long
    check_commit(ctx, g, og, rows, 8, blinds=[full(rng) for _ in range(8)], chunks=2)


@pytest.mark.parametrize("c", [5, 8])
def test_derefs_shaped_commitment_with_and_without_hot_columns(ctx, tables, c):
    """8 rows of R = 256: three row-derefs rows, the col-derefs rows of three matrices -- a hot column with 40 % of the entries in
    the first, none in the second, a rare one in the third -- and the two all-zero padding rows (constant rows)"""
    g, og = tables[c]
    rng = np.random.default_rng(5 + c)
    R = N = 256
    ncol = 512
    e_ry = [full(rng) for _ in range(ncol)]
    e_ry[7] = 0  # a zero value in the memory: its entries are skipped wherever they sit
    col = rng.integers(0, ncol, size=(3, N), dtype=np.uint32)
    hot = [11, None, 123]
    col[0][rng.random(N) < 0.4] = 11
    col[2][[3, 250]] = 123
    vals = [full(rng) for _ in range(3 * N)] + [e_ry[int(col[m][i])] for m in range(3) for i in range(N)] + [0] * (2 * N)
    Z = M.ints_to_table(vals)
    exp = O.hyrax_commit(Z, 8, np.zeros((8, 4), dtype=np.uint64), og, R + 1)
    dZ, dE = ctx.upload(Z), ctx.upload(M.ints_to_table(e_ry))
    try:
        taken0 = ctx.row_table_rows()
        with env(VPIN_MSM_ROW_MIN=0):
            got = ctx.hyrax_commit_derefs(g, dZ, 8, N, col, hot, dE)
        assert ctx.row_table_rows() == taken0 + 8
        with env(VPIN_MSM_ROW_TABLE=0):
            walk = ctx.hyrax_commit_derefs(g, dZ, 8, N, col, hot, dE)
        assert ctx.row_table_rows() == taken0 + 8
    finally:
        dZ.free()
        dE.free()
    assert np.array_equal(walk, exp)
    assert np.array_equal(got, exp)


def model_additions(s, c):
    """non-zero signed digits of s as msm_rows_win_kernel recodes it (row_digit in msm.hip)"""
    W, half, fullw = windows(c), 1 << (c - 1), 1 << c
    flip = s >= (1 << 251)
    if flip:
        s = Q - s
    carry = n = 0
    for w in range(W):
        v = (s & (fullw - 1)) + carry
        s >>= c
        neg = w != W - 1 and (v >= half if flip else v > half)
        mag = fullw - v if neg else v
        carry = 1 if neg else 0
        n += mag != 0
    return n


@pytest.mark.parametrize("c", [8, 13, 16])
def test_counting_aid_counts_the_row_table_additions(ctx, tables, c):
    """vpin_prof_enable(ctx, 2): the additions of 128 rows of 64 non-zero full-width scalars are what the recoding gives, and per
    scalar ceil(252 / c) less the zero digits: a digit is zero with probability 2^-c, the top one (252 - c (W - 1) bits) more often"""
    g, og = tables[c]
    rng = np.random.default_rng(31 * c)
    rows, ncols, W = 128, 64, -(-252 // c)
    vals = [full(rng) or 1 for _ in range(rows * ncols)]
    Z = M.ints_to_table(vals)
    ctx.prof_enable(2)
    try:
        ctx.prof_reset()
        with env(VPIN_MSM_ROW_MIN=0):
            ctx.gens_msm(g, Z, rows, ncols)
        counted = ctx.prof_read()["msm_rows"]["units"]
    finally:
        ctx.prof_enable(0)
    assert counted == sum(model_additions(s, c) for s in vals)
    per_scalar = counted / len(vals)
    top_bits = 252 - c * (W - 1)
    print(f"c = {c}: {per_scalar:.3f} additions per full-width scalar, W = {W}")
    assert W == windows(c)
    assert W - 2.0 ** -(top_bits - 1) - W * 2.0 ** -c - 0.05 <= per_scalar <= W


SNARK_SCRIPT = r"""
import hashlib, json, sys
sys.path.insert(0, %(root)r)
import vpin_amd
from vpin_amd import gadgets as G
SEED_C, SEED_P = bytes(range(64)), bytes((7 * i + 3) %% 256 for i in range(64))
out = {}
with vpin_amd.Context(0) as ctx:
    for key in ("3_32-mult", "3_32-add", "A-mult", "A-add"):
        label, kind = key.split("-")
        d = ctx.gadget_point_mult_dev(*G.synthetic_mult_inputs(label)) if kind == "mult" else ctx.gadget_point_add_dev(*G.synthetic_add_inputs(label))
        r = d.snark_prove(SEED_C, SEED_P)
        out[key] = hashlib.sha256(r["proof"]).hexdigest()
        d.free()
    out["rows"] = ctx.row_table_rows()
print(json.dumps(out))
"""


@pytest.mark.parametrize("c", [5, 13])
def test_whole_snarks_over_a_forced_row_table(c):
    """the 3_32 and A instances with every table of the process (a registry: hence the child) carrying a c-bit row table and every
    row commitment, the derefs commitment with its hot columns included, on the row-table kernels: the golden SNARK digests"""
    with open(os.path.join(ROOT, "tests", "golden", "config_digests.json")) as f:
        gold = json.load(f)["cases"]
    e = dict(os.environ, VPIN_ROW_TABLE_C=str(c), VPIN_MSM_ROW_MIN="0")
    for k in ("VPIN_MSM_STRIP", "VPIN_MSM_STRIP_MIN", "VPIN_MSM_ROW_TABLE", "VPIN_ROW_TABLE"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", SNARK_SCRIPT % dict(root=ROOT)], capture_output=True, text=True, env=e, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["rows"] > 0, "no commitment went through the row-table kernels"
    for key in ("3_32-mult", "3_32-add", "A-mult", "A-add"):
        assert res[key] == gold[key]["snark_sha256"], key


POLICY_SCRIPT = r"""
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import vpin_amd
import oracle_lib as O
L = vpin_amd.lib()
L.vpin_gens_layout.argtypes = [C.c_void_p, C.c_void_p]
L.vpin_gens_row_layout.argtypes = [C.c_void_p, C.c_void_p]
L.vpin_spark_gens_view.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
def layouts(h):
    lay, row = (C.c_size_t * 6)(), (C.c_size_t * 4)()
    assert L.vpin_gens_layout(h, lay) == 0 and L.vpin_gens_row_layout(h, row) == 0
    return list(lay), list(row)
with vpin_amd.Context(0) as ctx:
    gv, Lv, Rv = C.c_void_p(), C.c_size_t(), C.c_size_t()
    assert L.vpin_spark_gens_view(ctx.h, 24, C.byref(gv), C.byref(Lv), C.byref(Rv)) == 0   # R = 4096: 4098 generators, the provers' path
    prover = layouts(gv)
    xyzt, _ = O.gens_stream_xyzt(4098, b"gens_r1cs_eval")
    public = layouts(ctx.gens_shared("gens_r1cs_eval", xyzt, %(gb)d).h)                     # the public entry point, same budget
print(json.dumps(dict(prover=prover, public=public)))
"""


@pytest.mark.parametrize("gb,row", [(4, True), (3, False)])
def test_budget_policy_in_a_fresh_process(gb, row):
    """4098 generators in 96-byte slots: a 13-bit row table (1.61 GB) beside the 8-bit multi-window table of the 4111 bases (1.62 GB)
    fits 4 GiB and not 3 GiB (by 7 MB).  Where it fits the provers' table is that pair; where it does not, its geometry is exactly
    the public entry point's, 9-bit windows -- which never builds a row table in either case."""
    e = dict(os.environ, VPIN_SPARK_GENS_BUDGET_GB=str(gb), VPIN_TABLE_SLOT="96")
    for k in ("VPIN_ROW_TABLE_C", "VPIN_ROW_TABLE", "VPIN_GENS_CMAX"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", POLICY_SCRIPT % dict(root=ROOT, gb=gb)], capture_output=True, text=True, env=e, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    (lay, rlay), (plain, plain_row) = res["prover"], res["public"]
    assert plain_row == [0, 0, 0, 0]
    assert plain[:2] == [9, 29], plain   # the widest multi-window table under either budget, as before (10 bits are 5.2 GB)
    if row:
        assert rlay == [13, 20, 4098, 1228], rlay
        assert lay[:2] == [8, 32] and lay[3] == 0 and lay[2] == lay[5], lay
    else:
        assert rlay == [0, 0, 0, 0], rlay
        assert lay == plain, (lay, plain)
