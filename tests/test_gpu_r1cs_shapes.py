"""The kernels of r1cs.hip through the C ABI on the structural instances of r1cs_shapes.py: the sequence of
test_gpu_sat.test_r1cs_kernels_vs_oracle (r1cs_upload, r1cs_build_z, r1cs_multiply_vec, r1cs_eval_table, r1cs_evaluate with
eq tables of random points), compared exactly with the plain Python-integer reference -- above 2 * 10^5 entries with the
oracle's C loops, which test_r1cs_shapes.py shows to agree with it.  Then the refusals: an index one past the limit and
num_inputs == num_vars must come back as VPIN_ESHAPE from vpin_r1cs_upload and vpin_spark_encode, and leave the context
working."""
import ctypes as C

import numpy as np
import pytest

import pymodel as M
import r1cs_shapes as S

pytestmark = pytest.mark.gpu

VPIN_ESHAPE = -5
PY_REF_MAX = 200_000


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def _upload(ctx, inst, null_empty=False):
    """Context.r1cs_upload; null_empty: matrices without entries go up with NULL pointers"""
    from vpin_amd import capi
    if not null_empty:
        return ctx.r1cs_upload(inst)
    r = capi.make_r1cs(inst)
    for m in range(3):
        if r.nnz[m] == 0:
            r.row[m] = r.col[m] = r.val[m] = None
    h = C.c_void_p()
    capi._chk(capi.lib().vpin_r1cs_upload(ctx.h, C.byref(r), C.byref(h)), "vpin_r1cs_upload")
    return capi.R1csDev(ctx, h, inst["num_cons"], inst["num_vars"], inst["num_inputs"])


def run_case(ctx, name, inst=None, null_empty=False):
    inst = inst if inst is not None else S.build(name)
    nc, nv = inst["num_cons"], inst["num_vars"]
    nnz = sum(len(inst[k][0]) for k in "ABC")
    use_py = nnz <= PY_REF_MAX
    di = _upload(ctx, inst, null_empty)
    try:
        tv = ctx.upload(inst["vars"])
        z = ctx.r1cs_build_z(di, tv, inst["inputs"])
        zh = z.read()
        assert np.array_equal(zh, S.build_z(inst))
        got = [t.read() for t in ctx.r1cs_multiply_vec(di, z)]
        exp = [S.dense(d, nc) for d in S.ref_multiply_vec(inst, zh)] if use_py else S.oracle_multiply_vec(inst, zh)
        for m, (g, e) in enumerate(zip(got, exp)):
            assert np.array_equal(g, e), f"{name}: {'ABC'[m]}z differs at rows {np.flatnonzero(np.any(g != e, axis=1))[:8]}"
        rx, ry, rabc, rabc_i = S.challenge_points(name, inst)
        erx, ery = ctx.eq_table(rx), ctx.eq_table(ry)
        erx_h = erx.read()
        tab = ctx.r1cs_eval_table(di, erx, rabc).read()
        if use_py:
            exp_tab = S.dense(S.ref_eval_table(inst, erx_h, rabc_i), 2 * nv)
            exp_ev = M.ints_to_table(S.ref_evaluate(inst, erx_h, ery.read()))
        else:
            exp_tab = S.combine_tables(S.oracle_eval_tables(inst, erx_h), rabc_i)
            exp_ev = S.oracle_evaluate(inst, rx, ry)
        assert np.array_equal(tab, exp_tab), f"{name}: eval table differs at columns {np.flatnonzero(np.any(tab != exp_tab, axis=1))[:8]}"
        assert np.array_equal(ctx.r1cs_evaluate(di, erx, ery), exp_ev), f"{name}: evaluate"
        return got, tab
    finally:
        di.free()


def test_col_lengths(ctx):
    """columns of 1, 255, 256, 257, 2047, 2048, 2049, 4097 and 64 * 2048 + 1 entries; long in A only, B only, C only, all three"""
    run_case(ctx, "col_lengths")


def test_wave_patterns(ctx):
    """64 equal keys, 64 distinct, exactly four repeated keys, six repeated keys, partial last waves of 1 and 63, the hottest
    key in the tail only -- on the row side, the column side, both"""
    run_case(ctx, "wave_patterns")


@pytest.mark.parametrize("name", sorted(S.SCAN_DIMS))
def test_scan_sizes(ctx, name):
    run_case(ctx, name)


def test_second_grid_stride_round(ctx):
    """nnz = 4096 * 256 + 4097: the histogram and the scatter go round twice; a third of the entries in one column"""
    run_case(ctx, "grid_stride")


def test_c_empty_with_null_pointers(ctx):
    got, _ = run_case(ctx, "c_empty", null_empty=True)
    assert not got[2].any()


def test_all_empty(ctx):
    got, tab = run_case(ctx, "all_empty", null_empty=True)
    assert not any(g.any() for g in got) and not tab.any()
    got, tab = run_case(ctx, "all_empty")
    assert not any(g.any() for g in got) and not tab.any()


def test_duplicates_that_cancel(ctx):
    got, _ = run_case(ctx, "dup_cancel")
    assert not got[0].any() and got[1].any()


@pytest.mark.parametrize("name", ["explicit_zeros", "zero_witness"])
def test_zero_values_and_zero_witness(ctx, name):
    got, _ = run_case(ctx, name)
    assert not got[0].any() and got[1].any()


# ---- refusals: error paths, never faults.  The guards: `ok` in triplet_hist_kernel / triplet_scatter_kernel keeps an entry with
# an index out of range away from every counter and store; bounds_kernel reports it and ranks_kernel's `keys[p] < M` keeps it
# from the audit table.  Indices exactly one past the limit, nothing larger. -----------------------------------------------------

def _good():
    return S.build("zero_witness")


def _bad_last_row_of_c():
    inst = _good()
    rows = inst["C"][0].copy()
    rows[-1] = inst["num_cons"]
    inst["C"] = (rows,) + inst["C"][1:]
    return inst


def _bad_first_col_of_a():
    inst = _good()
    cols = inst["A"][1].copy()
    cols[0] = 2 * inst["num_vars"]
    inst["A"] = (inst["A"][0], cols, inst["A"][2])
    return inst


def _inputs_fill_the_half():
    inst = _good()
    inst["num_inputs"] = inst["num_vars"]
    inst["inputs"] = S.random_table(S.rng_of("inputs"), inst["num_vars"])
    return inst


@pytest.mark.parametrize("make", [_bad_last_row_of_c, _bad_first_col_of_a, _inputs_fill_the_half])
def test_refusals(ctx, make):
    from vpin_amd import VpinError
    bad = make()
    with pytest.raises(VpinError) as e:
        ctx.r1cs_upload(bad)
    assert e.value.code == VPIN_ESHAPE
    run_case(ctx, "zero_witness")
    with pytest.raises(VpinError) as e:
        ctx.spark_encode(bad)
    assert e.value.code == VPIN_ESHAPE
    run_case(ctx, "dup_cancel")
    dec, comm = ctx.spark_encode(_good())  # and the encoder still encodes
    assert len(comm) > 0
    dec.free()
