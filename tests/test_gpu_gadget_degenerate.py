"""The seam between the two point-multiplication witness kernels (gadget_dev.hip), on inputs whose denominators vanish.

vpin_gadget_point_mult_dev runs gd_mult_witness_fast_kernel (Jacobian chains, three batched inversions) and hands the
operations it flags to the step-by-step gd_mult_witness_kernel, which carries the reference's inverse(0) = 0 through every
later step.  Every comparison here is exact -- vars_para, vars_input, vars against the Python model of point_mult.rs --
and Context.witness_redo_ops() tells which kernel wrote each batch: the fast kernel must flag exactly the operations whose
denominator_trace (tests/degenerate_points.py, verified without a GPU in tests/test_degenerate_points.py) is not empty.
Why exactly those: up to the first vanishing denominator the Jacobian and the affine values coincide; a zero Z of A_{i+1} is a
zero 2 ay_i, a zero Z of C_i is bx_i = ax_i, and the third batch inverts the denominators themselves."""
import numpy as np
import pytest

import degenerate_points as D
import gadgets_model as GM
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED_C = bytes(range(64))
SEED_P = bytes((13 * i + 7) % 256 for i in range(64))
MULT_VARS, ADD_VARS = 128 * 27 + 10, 15


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def dev_mult(ctx, ops):
    return ctx.gadget_point_mult_dev([o[0] for o in ops], D.bytes32(o[1] for o in ops), D.bytes32(o[2] for o in ops))


def read_tables(g):
    return [getattr(g, k).read() for k in ("vars_para", "vars_input", "vars")]


def table_problems(got, exp, stride, what=""):
    out = []
    for name, a, b in zip(("vars_para", "vars_input", "vars"), got, exp):
        diff = D.first_difference(a, b)
        if diff is not None:
            out.append(f"{what}{name}: {diff[0]} entries differ, first at {diff[1]} (operation {diff[1] // stride}, slot {diff[1] % stride})")
    return out


def assert_tables(got, exp, stride, what=""):
    problems = table_problems(got, exp, stride, what)
    assert not problems, "; ".join(problems)


def flagged(ops):
    return sum(1 for op in ops if D.denominator_trace(*op))


def check_mult(ctx, ops, expected, want_redo, what=""):
    """the witness of ops on the device is the expected tables and the step-by-step kernel wrote want_redo of them: one
    assertion, so that a wrong flag shows both as bytes and as a count"""
    g = dev_mult(ctx, ops)
    try:
        redo = ctx.witness_redo_ops()
        problems = table_problems(read_tables(g), expected, MULT_VARS, what)
    finally:
        g.free()
    if redo != want_redo:
        problems.append(f"{what}redo count {redo}, the model predicts {want_redo}")
    assert not problems, "; ".join(problems)
    return redo


@pytest.fixture(scope="module")
def rows():
    ops = [r[1] for r in D.table_rows()]
    return ops, D.padded_assignment(GM.point_mult_assignment(ops))


@pytest.fixture(scope="module")
def batches():
    """the three 66-operation batches with the model's tables, computed once and left unchanged"""
    return [(ops, D.padded_assignment(GM.point_mult_assignment(ops))) for ops in D.edge_batches()]


def test_one_operation_per_table_row(ctx, rows):
    ops, expected = rows
    assert flagged(ops) == 15 and len(ops) == 23
    redo = check_mult(ctx, ops, expected, flagged(ops))
    print(f"table rows: N = {len(ops)}, redo count {redo}, model predicts {flagged(ops)}")


def test_each_table_row_alone(ctx):
    """N = 1 per row: the flag of every row on its own (a batch only shows their number), one workgroup of one lane"""
    for name, op, first, _ in D.table_rows():
        check_mult(ctx, [op], D.padded_assignment(GM.point_mult_assignment([op])), 0 if first is None else 1, name + ": ")


@pytest.mark.parametrize("which,name", [(0, "lanes 0, 63, 64, 65"), (1, "all degenerate"), (2, "all honest")])
def test_wave_and_workgroup_edges(ctx, batches, which, name):
    """N = 66, workgroups of 64: the fast kernel's second workgroup has two lanes; with all 66 flagged the redo list spans
    two workgroups of the step-by-step kernel (op_list)"""
    ops, expected = batches[which]
    assert flagged(ops) == (4, 66, 0)[which]
    redo = check_mult(ctx, ops, expected, flagged(ops))
    print(f"{name}: N = {len(ops)}, redo count {redo}, model predicts {flagged(ops)}")


def test_single_operation_batches(ctx, batches):
    for ops, want in ((batches[1][0][:1], 1), (batches[2][0][:1], 0)):
        check_mult(ctx, ops, D.padded_assignment(GM.point_mult_assignment(ops)), want)


def test_literal_switch_writes_the_same_bytes(ctx, batches, rows, monkeypatch):
    """VPIN_WITNESS_LITERAL (read on every call) sends every operation to the step-by-step kernel: the counter is N and the
    tables are those of the two-kernel path -- the two kernels compared directly, on honest and unflagged-edge inputs too"""
    for ops, expected in (*batches, rows):
        monkeypatch.delenv("VPIN_WITNESS_LITERAL", raising=False)
        g = dev_mult(ctx, ops)
        both = read_tables(g)
        g.free()
        assert ctx.witness_redo_ops() == flagged(ops)
        monkeypatch.setenv("VPIN_WITNESS_LITERAL", "1")
        g = dev_mult(ctx, ops)
        literal = read_tables(g)
        g.free()
        assert ctx.witness_redo_ops() == len(ops)
        assert_tables(literal, both, MULT_VARS, "literal vs fast+redo, ")
        assert_tables(literal, expected, MULT_VARS, "literal, ")
    monkeypatch.delenv("VPIN_WITNESS_LITERAL", raising=False)
    check_mult(ctx, *batches[2], 0)


def test_point_add_degenerate(ctx):
    """N = 65: R = P, R = -P, rz = 1 with an arbitrary R, rx = px = 0, encodings >= q in lanes 63 and 64"""
    ops = D.add_ops()
    g = ctx.gadget_point_add_dev(*[D.bytes32(o[k] for o in ops) for k in range(4)], np.array([o[4] for o in ops], dtype=np.uint8))
    try:
        assert_tables(read_tables(g), D.padded_assignment(GM.point_add_assignment(ops)), ADD_VARS)
        assert not g.is_sat()
    finally:
        g.free()


def test_downstream_agreement(ctx):
    """is_sat and the proof bytes of a 4-operation instance (2^14 variables) with two degenerate rows: both sides find it
    unsatisfied, and the commitments and the proof the prover writes for it are the oracle's, byte for byte"""
    by_name = {r[0]: r[1] for r in D.table_rows()}
    honest = [by_name["honest, w=2^128-1"], by_name["honest, w=1"], by_name["2P.x=0, w=3"], by_name["order 3, w=0"]]
    bad = [honest[0], by_name["order 3, w=3"], by_name["order 4, w=5"], honest[1]]
    for ops, sat, redo in ((bad, False, 2), (honest, True, 0)):
        inst = GM.instance_new(GM.build_point_mult(ops))
        g = dev_mult(ctx, ops)
        try:
            assert ctx.witness_redo_ops() == redo
            assert_tables(read_tables(g), [inst[k] for k in ("vars_para", "vars_input", "vars")], MULT_VARS)
            assert g.is_sat() == bool(O.is_sat(inst)) == sat
            if not sat:
                got = g.snark_prove(SEED_C, SEED_P)
                exp = O.snark_prove(inst, SEED_C, SEED_P)
                assert np.array_equal(got["comm_para"], exp["comm_para"]) and np.array_equal(got["comm_input"], exp["comm_input"])
                assert got["comm"] == exp["comm"]
                assert got["proof"] == exp["proof"]
                assert O.snark_verify(inst, got) != 1
        finally:
            g.free()
