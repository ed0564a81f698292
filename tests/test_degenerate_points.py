"""The degenerate gadget inputs of tests/degenerate_points.py, checked where no GPU is needed: every construction puts its
vanishing denominator at the step and of the kind it is made for (or, for the rows made to stay regular, nowhere), and the
host builder (gadgets.cpp: vpin_gadget_point_mult / vpin_gadget_point_add) writes the model's three assignment vectors for
them -- the reference's inverse(0) = 0 carried through every later step (point_mult.rs:414-500, 667-704)."""
import numpy as np
import pytest

import degenerate_points as D
import gadgets_model as GM
from vpin_amd import gadgets as G

ROWS = D.table_rows()


def test_square_root():
    for v in (0, 1, 4, 2, 5, GM.E2_A, D.Q - 1):
        r = D.sqrt_mod_q(v)
        assert (r is None) == (pow(v, (D.Q - 1) // 2, D.Q) == D.Q - 1)
        assert r is None or r * r % D.Q == v % D.Q
    assert D.sqrt_mod_q(2) is None and D.sqrt_mod_q(D.Q - 1) is not None  # q = 5 mod 8: 2 is no square, -1 is


def test_points_have_the_order_they_are_made_for():
    """on the sibling curve through the point, with the model's own group law formulas"""
    a = GM.E2_A
    dbl = lambda p: GM._pd(p[0], p[1], a)[:2]
    assert D.order2_point(1)[1] == 0
    p = D.order4_point(2)
    assert p[1] != 0 and dbl(p)[1] == 0
    p = D.order3_point(3)
    assert dbl(p) == (p[0], D.Q - p[1])
    p = D.double_has_x_zero_point(5)
    assert p[0] != 0 and p[1] != 0 and dbl(p)[0] == 0 and dbl(p)[1] != 0
    assert D.x_zero_point(4)[0] == 0 and D.x_zero_point(4)[1] != 0
    p = D.order5_point(6)
    p2 = dbl(p)
    assert p2[0] != p[0] and dbl(p2) == (p[0], D.Q - p[1])  # 4P = -P, 2P != +-P


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_trace_is_what_the_construction_claims(row):
    _, op, first, whole = row
    trace = D.denominator_trace(*op)
    assert (trace[0] if trace else None) == first
    if whole is not None:
        assert trace == whole
    assert op[0] < 1 << 128 and op[1] < 1 << 256 and op[2] < 1 << 256


def test_table_covers_both_outcomes_and_both_kinds():
    firsts = [r[2] for r in ROWS]
    assert sum(f is None for f in firsts) == 8 and sum(f is not None for f in firsts) == 15
    assert {f[0] for f in firsts if f} == {"pa", "pd"} and {f[1] for f in firsts if f} == {0, 1, 3, 101}
    assert any(op[1] >= D.Q for _, op, _, _ in ROWS) and any(op[2] >= D.Q for _, op, _, _ in ROWS)


def test_edge_batches_are_degenerate_where_they_say():
    mixed, degenerate, honest = D.edge_batches()
    assert len(mixed) == len(degenerate) == len(honest) == 66
    assert [j for j, op in enumerate(mixed) if D.denominator_trace(*op)] == [0, 63, 64, 65]
    assert all(D.denominator_trace(*op) for op in degenerate) and len(set(degenerate)) >= 8
    assert not any(D.denominator_trace(*op) for op in honest)
    # neighbours differ in kind: a lane that the fast kernel leaves early sits beside lanes that leave later, or not at all
    assert len({D.denominator_trace(*mixed[j])[0] for j in (0, 63, 64, 65)}) == 4


def host_mult_tables(ops):
    inst = G.point_mult([o[0] for o in ops], D.bytes32(o[1] for o in ops), D.bytes32(o[2] for o in ops))
    try:
        d = inst.as_dict()
        return [d[k] for k in ("vars_para", "vars_input", "vars")], inst.is_sat()
    finally:
        inst.free()


def assert_tables(got, exp, stride):
    for name, g, e in zip(("vars_para", "vars_input", "vars"), got, exp):
        diff = D.first_difference(g, e)
        assert diff is None, f"{name}: {diff[0]} entries differ, first at {diff[1]} (operation {diff[1] // stride}, slot {diff[1] % stride})"


def test_host_builder_equals_model_on_every_row():
    ops = [r[1] for r in ROWS]
    got, sat = host_mult_tables(ops)
    assert_tables(got, D.padded_assignment(GM.point_mult_assignment(ops)), 128 * 27 + 10)
    assert not sat  # c * (bx - ax) = 1 cannot hold with c = 0


def test_host_builder_equals_model_on_honest_rows():
    ops = [r[1] for r in ROWS if r[2] is None]
    got, sat = host_mult_tables(ops)
    assert_tables(got, D.padded_assignment(GM.point_mult_assignment(ops)), 128 * 27 + 10)
    assert sat  # nothing vanishes: satisfied, on the curve or not


@pytest.mark.parametrize("which", [0, 1], ids=["mixed", "all degenerate"])
def test_host_builder_equals_model_on_edge_batches(which):
    ops = D.edge_batches()[which]
    got, sat = host_mult_tables(ops)
    assert_tables(got, D.padded_assignment(GM.point_mult_assignment(ops)), 128 * 27 + 10)
    assert not sat


def test_host_point_add_equals_model():
    ops = D.add_ops()
    assert len(ops) == 65
    zero_den = [i for i, o in enumerate(ops) if (o[2] - o[0]) % D.Q == 0]
    assert zero_den == [2, 3, 6, 7, 64]
    assert [i for i, o in enumerate(ops) if max(o[:4]) >= D.Q] == [63, 64]
    inst = G.point_add(*[D.bytes32(o[k] for o in ops) for k in range(4)], np.array([o[4] for o in ops], dtype=np.uint8))
    try:
        d = inst.as_dict()
        assert_tables([d[k] for k in ("vars_para", "vars_input", "vars")], D.padded_assignment(GM.point_add_assignment(ops)), 15)
        assert not inst.is_sat()
    finally:
        inst.free()


def test_assignment_split_is_the_builders_formula():
    """build_point_mult / build_point_add return what point_*_assignment computes: one formula, two callers"""
    ops = [ROWS[2][1], ROWS[-1][1]]
    g = GM.build_point_mult(ops)
    assert (g["vars_para"], g["vars_input"], g["vars"]) == GM.point_mult_assignment(ops)
    ops = D.add_ops()[:8]
    g = GM.build_point_add(ops)
    assert (g["vars_para"], g["vars_input"], g["vars"]) == GM.point_add_assignment(ops)
    assert np.array_equal(D.to_table([0, 1, D.Q - 1, 5]), GM.M.ints_to_table([0, 1, D.Q - 1, 5]))
