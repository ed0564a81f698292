"""fp10_dev.h and ge_tree_dev.h's ge10_horner_windows on the GPU through tests/devarith/devarith.hip: the ten-limb field
functions on raw limbs at their documented bounds, and the ten-limb point functions on points whose eight-limb coordinates sit
at the top of their range (limb 9 of the ten-limb form all ones), which ge10_from_ext has to bring inside the bound that
fe10_sub assumes of its second operand.  Exact: field values mod p, points as affine (X/Z, Y/Z) with pymodel_group."""
import pytest

import devarith_lib as D
import limb_vectors as V

pytestmark = pytest.mark.gpu
P = V.P
EDGE, PLAIN = V.edge_points(), V.plain_points()


def test_fe10_mul():
    cases = V.fe10_mul_cases()
    out = D.run("fe10_mul", [f + g for f, g in cases], 10)
    for (f, g), o in zip(cases, out):
        assert V.fe10_value(o) % P == V.fe10_value(f) * V.fe10_value(g) % P, (f, g)
        assert V.fe10_is_1x(o), (f, g, "the product is wider than 1x")


def test_fe10_from_fp_and_back():
    xs = V.FP_SEEDS + [a for a, _ in V.FP_PAIRS[-256:]]
    ten = D.run("fe10_from_fp", [V.limbs(a) for a in xs], 10)
    for a, o in zip(xs, ten):
        assert [int(x) for x in o] == V.fe10_split(a), hex(a)
    back = D.ints(D.run("fe10_to_fp", ten, 8))
    assert [b % P for b in back] == [a % P for a in xs]


def test_fe10_to_fp_up_to_4x():
    cases = [f for f, _ in V.fe10_mul_cases()] + [V.fe10_max(4), V.fe10_max(1)]
    back = D.ints(D.run("fe10_to_fp", cases, 8))
    assert [b % P for b in back] == [V.fe10_value(f) % P for f in cases]


def test_fe10_sub_and_add():
    cases = V.fe10_sub_cases()
    out = D.run("fe10_sub", [a + b for a, b in cases], 10)
    for (a, b), o in zip(cases, out):
        assert [int(x) for x in o] == [x + bias - y for x, y, bias in zip(a, b, V.FE10_SUB_BIAS)], (a, b)
        assert V.fe10_value(o) % P == (V.fe10_value(a) - V.fe10_value(b)) % P
    out = D.run("fe10_add", [a + b for a, b in cases], 10)
    assert [[int(x) for x in o] for o in out] == [[x + y for x, y in zip(a, b)] for a, b in cases]


def check_points(out, expected, what):
    bad = []
    for o, (label, pt) in zip(out, expected):
        xy, on = V.affine_of_words(o)
        if not on or xy != V.affine(pt):
            bad.append(label)
    assert not bad, (what, len(bad), bad[:8])


def test_ge10_from_ext_keeps_the_point_and_the_bound():
    out = D.run("ge10_roundtrip", [V.point_words(e[1]) for e in EDGE + PLAIN], 72)
    for e, o in zip(EDGE + PLAIN, out):
        for k in range(4):
            assert V.fe10_value(o[10 * k:10 * k + 10]) % P == e[1][k] % P, (e[0], V.COORDS[k])
            assert V.fe10_is_1x(o[10 * k:10 * k + 10]), (e[0], V.COORDS[k], "ge10_from_ext returns more than 1x")
    check_points([o[40:] for o in out], [(e[0], e[2]) for e in EDGE + PLAIN], "ge10_to_ext(ge10_from_ext)")


def test_ge10_add_ge10_either_operand():
    cases = [(a, b) for a in EDGE for b in PLAIN + EDGE[:4]] + [(b, a) for a in EDGE for b in PLAIN + EDGE[:4]]
    out = D.run("ge10_add_ge10", [V.point_words(a[1]) + V.point_words(b[1]) for a, b in cases], 32)
    check_points(out, [(a[0] + " + " + b[0], a[2] + b[2]) for a, b in cases], "ge10_add_ge10")


@pytest.mark.parametrize("neg", [0, 1])
def test_ge10_add_niels(neg):
    cases = [(a, b) for a in EDGE + PLAIN for b in PLAIN]
    out = D.run("ge10_add_niels", [V.point_words(a[1]) + V.niels_words(b[2]) + [neg] for a, b in cases], 32)
    check_points(out, [(a[0] + " +-"[1 + neg] + b[0], a[2] - b[2] if neg else a[2] + b[2]) for a, b in cases], "ge10_add_niels")


def test_ge10_add_cached():
    cases = [(a, b) for a in EDGE + PLAIN for b in PLAIN + EDGE]
    out = D.run("ge10_add_cached", [V.point_words(a[1]) + V.cached_words(b[1]) for a, b in cases], 32)
    check_points(out, [(a[0] + " + " + b[0], a[2] + b[2]) for a, b in cases], "ge10_add_cached")


@pytest.mark.parametrize("neg", [0, 1])
def test_ge10_add_niels_entries_at_the_top_of_their_range(neg):
    """a weakly reduced table entry goes through the unchanged fe10_from_fp: limb 9 up to 2^26 - 1, a second factor of fe10_mul"""
    import pymodel_group as PG
    qs = [("id", None, PG.Pt.identity())] + PLAIN[::2]
    cases = [(a, b) for a in EDGE + PLAIN for b in qs]
    out = D.run("ge10_add_niels", [V.point_words(a[1]) + V.niels_words_top(b[2]) + [neg] for a, b in cases], 32)
    check_points(out, [(a[0] + " +-"[1 + neg] + b[0], a[2] - b[2] if neg else a[2] + b[2]) for a, b in cases], "ge10_add_niels")


def test_ge10_add_cached_entries_at_the_top_of_their_range():
    cases = [(a, b) for a in EDGE + PLAIN for b in V.cached_top_cases()]
    out = D.run("ge10_add_cached", [V.point_words(a[1]) + b[1] for a, b in cases], 32)
    check_points(out, [(a[0] + " + " + b[0], a[2] + b[2]) for a, b in cases], "ge10_add_cached")


def test_ge10_double():
    out = D.run("ge10_double", [V.point_words(a[1]) for a in EDGE + PLAIN], 32)
    check_points(out, [(a[0], a[2] + a[2]) for a in EDGE + PLAIN], "ge10_double")


@pytest.mark.parametrize("cw", [3, 9, 13])
def test_ge10_horner_three_windows(cw):
    q0, q1 = PLAIN[0], PLAIN[3]
    cases = [(e, q0, q1) for e in EDGE] + [(q0, e, q1) for e in EDGE] + [(q0, q1, e) for e in EDGE]
    cases += [(EDGE[0], EDGE[0], EDGE[0]), (EDGE[0], EDGE[1], EDGE[4]), (EDGE[5], EDGE[0], EDGE[0])]
    rows = [V.point_words(a[1]) + V.point_words(b[1]) + V.point_words(c[1]) + [cw] + [0] * 31 for a, b, c in cases]
    out = D.run("ge10_horner3", rows, 32)
    exp = [("/".join((a[0], b[0], c[0])), a[2] + (1 << cw) * b[2] + (1 << (2 * cw)) * c[2]) for a, b, c in cases]
    check_points(out, exp, "ge10_horner_windows")
