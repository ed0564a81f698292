"""fp_dev.h and ge_tree_dev.h's ge_tree_quad on the GPU, function by function through tests/devarith/devarith.hip, on the limb
patterns of limb_vectors.py: every representative below 2^256 is a valid input, results are compared mod p (exactly where the
function promises the canonical form), points as affine (X/Z, Y/Z) with pymodel_group.
"""
import pytest

import devarith_lib as D
import limb_vectors as V
import pymodel_group as PG

pytestmark = pytest.mark.gpu
P, B256 = V.P, V.B256
UNARY = V.FP_SEEDS + [a for a, _ in V.FP_PAIRS[-256:]]


def rows2(pairs):
    return [V.limbs(a) + V.limbs(b) for a, b in pairs]


def rows1(xs):
    return [V.limbs(a) for a in xs]


@pytest.mark.parametrize("name,ref", [("fp_add", lambda a, b: a + b), ("fp_sub", lambda a, b: a - b), ("fp_mul", lambda a, b: a * b)])
def test_binary(name, ref):
    got = D.ints(D.run(name, rows2(V.FP_PAIRS), 8))
    bad = [(hex(a), hex(b), hex(g)) for (a, b), g in zip(V.FP_PAIRS, got) if g % P != ref(a, b) % P]
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("name,ref", [("fp_neg", lambda a: -a), ("fp_sqr", lambda a: a * a)])
def test_unary(name, ref):
    got = D.ints(D.run(name, rows1(UNARY), 8))
    bad = [(hex(a), hex(g)) for a, g in zip(UNARY, got) if g % P != ref(a) % P]
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("s", V.FP_SMALL)
def test_mul_small(s):
    got = D.ints(D.run("fp_mul_small", [V.limbs(a) + [s] for a in UNARY], 8))
    bad = [(hex(a), hex(g)) for a, g in zip(UNARY, got) if g % P != a * s % P]
    assert not bad, (len(bad), bad[:4])


def test_freeze_is_exact():
    got = D.ints(D.run("fp_freeze", rows1(UNARY), 8))
    bad = [(hex(a), hex(g)) for a, g in zip(UNARY, got) if g != a % P]
    assert not bad, (len(bad), bad[:4])


def test_predicates_on_unequal_representatives():
    vals = list(range(0, 40)) + [P - 2, P - 1, 2**254, 2**255 - 20] + [a % P for a in V.FP_SEEDS]
    reps = lambda v: [r for r in (v % P, v % P + P, v % P + 2 * P) if r < B256]
    cases = [(a, b) for v in vals for a in reps(v) for b in reps(v)]
    cases += [(a, b) for v in vals for a in reps(v) for b in reps(v + 1)] + [(a, 0) for a in V.FP_SEEDS]
    out = D.run("fp_pred", rows2(cases), 3)
    assert sum(1 for a, b in cases if a != b and a % P == b % P) > 100
    for (a, b), o in zip(cases, out):
        assert [int(x) for x in o] == [(a % P) & 1, int(a % P == b % P), int(a % P == 0)], (hex(a), hex(b))


def test_invert_and_pow_p58():
    xs = [1, P - 1, 2 * P + 1, 2, P + 2, 2 * P + 2] + UNARY  # 2p + 1 and 2p + 2: the top representatives of 1 and of 2
    inv = D.ints(D.run("fp_invert", rows1(xs), 8))
    p58 = D.ints(D.run("fp_pow_p58", rows1(xs), 8))
    for a, i, e in zip(xs, inv, p58):
        assert i % P == pow(a, P - 2, P) and e % P == pow(a, (P - 5) // 8, P), hex(a)
    assert inv[2] % P == 1 and inv[5] % P == inv[3] % P == pow(2, -1, P)


def test_invsqrt_both_outcomes():
    xs = UNARY
    out = D.run("fp_invsqrt", rows1(xs), 9)
    seen = set()
    for a, o in zip(xs, out):
        ok, r = PG.sqrt_ratio_m1(1, a)
        assert (V.from_limbs(o[:8]) % P, int(o[8])) == (r, int(ok)), hex(a)
        seen.add(bool(ok))
    assert seen == {False, True}


POINTS = V.plain_points() + V.edge_points()


def check_points(out, expected, what):
    for o, (label, pt) in zip(out, expected):
        xy, on = V.affine_of_words(o)
        assert on, (what, label, "X Y != Z T")
        assert xy == V.affine(pt), (what, label)


def test_ge_add_and_double():
    cases = [(a, b) for a in POINTS for b in POINTS[:6] + POINTS[-4:]]
    out = D.run("ge_add", [V.point_words(a[1]) + V.point_words(b[1]) for a, b in cases], 32)
    check_points(out, [(a[0] + "+" + b[0], a[2] + b[2]) for a, b in cases], "ge_add")
    out = D.run("ge_double", [V.point_words(a[1]) for a in POINTS], 32)
    check_points(out, [(a[0], a[2] + a[2]) for a in POINTS], "ge_double")


@pytest.mark.parametrize("neg", [0, 1])
def test_ge_add_niels_and_cached(neg):
    cases = [(a, b) for a in POINTS for b in POINTS[:6] + POINTS[-4:]]
    exp = [(a[0] + "+-"[neg] + b[0], a[2] - b[2] if neg else a[2] + b[2]) for a, b in cases]
    out = D.run("ge_add_niels", [V.point_words(a[1]) + V.niels_words(b[2]) + [neg] for a, b in cases], 32)
    check_points(out, exp, "ge_add_niels")
    out = D.run("ge_add_cached", [V.point_words(a[1]) + V.cached_words(b[1]) + [neg] for a, b in cases], 32)
    check_points(out, exp, "ge_add_cached")


@pytest.mark.parametrize("neg", [0, 1])
def test_table_entries_at_the_top_of_their_range(neg):
    qs = [PG.Pt.identity()] + V.base_points()
    cases = [(a, q) for a in POINTS for q in qs]
    exp = [(a[0], a[2] - q if neg else a[2] + q) for a, q in cases]
    out = D.run("ge_add_niels", [V.point_words(a[1]) + V.niels_words_top(q) + [neg] for a, q in cases], 32)
    check_points(out, exp, "ge_add_niels")
    cases = [(a, b) for a in POINTS for b in V.cached_top_cases()]
    out = D.run("ge_add_cached", [V.point_words(a[1]) + b[1] + [neg] for a, b in cases], 32)
    check_points(out, [(a[0] + b[0], a[2] - b[2] if neg else a[2] + b[2]) for a, b in cases], "ge_add_cached")


def test_ge_compress_of_non_canonical_coordinates():
    out = D.run("ge_compress", [V.point_words(a[1]) for a in POINTS], 8)
    for a, o in zip(POINTS, out):
        assert V.from_limbs(o).to_bytes(32, "little") == a[2].encode(), a[0]


def decode_steps(s):
    """RFC 9496 4.3.1 on a canonical even s, step by step: (was_square, x was negated, t is negative, y == 0)"""
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2s = u2 * u2 % P
    v = (-(PG.D * u1 % P * u1) - u2s) % P
    ok, invsqrt = PG.sqrt_ratio_m1(1, v * u2s % P)
    den_x = invsqrt * u2 % P
    x0 = 2 * s * den_x % P
    x = P - x0 if x0 & 1 else x0
    y = u1 * (invsqrt * den_x % P * v % P) % P
    return ok, bool(x0 & 1), bool((x * y % P) & 1), y == 0


def test_ge_decompress():
    good = [int.from_bytes(a[2].encode(), "little") for a in POINTS] + [0]
    good += [int.from_bytes((k * PG.basepoint()).encode(), "little") for k in range(3, 40)]
    good = sorted(set(good))
    # what must not decode: non-canonical even encodings (s + p, p + 2, 2^255 - 1 + ... ), bit 255 set, negative (odd) ones,
    # y == 0 (s = p - 1), and small even s that fail the square test or give a negative t
    bad = [s + P for s in good if s + P < B256] + [s + 2**255 for s in good[:6]] + [P, P + 2, 2**255 - 1, 2**255 - 2, 2**255,
                                                                                  B256 - 1, B256 - 2, 1, 3, P - 1, P - 2]
    small = list(range(2, 200, 2))  # some of these decode, the others fail the square test or give a negative t
    bad += [s + 1 for s in good[:4]] + small
    xs = good + bad
    out = D.run("ge_decompress", rows1(xs), 33)
    for s, o in zip(xs, out):
        pt = PG.decode(s.to_bytes(32, "little"))
        assert int(o[32]) == int(pt is not None), hex(s)
        if pt is not None:
            X, Y, Z, T = (V.from_limbs(o[8 * i:8 * i + 8]) % P for i in range(4))
            assert (X, Y, Z, T) == (pt.X, pt.Y, pt.Z, pt.T), hex(s)
    assert all(int(o[32]) == 1 for o in out[:len(good)]) and not any(int(o[32]) for o in out[len(good):len(xs) - len(small)])
    # the vectors reach every way out of the function
    assert {decode_steps(s)[1] for s in good if s} == {False, True}, "x negated and not"
    assert decode_steps(P - 1)[3] and PG.decode((P - 1).to_bytes(32, "little")) is None, "y == 0"
    steps = [decode_steps(s) for s in small]
    assert any(not st[0] for st in steps) and any(st[0] and st[2] for st in steps), "not a square; t negative"


@pytest.mark.parametrize("n,split", [(64, 0), (64, 16), (64, 1), (256, 0), (256, 64), (256, 128)])
def test_ge_tree_quad(n, split):
    B = PG.basepoint()
    pts, acc = [], PG.Pt.identity()
    for i in range(n):
        acc = acc + B
        pts.append(acc)
    reps = [[pt.X, pt.Y, pt.Z, pt.T] if i % 3 else [pt.X + P, pt.Y, pt.Z + P, pt.T + P] for i, pt in enumerate(pts)]
    for k, e in enumerate(V.edge_points()):  # representatives at the top of the range, the identity and repeats among them
        reps[(5 * k + 2) % n], pts[(5 * k + 2) % n] = e[1], e[2]
    reps[7], pts[7] = reps[6], pts[6]
    out = D.run(f"ge_tree_quad{n}", [[w for r in reps for w in V.point_words(r)] + [split]], 64)[0]
    total = [PG.Pt.identity(), PG.Pt.identity()]
    for i, pt in enumerate(pts):
        total[1 if i & split else 0] = total[1 if i & split else 0] + pt
    check_points([out[:32]], [("sh[0]", total[0])], "ge_tree_quad")
    if split:
        check_points([out[32:]], [("sh[split]", total[1])], "ge_tree_quad")
