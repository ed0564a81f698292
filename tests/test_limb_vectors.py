"""The vector sets of limb_vectors.py reach what they are meant to reach.  Evaluated from the integer reference alone, on the
CPU: these are requirements on the vectors, not measurements of the code under test."""
import limb_vectors as V
import pymodel_group as PG

P, Q, B256 = V.P, V.Q, V.B256


def test_seed_sets():
    assert 20 <= len(V.FQ_SEEDS) <= 48 and 36 <= len(V.FP_SEEDS) <= 56
    assert len(set(V.FQ_SEEDS)) == len(V.FQ_SEEDS) and len(set(V.FP_SEEDS)) == len(V.FP_SEEDS)
    for x in (0, 1, 2, 2**252 - 1, 2**252, 2**252 + 1, Q - 2, Q - 1, V.R, V.R2, 0xFFFFFFFF, 0xFFFFFFFF << 192):
        assert x in V.FQ_SEEDS and x in V.FP_SEEDS
    for x in (18, 19, 37, 38, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**255 - 1, 2**255, B256 - 39, B256 - 38, B256 - 1):
        assert x in V.FP_SEEDS
    assert len(V.FQ_PAIRS) == len(V.FQ_SEEDS) ** 2 + 4096 and len(V.FP_PAIRS) == len(V.FP_SEEDS) ** 2 + 4096
    assert all(a < Q and b < Q for a, b in V.FQ_PAIRS) and all(a < B256 and b < B256 for a, b in V.FP_PAIRS)


def test_fp_add_sub_reach_every_wrap():
    assert {V.fp_add_wraps(a, b) for a, b in V.FP_PAIRS} == {0, 1, 2}
    assert V.fp_add_wraps(B256 - 1, B256 - 1) == 2 and (B256 - 1, B256 - 1) in V.FP_PAIRS
    assert {V.fp_sub_borrows(a, b) for a, b in V.FP_PAIRS} == {0, 1, 2}
    assert V.fp_sub_borrows(0, B256 - 1) == 2 and (0, B256 - 1) in V.FP_PAIRS


def test_fp_mul_reaches_both_ends_of_the_fold():
    carries = {V.fp_mul_fold_carry(a, b) for a, b in V.FP_PAIRS}
    assert (B256 - 1, B256 - 1) in V.FP_PAIRS
    assert V.fp_mul_fold_carry(B256 - 1, B256 - 1) == 37 and V.FP_MUL_MAX_FOLD_CARRY == max(carries) and 0 in carries
    # the last fold wraps a second time for some pair of the set as well
    assert any(((a * b % B256) + 38 * (a * b >> 256)) % B256 + 38 * V.fp_mul_fold_carry(a, b) >= B256 for a, b in V.FP_PAIRS)


def test_fp_freeze_ranges_and_gaps():
    assert {V.fp_range(a) for a in V.FP_SEEDS} == {0, 1, 2}
    assert all(a in V.FP_SEEDS for a in V.FP_FREEZE_EDGES)
    for boundary in (P, 2 * P):
        assert boundary - 1 in V.FP_SEEDS and boundary in V.FP_SEEDS and boundary + 1 in V.FP_SEEDS
    assert 2**255 - 1 in V.FP_SEEDS and 2**255 in V.FP_SEEDS  # a + 19 on each side of 2^255
    assert B256 - 39 == 2 * P - 1 and B256 - 1 in V.FP_SEEDS    # ... and of 2^256


def test_fq_sums_and_differences():
    sums = {a + b for a, b in V.FQ_PAIRS}
    assert {Q - 1, Q, Q + 1, 2 * Q - 2} <= sums
    diffs = {a - b for a, b in V.FQ_PAIRS}
    assert {0, -1, -(Q - 1)} <= diffs
    assert {Q - 1, Q, Q + 1, 2 * Q - 2, 0} <= set(V.FQ_COND_SUB_INPUTS) and max(V.FQ_COND_SUB_INPUTS) < 2 * Q


def test_fqw_cases():
    cases = V.fqw_cases()
    assert {len(c) for c in cases} == set(range(1, 8))
    assert [(Q - 1, Q - 1)] * 7 in cases
    assert all(V.fqw_sum(c) < B256 * Q for c in cases)  # the contract of fqw_reduce; eight products would break it
    tops = {V.fqw_sum(c) >> 480 != 0 for c in cases}
    assert tops == {False, True}
    assert all(V.fqw_sum(c) * V.RINV % Q == sum(V.fq_mont_mul(a, b) for a, b in c) % Q for c in cases)


def test_fq_const_cases():
    cases = V.fq_const_cases()
    top = [Q - 1] * 8
    assert (Q - 1, top) in cases and (2**252 - 1, top) in cases
    assert max(V.fq_const_S(d, T) for d, T in cases) == V.fq_const_S(2**252 - 1, top) < 2**288
    assert {V.fq_const_borrows(d, T) for d, T in cases} == {False, True}
    assert {(V.fq_const_S(d, T) >> 284) != 0 for d, T in cases} == {False, True}  # h1
    assert all(d < Q and all(t < Q for t in T) for d, T in cases)


def test_window_shapes():
    assert {c for c, W, wide in V.WINDOW_SHAPES if wide == W} >= {9, 10, 11, 12}
    for c, W, wide in V.WINDOW_SHAPES:
        ws = V.window_widths(c, W, wide)
        assert sum(ws) >= 253 and min(ws) >= 3 and max(ws) <= 13
        sc = V.window_scalars(c, W, wide)
        assert {0, 1, Q - 1} <= set(sc) and all(s < Q for s in sc)


def test_fe10_cases():
    cases = V.fe10_mul_cases()
    assert (V.fe10_max(4), V.fe10_max(3)) in cases
    assert max(V.fe10_column_max(f, g) for f, g in cases) == V.fe10_column_max(V.fe10_max(4), V.fe10_max(3)) < 2**64
    assert all(19 * max(g) < 2**32 for f, g in cases)
    assert any(V.fe10_is_1x(f) and V.fe10_is_1x(g) for f, g in cases)
    for a in V.FP_SEEDS:
        assert V.fe10_value(V.fe10_split(a)) == a
    sub = V.fe10_sub_cases()
    for i in range(10):
        assert ([0] * 10, [V.FE10_1X[k] if k == i else 0 for k in range(10)]) in sub
    assert all(V.fe10_is_1x(b) for a, b in sub)
    assert all(bias >= m for bias, m in zip(V.FE10_SUB_BIAS, V.FE10_1X))  # the bias covers a 1x second operand
    assert V.fe10_value(V.FE10_SUB_BIAS) == 2 * P


def test_edge_points():
    pts = V.edge_points()
    assert pts[0][1] == [2 * P, 1, 1, 0] and pts[1][1] == [P, 1, 1, 0]
    seen = set()
    for label, rep, pt in pts:
        assert all(0 <= x < B256 for x in rep)
        assert rep[0] * rep[1] % P == rep[2] * rep[3] % P
        assert PG.Pt(*rep) == pt and (rep[0] * pt.Z - pt.X * rep[2]) % P == 0 and (rep[1] * pt.Z - pt.Y * rep[2]) % P == 0
        nine = [V.fe10_split(x)[9] for x in rep]
        for i, n in enumerate(V.COORDS):
            if label.endswith("-" + n):
                partner = V.COORDS.index(V._PARTNER[n])
                assert nine[i] == 2**26 - 1 and nine[partner] == 0
                seen.add(n)
    assert seen == set(V.COORDS)
    assert V.fe10_split(2 * P)[9] == 2**26 - 1


def test_table_entries_at_the_top_of_their_range():
    nine = lambda ws, i: V.fe10_split(V.from_limbs(ws[8 * i:8 * i + 8]))[9]
    ident = V.niels_words_top(PG.Pt.identity())
    assert [V.from_limbs(ident[8 * i:8 * i + 8]) for i in range(3)] == [2 * P + 1, 2 * P + 1, 2 * P]
    assert all(nine(ident, i) == 2**26 - 1 for i in range(3))
    for pt in V.base_points():
        ws = V.niels_words_top(pt)
        assert all(nine(ws, i) >= 2**25 for i in range(3))  # bit 255 set: beyond 1x on limb 9
        x, y = V.affine(pt)
        assert [V.from_limbs(ws[8 * i:8 * i + 8]) % P for i in range(3)] == [(y + x) % P, (y - x) % P, 2 * PG.D * x * y % P]
    for label, ws, pt in V.cached_top_cases():
        e = [V.from_limbs(ws[8 * i:8 * i + 8]) for i in range(4)]
        assert nine(ws, 0) == 2**26 - 1 and all(nine(ws, i) >= 2**25 for i in range(4)) and all(x < B256 for x in e)
        X, Y = (e[0] - e[1]) * pow(2, -1, P) % P, (e[0] + e[1]) * pow(2, -1, P) % P
        assert PG.Pt(X, Y, e[2], X * Y * pow(e[2], -1, P)) == pt and e[3] % P == 2 * PG.D * X * Y * pow(e[2], -1, P) % P
