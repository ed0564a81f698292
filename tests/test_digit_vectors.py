"""The vectors of digit_vectors.py are what their names say, the two restated recoders of msm.hip agree on them, and the set
tells carry_into from its plausible mistakes at every lane boundary.  Evaluated from Python integers alone, on the CPU: these
are requirements on the vectors and on the recoding scheme, not measurements of the code under test."""
import pytest

import digit_vectors as D

Q = D.Q


@pytest.fixture(scope="module")
def sets():
    return {c: D.edge_scalars(c, D.windows(c)) for c in D.WIDTHS}


def test_geometry_of_the_widths_the_gpu_tests_use():
    assert [(c, D.windows(c), D.lane_windows(D.windows(c))) for c in (12, 8, 7)] == [(12, 22, 3), (8, 32, 4), (7, 37, 5)]
    assert D.lane_boundaries(12, 22) == [3, 6, 9, 12, 15, 18]
    assert D.lane_boundaries(8, 32) == [4, 8, 12, 16, 20, 24, 28]
    assert D.lane_boundaries(7, 37) == [5, 10, 15, 20, 25, 30, 35]   # lane 7 holds windows 35, 36 only


def test_scalar_digit_is_the_plain_shift():
    for c in D.WIDTHS:
        for s in (Q - 1, (1 << 256) - 1, 0x0123456789ABCDEF << 190):
            for w in range(D.windows(c)):
                assert D.scalar_digit(s, w, c) == (s >> (c * w)) & ((1 << c) - 1)


def test_every_vector_is_a_nonzero_scalar_and_named_once(sets):
    for c, vs in sets.items():
        assert all(0 < v.s < Q for v in vs), c
        assert len({v.s for v in vs}) == len(vs) and len({v.name for v in vs}) == len(vs), c
        assert 60 <= len(vs) <= 160, (c, len(vs))   # a row each on the GPU: the list stays short


def test_required_vectors_are_present(sets):
    for c, vs in sets.items():
        W, half, wpg = D.windows(c), 1 << (c - 1), D.lane_windows(D.windows(c))
        have = {v.s for v in vs}
        base = [1, half, half + 1, (1 << c) - 1, 1 << c, (1 << 250) - 1, (Q - 1) // 2, (Q + 1) // 2, (1 << 251) - 1, 1 << 251,
                (1 << 251) + 1, Q - (1 << 251), Q - (1 << 251) + 1, Q - 1]
        nfull = 251 // c
        base += [sum(half << (c * w) for w in range(nfull)), sum((half + 1) << (c * w) for w in range(nfull))]
        for b in D.lane_boundaries(c, W):
            base.append(sum(half << (c * w) for w in range(b)))
            for k in {1, 2, wpg}:
                if b - k >= 1:
                    run = sum(half << (c * w) for w in range(b - k, b))
                    for below in (half + 1, half - 1):
                        base.append(run + (below << (c * (b - k - 1))) + (1 << (c * b)))
        for x in base:
            assert x in have and (Q - x) % Q in have, (c, hex(x))


def test_names_are_true(sets):
    for c, vs in sets.items():
        W = D.windows(c)
        for v in vs:
            folded, flip = D.fold(v.s)
            assert (folded, flip) == (v.folded, v.flip), (c, v.name)
            assert folded <= Q - (1 << 251) < (1 << 252), (c, v.name)   # the largest value a walk sees: bit 251 and 125 bits below
            if v.digits is not None:
                assert [D.scalar_digit(folded, w, c) for w in range(W)] == [v.digits.get(w, 0) for w in range(W)], (c, v.name)
        by = {v.name: v for v in vs}
        half = 1 << (c - 1)
        # the names that promise an effect on the walk rather than digits
        d, carry = D.recode_walk(by["2^250-1"].s, c, W)
        top = 250 // c
        assert d[0] == -1 and all(x == 0 for x in d[1:top]) and d[top] == 1 << (250 - c * top) and carry == 0, c
        d, _ = D.recode_walk(by["every digit below bit 251 = half"].s, c, W)
        assert d == [half] * (251 // c) + [0] * (W - 251 // c), c            # exactly half stays positive, no carry anywhere
        d, _ = D.recode_walk(by["every digit below bit 251 = half+1"].s, c, W)
        assert d[0] == -(half - 1) and all(x == -(half - 2) for x in d[1:251 // c]) and d[251 // c] == 1, c   # the carry ripples to the top
        for name in ("2^251", "2^251+1"):                                      # the folded value carries bit 251 into the top windows
            assert by[name].flip and by[name].folded >> 251 == 1
        assert by["q-2^251"].folded == 1 << 251


def test_recoders_rebuild_the_scalar_and_agree(sets):
    for c, vs in sets.items():
        W, half = D.windows(c), 1 << (c - 1)
        for v in vs:
            walk, carry_w = D.recode_walk(v.s, c, W)
            lanes, carry_l = D.recode_lanes(v.s, c, W)
            assert len(walk) == len(lanes) == W
            assert walk == lanes, (c, v.name)
            assert carry_w == 0 and carry_l == 0, (c, v.name)
            assert max(abs(x) for x in walk) <= half, (c, v.name)
            assert sum(x << (c * w) for w, x in enumerate(walk)) % Q == v.s, (c, v.name)
            if v.flip and Q - v.s < D.FOLD:   # the same magnitudes as the unfolded twin, every sign flipped
                assert walk == [-x for x in D.recode_walk(Q - v.s, c, W)[0]], (c, v.name)


def test_each_wrong_carry_rule_is_caught_at_every_lane_boundary(sets):
    """the cap that keeps the list from thinning out: for every lane boundary and every wrong rule some vector's digits at
    that boundary's lane differ -- on both sides of the fold"""
    for c, vs in sets.items():
        W, wpg = D.windows(c), D.lane_windows(D.windows(c))
        bounds = D.lane_boundaries(c, W)
        assert bounds and bounds[0] == wpg
        right = [D.recode_lanes(v.s, c, W)[0] for v in vs]
        for rule in D.WRONG_CARRY_RULES:
            wrong = [D.recode_lanes(v.s, c, W, rule)[0] for v in vs]
            for b in bounds:
                for flip in (False, True):
                    hit = [v.name for v, r, x in zip(vs, right, wrong) if v.flip == flip and r[b:b + wpg] != x[b:b + wpg]]
                    assert hit, (c, rule.__name__, b, flip)
            assert sum(r != x for r, x in zip(right, wrong)) >= 2 * len(bounds), (c, rule.__name__)
