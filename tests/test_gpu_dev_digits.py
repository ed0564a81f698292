"""The signed-digit recoders of ge_tree_dev.h on the GPU, digit by digit through tests/devarith/devarith.hip: the table walks'
(fq_fold_sign, fq_take_window, walk_digit; scalar_digit and carry_into for the lane-split form) against
tests/digit_vectors.recode_walk / recode_lanes on edge_scalars(c, W), and the row table's row_digit against the restatement
tests/test_gpu_row_table.py counts additions with.  One launch of one workgroup per case; the comparison is exact."""
import numpy as np
import pytest

import devarith_lib as D
import digit_vectors as DV
import limb_vectors as V
from test_gpu_row_table import Q, edge_scalars as row_edge_scalars, model_additions, windows as row_windows

pytestmark = pytest.mark.gpu


def sign_mag(d):
    """a signed digit as the harness writes it: magnitude, sign in bit 15"""
    return -d | 0x8000 if d < 0 else d


@pytest.mark.parametrize("c", [7, 8, 12])
def test_walk_digits(c):
    W = DV.windows(c)
    vecs = DV.edge_scalars(c, W)
    out = D.run("walk_digits", [V.limbs(v.s) + [c, W] for v in vecs], 45)
    for v, o in zip(vecs, out):
        digits, carry = DV.recode_walk(v.s, c, W)
        assert [int(x) for x in o[:W]] == [sign_mag(d) for d in digits], (c, v.name)
        assert not any(o[W:44]) and int(o[44]) == carry, (c, v.name)


@pytest.mark.parametrize("c", [7, 8, 12])
def test_walk_lane_digits_and_carry_into(c):
    W = DV.windows(c)
    wpg = DV.lane_windows(W)
    vecs = DV.edge_scalars(c, W)
    out = D.run("walk_lane_digits", [V.limbs(v.s) + [c, W] for v in vecs], 53)
    for v, o in zip(vecs, out):
        digits, carry = DV.recode_lanes(v.s, c, W)
        assert [int(x) for x in o[:W]] == [sign_mag(d) for d in digits], (c, v.name)
        assert not any(o[W:44]) and int(o[44]) == carry, (c, v.name)
        exp = [DV.carry_into(v.folded, lane * wpg, c) if lane * wpg < W else 0 for lane in range(DV.LANES)]
        assert [int(x) for x in o[45:53]] == exp, (c, v.name)


def row_digit_words(s, c):
    """row_digit as tests/test_gpu_row_table.model_additions restates it, the digit words written out: (W words, last carry)"""
    W, half, fullw = row_windows(c), 1 << (c - 1), 1 << c
    flip = s >= (1 << 251)
    if flip:
        s = Q - s
    carry, out = 0, []
    for w in range(W):
        v = (s & (fullw - 1)) + carry
        s >>= c
        neg = w != W - 1 and (v >= half if flip else v > half)
        mag = fullw - v if neg else v
        carry = 1 if neg else 0
        out.append(0xFFFF if mag == 0 else (mag - 1) | (0x8000 if neg != flip else 0))
    return out, carry


@pytest.mark.parametrize("c", [13, 16])
def test_row_digits(c):
    W = row_windows(c)
    rng = np.random.default_rng(c)
    scalars = row_edge_scalars(c) + [int.from_bytes(rng.bytes(32), "little") % Q for _ in range(200)]
    out = D.run("row_digits", [V.limbs(s) + [c, W] for s in scalars], 66)
    for s, o in zip(scalars, out):
        words, carry = row_digit_words(s, c)
        got = [int(x) for x in o[:W]]
        assert got == words, hex(s)
        assert not any(o[W:64]) and int(o[64]) == carry == 0 and int(o[65]) == 0, (hex(s), "carry or scalar bits left over")
        assert sum(w != 0xFFFF for w in got) == model_additions(s, c), hex(s)
        # the words decode to digits that recombine to s (mod q: a folded scalar's digits are those of s - q)
        val = [0 if w == 0xFFFF else (-1 if w & 0x8000 else 1) * ((w & 0x7FFF) + 1) for w in got]
        assert sum(d << (c * k) for k, d in enumerate(val)) % Q == s, hex(s)
