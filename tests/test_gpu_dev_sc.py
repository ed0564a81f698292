"""sc_dev.h's shared sum-check pieces on the GPU (block_sum, take_pd, the pair bodies) through tests/devarith/devarith.hip;
every comparison is exact, against plain integer arithmetic mod q on the Montgomery images the kernels see."""
import random

import pytest

import devarith_lib as D
import limb_vectors as V

pytestmark = pytest.mark.gpu
Q = V.Q
SPECIAL = [0, 1, Q - 1, Q - 2, (Q - 1) // 2]
LOAD, FOLD, FOLD_C, FOLD_TO = 0, 1, 2, 3  # sc_dev.h PdMode


def mul(a, b):
    return V.fq_mont_mul(a, b)


def draw(rng, nonzero=False):
    """one of the special values or, half of the time, a random element"""
    while True:
        v = rng.randrange(Q) if rng.random() < 0.5 else rng.choice(SPECIAL)
        if v or not nonzero:
            return v


def const_words(r):
    """the 64 words tt[k][i] of make_fq_const(r): limb k of T_i = r * 2^(32 i) * 2^-256 mod q"""
    T = [V.limbs(r * (1 << (32 * i)) * V.RINV % Q) for i in range(8)]
    return [T[i][k] for k in range(8) for i in range(8)]


def words(xs):
    return [w for x in xs for w in V.limbs(x)]


# ---- block_sum ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads,ne", [(256, 2), (256, 3), (512, 2), (512, 3)])
def test_block_sum(threads, ne):
    rng = random.Random(threads * 10 + ne)
    cases = []
    for nw in (1, 2, threads // 64):
        for kind in ("mixed", "all q-1"):
            # waves at and above nw hold non-zero values: the result must leave them out
            sets = [[[Q - 1 if kind == "all q-1" else draw(rng, nonzero=t >= 64 * nw) for _ in range(ne)] for t in range(threads)]
                    for _ in range(2)]
            cases.append((nw, sets))
    out = D.run(f"block_sum_{ne}_{threads}", [[nw] + words(v for s in sets for t in s for v in t) for nw, sets in cases], 16 * ne)
    for (nw, sets), o in zip(cases, out):
        got = D.ints(o.reshape(2 * ne, 8))
        want = [sum(t[k] for t in s[:64 * nw]) % Q for s in sets for k in range(ne)]
        assert got == want, (threads, ne, nw, "first and second call")


# ---- take_pd --------------------------------------------------------------------------------------------------------------

def fold_model(T, q, r):
    lo = [(T[i] + mul(r, (T[2 * q + i] - T[i]) % Q)) % Q for i in range(q)]
    hi = [(T[q + i] + mul(r, (T[3 * q + i] - T[q + i]) % Q)) % Q for i in range(q)]
    return lo, hi


@pytest.mark.parametrize("q", [1, 3, 64])
def test_take_pd(q):
    rng = random.Random(q)
    rs = [0, 1, Q - 1, rng.randrange(Q)]
    tables = {r: [draw(rng) for _ in range(4 * q)] for r in rs}  # one table per r, the same for every mode
    cases = [(mode, r, tables[r]) for r in rs for mode in range(5)]  # 4: PD_FOLD_TO with dst == src
    rows = [[mode, q, 0, 0] + V.limbs(r) + const_words(r) + words(T) + [0] * (8 * (256 - 4 * q)) for mode, r, T in cases]
    out = D.run("take_pd", rows, 4096)
    results = {}
    for (mode, r, T), o in zip(cases, out):
        tab = D.ints(o[:2048].reshape(256, 8))[:4 * q]
        dst = D.ints(o[2048:3072].reshape(128, 8))[:2 * q]
        pd = D.ints(o[3072:].reshape(128, 8))
        p, d = pd[0:2 * q:2], pd[1:2 * q:2]
        lo, hi = fold_model(T, q, r)
        if mode == LOAD:
            assert p == T[:q] and d == [(T[q + i] - T[i]) % Q for i in range(q)], (q, hex(r))
            assert tab == T, "PD_LOAD wrote to the table"
            continue
        assert p == lo and d == [(h - l) % Q for h, l in zip(hi, lo)], (q, mode, hex(r))
        if mode == FOLD_TO:
            assert tab == T, "PD_FOLD_TO with another destination touched its source"
            assert dst == lo + hi, (q, hex(r))
        else:
            assert tab == lo + hi + T[2 * q:], (q, mode, hex(r))
        results[(mode, r)] = (p, d)
    for r in rs:
        assert results[(FOLD_C, r)] == results[(FOLD, r)], "the constant form differs from the plain form"
        assert results[(4, r)] == results[(FOLD, r)], "PD_FOLD_TO in place differs from PD_FOLD"


# ---- pair bodies ----------------------------------------------------------------------------------------------------------

KTAB2, KTAB4, PHASE1, PHASE1_LEAD, PROD, PROD_LEAD_NOW, PROD_LEAD_ACC, DOTP = range(8)
NTAB = {KTAB2: 2, KTAB4: 4, PHASE1: 3, PHASE1_LEAD: 3, PROD: 2, PROD_LEAD_NOW: 2, PROD_LEAD_ACC: 2, DOTP: 3}
# every (body, mode) a kernel instantiates
VARIANTS = [(KTAB2, LOAD), (KTAB2, FOLD), (KTAB4, LOAD), (KTAB4, FOLD),
            (PHASE1, LOAD), (PHASE1, FOLD), (PHASE1_LEAD, LOAD), (PHASE1_LEAD, FOLD), (PHASE1_LEAD, FOLD_C),
            (PROD, LOAD), (PROD, FOLD), (PROD_LEAD_NOW, LOAD), (PROD_LEAD_NOW, FOLD), (PROD_LEAD_NOW, FOLD_C),
            (PROD_LEAD_ACC, LOAD), (PROD_LEAD_ACC, FOLD_C), (DOTP, LOAD), (DOTP, FOLD_TO)]


def body_model(body, mode, n, r, E, tabs):
    """the sums of sc_dev.h's comments over pairs 0..n-1, and the tables afterwards"""
    e = [0, 0, 0]
    after = [list(t) for t in tabs]
    for i in range(n):
        pd = []
        for k, T in enumerate(tabs):
            if mode == LOAD:
                p, hi = T[i], T[n + i]
            else:
                p = (T[i] + mul(r, (T[2 * n + i] - T[i]) % Q)) % Q
                hi = (T[n + i] + mul(r, (T[3 * n + i] - T[n + i]) % Q)) % Q
                after[k][i], after[k][n + i] = p, hi
            pd.append((p, (hi - p) % Q))
        at = lambda k, x: (pd[k][0] + x * pd[k][1]) % Q  # table k's line at x
        if body == KTAB2:  # A*B at x = 0, 2
            for s, x in enumerate((0, 2)):
                e[s] += mul(at(0, x), at(1, x))
        elif body == KTAB4:  # A*(B*C - D) at x = 0, 2, 3
            for s, x in enumerate((0, 2, 3)):
                e[s] += mul(at(0, x), (mul(at(1, x), at(2, x)) - at(3, x)) % Q)
        elif body == PHASE1:  # E*(B*C - D) at x = 0, 2, 3
            for s, x in enumerate((0, 2, 3)):
                e[s] += mul(E[i], (mul(at(0, x), at(1, x)) - at(2, x)) % Q)
        elif body == PHASE1_LEAD:  # t(0), the x^2 coefficient and, unfolded, t(1)
            e[0] += mul(E[i], (mul(at(0, 0), at(1, 0)) - at(2, 0)) % Q)
            e[1] += mul(E[i], mul(pd[0][1], pd[1][1]))
            if mode == LOAD:
                e[2] += mul(E[i], (mul(at(0, 1), at(1, 1)) - at(2, 1)) % Q)
        elif body == PROD:  # E*A*B at x = 0, 2, 3
            for s, x in enumerate((0, 2, 3)):
                e[s] += mul(E[i], mul(at(0, x), at(1, x)))
        elif body in (PROD_LEAD_NOW, PROD_LEAD_ACC):  # t(0) and the x^2 coefficient
            e[0] += mul(E[i], mul(at(0, 0), at(1, 0)))
            e[1] += mul(E[i], mul(pd[0][1], pd[1][1]))
        else:  # L*R*W at x = 0, 2, 3
            for s, x in enumerate((0, 2, 3)):
                e[s] += mul(at(2, x), mul(at(0, x), at(1, x)))
    return [v % Q for v in e], after


def body_cases():
    rng = random.Random(25)
    cases = []
    for body, mode in VARIANTS:
        # one pair per lane on the special operands; LeadAcc also 7, 8 and 15 pairs (the every-seventh flush, the final one)
        counts = [1] * 24 + ([7, 8, 15] * 3 if body == PROD_LEAD_ACC else [2, 15])
        for j, n in enumerate(counts):
            special = j < 12  # half of the one-pair lanes on special values alone
            pick = (lambda: rng.choice(SPECIAL)) if special else (lambda: draw(rng))
            used = (2 if mode == LOAD else 4) * n
            tabs = [[pick() for _ in range(used)] for _ in range(NTAB[body])]
            cases.append((body, mode, n, pick() if special else rng.randrange(Q), [pick() for _ in range(n)], tabs))
    return cases


@pytest.mark.parametrize("lane,lane_mode", [("load", LOAD), ("fold", FOLD), ("fold_c", FOLD_C), ("fold_to", FOLD_TO)])
def test_pair_bodies(lane, lane_mode):
    cases = [c for c in body_cases() if c[1] == lane_mode]  # one lane kernel per fold mode
    rows = []
    for body, mode, n, r, E, tabs in cases:
        row = [body, 0, n, 0] + V.limbs(r) + const_words(r) + words(E) + [0] * (8 * (15 - n))
        for k in range(4):
            T = tabs[k] if k < len(tabs) else []
            row += words(T) + [0] * (8 * (60 - len(T)))
        rows.append(row)
    out = D.run("sc_body_" + lane, rows, 2672)
    for (body, mode, n, r, E, tabs), o in zip(cases, out):
        want, after = body_model(body, mode, n, r, E, tabs)
        ne = 2 if body == KTAB2 else 3
        got = D.ints(o[:8 * ne].reshape(ne, 8))
        assert got == want[:ne], (body, mode, n, hex(r))
        got_tabs = D.ints(o[32:32 + 1920].reshape(240, 8))
        if body == DOTP and mode == FOLD_TO:  # folded into the destination tables, the sources as they were
            dst = D.ints(o[1952:].reshape(90, 8))
            for k, T in enumerate(tabs):
                assert got_tabs[60 * k:60 * k + len(T)] == T, (body, n, "source table", k)
                assert dst[30 * k:30 * k + 2 * n] == after[k][:2 * n], (body, n, "destination table", k)
        else:
            for k, T in enumerate(after):
                assert got_tabs[60 * k:60 * k + len(T)] == T, (body, mode, n, "table", k)
