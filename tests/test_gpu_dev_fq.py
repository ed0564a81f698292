"""fq_dev.h and ge_tree_dev.h's fq_signed_window on the GPU, function by function through tests/devarith/devarith.hip, on the
limb patterns of limb_vectors.py; every comparison is exact, against plain integer arithmetic."""
import pytest

import devarith_lib as D
import limb_vectors as V

pytestmark = pytest.mark.gpu
Q = V.Q
UNARY = V.FQ_SEEDS + [a for a, _ in V.FQ_PAIRS[-256:]]


def rows2(pairs):
    return [V.limbs(a) + V.limbs(b) for a, b in pairs]


def rows1(xs):
    return [V.limbs(a) for a in xs]


@pytest.mark.parametrize("name,ref", [("fq_add", lambda a, b: (a + b) % Q), ("fq_sub", lambda a, b: (a - b) % Q),
                                      ("fq_mul", V.fq_mont_mul)])
def test_binary(name, ref):
    got = D.ints(D.run(name, rows2(V.FQ_PAIRS), 8))
    bad = [(hex(a), hex(b), hex(g)) for (a, b), g in zip(V.FQ_PAIRS, got) if g != ref(a, b)]
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("name,ref", [("fq_neg", lambda a: (-a) % Q), ("fq_dbl", lambda a: 2 * a % Q),
                                      ("fq_sqr", lambda a: V.fq_mont_mul(a, a)), ("fq_from_mont", lambda a: a * V.RINV % Q)])
def test_unary(name, ref):
    got = D.ints(D.run(name, rows1(UNARY), 8))
    bad = [(hex(a), hex(g)) for a, g in zip(UNARY, got) if g != ref(a)]
    assert not bad, (len(bad), bad[:4])


def test_from_mont_of_any_256_bit_pattern():
    got = D.ints(D.run("fq_from_mont", rows1(V.FP_SEEDS), 8))
    assert got == [a * V.RINV % Q for a in V.FP_SEEDS]


def test_cond_sub_q():
    xs = V.FQ_COND_SUB_INPUTS
    got = D.ints(D.run("fq_cond_sub_q", rows1(xs), 8))
    assert got == [t - Q if t >= Q else t for t in xs]


def test_fqw_mac_reduce():
    cases = V.fqw_cases()
    rows = []
    for c in cases:
        r = [len(c)]
        for a, b in c + [(0, 0)] * (7 - len(c)):
            r += V.limbs(a) + V.limbs(b)
        rows.append(r)
    out = D.run("fqw_mac_reduce", rows, 24)
    flat = [p for c in cases for p in c]
    single = D.ints(D.run("fq_mul", rows2(flat), 8))
    at = 0
    for c, o in zip(cases, out):
        S = V.fqw_sum(c)
        assert V.from_limbs(o[8:24]) == S, (c, "the sixteen-limb sum")
        assert V.from_limbs(o[:8]) == S * V.RINV % Q, c
        assert V.from_limbs(o[:8]) == sum(single[at:at + len(c)]) % Q, (c, "differs from the sum of the fq_mul results")
        at += len(c)


def test_fq_mul_const():
    cases = V.fq_const_cases()
    got = D.ints(D.run("fq_mul_const", [V.limbs(d) + [w for t in T for w in V.limbs(t)] for d, T in cases], 8))
    bad = [(hex(d), [hex(t) for t in T], hex(g)) for (d, T), g in zip(cases, got) if g != V.fq_const_S(d, T) % Q]
    assert not bad, (len(bad), bad[:2])


def test_fq_mul_const_with_the_hosts_constants():
    ds = V.FQ_SEEDS
    for r in V.FQ_SEEDS:
        got = D.ints(D.run_mul_const_host(V.limbs(r), rows1(ds)))
        assert got == [V.fq_mont_mul(r, d) for d in ds], hex(r)
        assert got == D.ints(D.run("fq_mul", rows2([(r, d) for d in ds]), 8)), hex(r)


def test_fq_wave_sum():
    rnd = [a for a, _ in V.FQ_PAIRS[-64:]]
    waves = [[Q - 1] * 64, [V.FQ_SEEDS[i % len(V.FQ_SEEDS)] for i in range(64)], rnd, [0] * 63 + [Q - 1], [1] + [0] * 63,
             [Q - 1 if i & 1 else 1 for i in range(64)]]
    out = D.run("fq_wave_sum", [[w for a in wave for w in V.limbs(a)] for wave in waves], 512)
    for wave, o in zip(waves, out):
        lanes = D.ints(o.reshape(64, 8))
        assert lanes == [sum(wave) % Q] * 64


@pytest.mark.parametrize("c,W,wide", V.WINDOW_SHAPES)
def test_fq_signed_window(c, W, wide):
    ws = V.window_widths(c, W, wide)
    offs = [sum(ws[:w]) for w in range(W)]
    scalars = V.window_scalars(c, W, wide)
    out = D.run("fq_signed_window", [V.limbs(s) + [c, W, wide] for s in scalars], 90)
    for s, o in zip(scalars, out):
        digs = [int(x) for x in o[:W]]
        assert all(d < 1 << 16 for d in digs) and not any(o[W:88]), hex(s)  # sign and 15 bits of magnitude, nothing above
        val = [-(d & 0x7FFF) if d & 0x8000 else d for d in digs]
        assert sum(v << off for v, off in zip(val, offs)) == s, (hex(s), "the digits do not recombine")
        assert all(abs(v) <= 1 << (cw - 1) for v, cw in zip(val[:-1], ws)), (hex(s), "a digit past half")
        assert all(d != 0x8000 for d in digs), (hex(s), "a negative zero")
        assert not digs[-1] & 0x8000 and 0 <= val[-1] < 1 << 15, (hex(s), "the top window is negated")
        assert int(o[88]) == 0 and int(o[89]) == 0, (hex(s), "carry or scalar bits left over")
    # digits exactly at half stay positive, just past half go negative with a carry
    half = 1 << (ws[0] - 1)
    i, j = scalars.index(half), scalars.index(half + 1)
    assert int(out[i][0]) == half and int(out[j][0]) == (0x8000 | (half - 1)) and int(out[j][1]) == 1
