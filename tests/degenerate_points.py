"""Inputs of the point-multiplication and point-addition gadgets at which a denominator of the gadget's chord / tangent
formulas vanishes (point_mult.rs:667-704: inverse(0) = 0, dalek's Scalar::invert), at a chosen step.

Any (x, y) lies on the sibling curve y^2 = x^3 + a x + b' with b' = y^2 - x^3 - a x.  The gadget's formulas use only a, so
they are the group law of that curve, and a point of small order on a sibling curve puts a zero under 1/(2 ay) (the doubling
chain reaches a point with y = 0) or under 1/(bx - ax) (B = +-A) at a step the order and the weight decide:
  order 2   y = 0.
  order 4   2P has y = 0: lambda^2 = 2 x + x2 for a root x2 of x^3 + a x + b'; eliminating x2 gives the quadratic in b'
            -8 b'^2 + (20 x^3 - 4 a x) b' + (x^6 + 5 a x^4 - 5 a^2 x^2 - a^3) = 0.
  order 3   the 3-division polynomial 3 x^4 + 6 a x^2 + 12 b' x - a^2 = 0: b' = (a^2 - 3 x^4 - 6 a x^2) / (12 x).  2P = -P.
  2P.x = 0  lambda^2 = 2 x: y^2 = (3 x^2 + a)^2 / (8 x).
  order 5   Tate's normal form y^2 + (1 - t) x y - t y = x^3 - t x^2 has (0, 0) of order 5; in short form that is
            (3 b2, 108 a3) on Y^2 = X^3 - 27 c4 X - 54 c6, scaled by u with -27 c4 u^4 = a (t drawn until a fourth root exists).
            The only construction here whose first B = +-A comes after two set bits, when B's Jacobian Z is no longer 1.
Every construction draws x from a seeded generator until the square roots it needs exist.  denominator_trace states, with
the model's own _pa / _pd, which steps of an operation are degenerate; tests/test_degenerate_points.py holds every
construction to the step and kind it is made for, before any GPU test relies on it."""
import random

import numpy as np

import gadgets_model as GM
import pymodel as M

Q = GM.Q
A = GM.E2_A
N_BITS = 128


def sqrt_mod_q(v):
    """Tonelli-Shanks: a square root of v mod q, or None"""
    v %= Q
    if v == 0:
        return 0
    if pow(v, (Q - 1) // 2, Q) != 1:
        return None
    s, t = 0, Q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (Q - 1) // 2, Q) == 1:
        z += 1
    m, c, u, r = s, pow(z, t, Q), pow(v, t, Q), pow(v, (t + 1) // 2, Q)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % Q, i + 1
        b = pow(c, 1 << (m - i - 1), Q)
        m, c = i, b * b % Q
        u, r = u * c % Q, r * b % Q
    assert r * r % Q == v
    return r


def _inv(v):
    assert v % Q
    return pow(v % Q, Q - 2, Q)


def _draw(seed, make):
    rng = random.Random(seed)
    for _ in range(400):
        p = make(rng.randrange(1, Q))
        if p is not None:
            return p
    raise AssertionError("no point found")  # each draw succeeds with probability >= 1/4


def order2_point(seed):
    return _draw(seed, lambda x: (x, 0))


def order4_point(seed):
    def make(x):
        qa, qb = -8, (20 * x**3 - 4 * A * x) % Q
        qc = (x**6 + 5 * A * x**4 - 5 * A * A * x * x - A**3) % Q
        s = sqrt_mod_q(qb * qb - 4 * qa * qc)
        if s is None:
            return None
        for root in (s, -s):
            b1 = (-qb + root) * _inv(2 * qa) % Q
            y = sqrt_mod_q(x**3 + A * x + b1)
            if y:
                return x, y
        return None
    return _draw(seed, make)


def order3_point(seed):
    def make(x):
        b1 = (A * A - 3 * x**4 - 6 * A * x * x) * _inv(12 * x) % Q
        y = sqrt_mod_q(x**3 + A * x + b1)
        return (x, y) if y else None
    return _draw(seed, make)


def x_zero_point(seed):
    return 0, random.Random(seed).randrange(1, Q)


def double_has_x_zero_point(seed):
    def make(x):
        y = sqrt_mod_q((3 * x * x + A) ** 2 * _inv(8 * x))
        return (x, y) if y else None
    return _draw(seed, make)


def order5_point(seed):
    def make(t):
        a1, a3 = (1 - t) % Q, -t % Q
        b2, b4 = (a1 * a1 - 4 * t) % Q, a1 * a3 % Q
        c4 = (b2 * b2 - 24 * b4) % Q
        r = sqrt_mod_q(A * _inv(-27 * c4)) if c4 else None
        if r is None:
            return None
        for u2 in (r, Q - r):
            u = sqrt_mod_q(u2)
            if u is not None:
                return 3 * b2 * u2 % Q, 108 * a3 * u2 * u % Q
        return None
    return _draw(seed, make)


def denominator_trace(w, px, py, n=N_BITS):
    """[(kind, step)]: 'pa' where bx - ax is zero, 'pd' where 2 ay is, as the model's own loop (build_point_mult) meets them"""
    ax, ay = px % Q, py % Q
    bx, by, bz = 0, 0, 1
    out = []
    for i in range(n):
        if (bx - ax) % Q == 0:
            out.append(("pa", i))
        if 2 * ay % Q == 0:
            out.append(("pd", i))
        cx, cy = GM._pa(bx, by, bz, ax, ay)[:2]
        dx, dy = GM._pd(ax, ay, A)[:2]
        if (w >> i) & 1:
            bx, by, bz = cx, cy, 0
        ax, ay = dx, dy
    return out


def honest_ops(seed, weights):
    return GM.synthetic_mult_ops(seed, len(weights), weights=list(weights))


def table_rows(seed=0x5650494E + 70):
    """One operation per row: (name, (w, px, py) as the byte encodings' integers, first (kind, step) of the trace or None,
    the whole trace where the construction fixes it or None)."""
    o2, o4, o3, xz, dz = (order2_point(seed + 1), order4_point(seed + 2), order3_point(seed + 3), x_zero_point(seed + 4),
                          double_has_x_zero_point(seed + 5))
    o5 = order5_point(seed + 7)
    top = (1 << 256) - 1
    pa_from = lambda s: [("pa", i) for i in range(s, N_BITS)]
    rows = [
        ("order 2", ((1 << 127) + 9, *o2), ("pd", 0), None),
        ("order 4, w=5", (5, *o4), ("pd", 1), None),
        ("order 3, w=3", (3, *o3), ("pa", 1), [("pa", 1)]),
        ("order 3, w=1", (1, *o3), ("pa", 1), pa_from(1)),
        ("order 3, w=2^100", (1 << 100, *o3), ("pa", 101), pa_from(101)),
        ("order 3, w=0", (0, *o3), None, []),
        ("x=0, w=0", (0, *xz), ("pa", 0), None),
        ("x=0, w=1", (1, *xz), ("pa", 0), None),
        ("x=0, w=2^128-1", ((1 << 128) - 1, *xz), ("pa", 0), None),
        ("2P.x=0, w=2", (2, *dz), ("pa", 1), [("pa", 1)]),
        ("2P.x=0, w=3", (3, *dz), None, []),
        ("px=q", (6, Q, xz[1]), ("pa", 0), None),
        ("px=q+x, order 3", (3, Q + o3[0], o3[1]), ("pa", 1), [("pa", 1)]),
        ("py=q", (7, o2[0], Q), ("pd", 0), None),
        ("px=q, py=2^256-1", (2, Q, top), ("pa", 0), None),
        ("px=q+5, py=2^256-1", (3, Q + 5, top), None, []),
        # beyond the first set bit B = A_k with Z = 1, so a first B = +-A one step later is also seen by the denominator batch
        # through a bx that needs no inverse; after two set bits only the Z of C_i shows it: 3P = 8P and 7P = -8P
        ("order 5, w=3", (3, *o5), ("pa", 3), None),
        ("order 5, w=7", (7, *o5), ("pa", 3), None),
        ("order 5, w=0", (0, *o5), None, []),
    ]
    for (w, x, y), name in zip(honest_ops(seed + 6, [(1 << 128) - 1, 0, 1, 1 << 127]), ("2^128-1", "0", "1", "2^127")):
        rows.append(("honest, w=" + name, (w, x, y), None, []))
    return rows


def edge_batches(seed=0x5650494E + 71, n=66):
    """(mixed, all_degenerate, all_honest): n operations each.  mixed has degenerate operations of four kinds at lanes 0, 63, 64
    and 65 (both sides of the wave / workgroup boundary) and honest ones elsewhere."""
    st, ws = seed, []
    for _ in range(n):
        st, a = GM.splitmix64(st)
        st, b = GM.splitmix64(st)
        ws.append(((a << 64) | b) >> (a & 7))
    honest = honest_ops(seed + 1, ws)
    by_name = {name: op for name, op, first, _ in table_rows(seed + 2) if first is not None}
    kinds = list(by_name.values())
    mixed = list(honest)
    for name, lane in {"order 2": 0, "order 5, w=7": 63, "x=0, w=1": 64, "order 4, w=5": 65}.items():
        mixed[lane] = by_name[name]
    return mixed, [kinds[i % len(kinds)] for i in range(n)], honest


def add_ops(seed=0x5650494E + 72, n=65):
    """n point additions (px, py, rx, ry, rz) with the degenerate ones the gadget can meet: R = P, R = -P, rz = 1 with an
    arbitrary R, rx = px = 0, and encodings >= q in lane 63 (last of the first wave) and lane 64 (alone in the second)."""
    ops = GM.synthetic_add_ops(seed, n, rz_one_every=9)
    top = (1 << 256) - 1
    px, py = ops[1][0], ops[1][1]
    ops[2] = (px, py, px, py, 0)
    ops[3] = (px, py, px, Q - py, 0)
    ops[4] = (px, py, ops[5][2], ops[5][3], 1)
    ops[6] = (0, py, 0, ops[5][3], 0)
    ops[7] = (0, 0, 0, 0, 0)
    ops[63] = (Q + px, top, top, Q, 0)
    ops[64] = (Q, Q + py, Q + 0, top - 1, 0)   # rx = px = 0 again, through two encodings of zero
    return ops


def to_table(ints):
    """M.ints_to_table for long lists: (n, 4) uint64 Montgomery limbs through bytes instead of a row at a time"""
    raw = b"".join(((v % Q) * M.R % Q).to_bytes(32, "little") for v in ints)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def padded_assignment(assign):
    """the three assignment vectors as Instance::new pads them: [vars_para, vars_input, vars] tables of next_pow2 rows"""
    nv = len(assign[0])
    pad = GM.next_pow2(max(nv, 2)) - nv
    return [to_table(list(v) + [0] * pad) for v in assign]


def bytes32(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def first_difference(got, exp):
    """None when the two tables are equal, else (number of differing entries, index of the first)"""
    got, exp = np.asarray(got).reshape(-1, 4), np.asarray(exp).reshape(-1, 4)
    if got.shape != exp.shape:
        return (abs(len(got) - len(exp)), min(len(got), len(exp)))
    bad = np.nonzero((got != exp).any(axis=1))[0]
    return None if len(bad) == 0 else (len(bad), int(bad[0]))
