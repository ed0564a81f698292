"""The multi-window table walks of msm.hip at their digit edges: every kernel that recodes a scalar into signed digits gets
every named vector of tests/digit_vectors.py for the window width of the table it walks, byte for byte against the CPU oracle.

    msm_rows_kernel / table_mul_acc<ge10> (sequential walk, ten-limb accumulator)     gens_msm, hyrax_commit (blinds: n_extra)
    msm_wide_kernel<1|4> / table_mul_acc_range (eight lanes per scalar)           gens_msm_parts, 64 and 32768 columns
    single_base_mul_kernel / table_mul_acc_range                                   hyrax_commit_pair_split
    bullet_step_kernel / table_mul_acc_range                                       vpin_bullet_reduce, fused rounds
    scalar_times_bases_kernel / table_mul_acc (extended accumulator), add_cached   hyrax_commit_derefs with hot columns

The window width follows from the generator count under a 1 GiB budget (fit in gens_build_once): 12 bits (W = 22, three
windows per lane), 8 bits (W = 32, four per lane: the width of the table narrowed beside a row table, and of the second
segment) and 7 bits (W = 37, five per lane, the last lane short).  Every test reads vpin_gens_layout, asserts the width it
was written for and builds its vectors from what it read."""
import ctypes as C

import numpy as np
import pytest

import digit_vectors as D
import oracle_lib as O
import pymodel as M
from test_gpu_bullet import device as bullet_device, model as bullet_model
from test_gpu_msm_wide import NB as NB_BIG, sum_parts

pytestmark = pytest.mark.gpu
Q = M.Q
NB = {12: 200, 8: 2000, 7: 3000}   # widest c with nb * ceil(254 / c) * 2^(c-1) * 96 <= 2^30: 12 up to 248, 8 in 1507..2730, 7 in 2731..4723
R = 64                             # columns of every small case; the blind base is generator R + 1


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def layout(g):
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_gens_layout.argtypes = [C.c_void_p, C.c_void_p]
    lay = (C.c_size_t * 6)()
    assert L.vpin_gens_layout(g.h, lay) == 0
    return [int(x) for x in lay]


@pytest.fixture(scope="module")
def tables(ctx):
    xyzt, og = O.gens_stream_xyzt(max(NB.values()))
    return {c: (ctx.gens_shared(f"test_msm_digits_c{c}", xyzt[:nb], 1), og) for c, nb in NB.items()}


@pytest.fixture(scope="module")
def big(ctx):
    """the shared two-segment table of tests/test_gpu_msm_wide.py: same label, same budget, one build per session"""
    xyzt, og = O.gens_stream_xyzt(NB_BIG, b"gens_r1cs_eval")
    return ctx.gens_shared("gens_r1cs_eval", xyzt, 80 if ctx.device_total_bytes() >= (200 << 30) else 24), og


def vectors_for(g, c):
    """the vectors of the layout READ from the table, which must be the one the test was written for"""
    lay = layout(g)
    assert lay[:2] == [c, D.windows(c)] and lay[3:5] == [0, 0] and lay[2] == lay[5], (c, lay)
    assert (lay[1] + 7) // 8 == {12: 3, 8: 4, 7: 5}[c]
    return D.edge_scalars(lay[0], lay[1])


def full(rng):
    return int.from_bytes(rng.bytes(32), "little") % Q


def mul_bytes(p, k):
    L = O.lib()
    r = O.Ge()
    L.ge_scalarmul_bytes(C.byref(r), (C.c_uint8 * 32)(*int(k).to_bytes(32, "little")), C.byref(p))
    return r


def compress(p):
    out = (C.c_uint8 * 32)()
    O.lib().ge_compress(out, C.byref(p))
    return bytes(out)


def add(p, q):
    r = O.Ge()
    O.lib().ge_add(C.byref(r), C.byref(p), C.byref(q))
    return r


_cases = {}


def cases(c, vecs):
    """the three layouts of the rows tests, built once per width: vals, rows, expected bytes per row"""
    if c in _cases:
        return _cases[c]
    vals = [v.s for v in vecs]
    n = len(vals)
    rng = np.random.default_rng(1000 + c)
    alone = [0] * (n * R)                      # row i holds vector i alone, at column i % R
    for i, s in enumerate(vals):
        alone[i * R + i % R] = s
    out = [("alone", alone, n)]
    for rows in (-(-n // 16), 128):            # fewer than 128 rows: column chunks; 128 and more: one workgroup per row
        assert rows == 128 or rows < 128 and rows * 16 >= n
        per = -(-n // rows)
        mixed = []
        for r in range(rows):
            row = [full(rng) if k < 24 else 0 for k in range(R)]
            pos = rng.permutation(R)
            for k, s in enumerate(vals[r * per:(r + 1) * per]):
                row[int(pos[k])] = s
            mixed += row
        assert sorted(set(mixed) & set(vals)) == sorted(vals)
        out.append((f"among full-width scalars and zeros, {rows} rows", mixed, rows))
    _cases[c] = out
    return out


def expected(og, vals, rows, vecs):
    if rows == len(vecs):                      # one vector per row: the oracle's double-and-add on that generator
        return [compress(mul_bytes(og[i % R], v.s)) for i, v in enumerate(vecs)]
    exp = O.hyrax_commit(M.ints_to_table(vals), rows, np.zeros((rows, 4), dtype=np.uint64), og, R + 1)
    return [bytes(e) for e in exp]


@pytest.mark.parametrize("c", [12, 8, 7])
def test_rows_kernel_walks_every_vector(ctx, tables, c):
    """msm_rows_kernel / table_mul_acc<ge10> through vpin_gens_msm"""
    g, og = tables[c]
    vecs = vectors_for(g, c)
    for what, vals, rows in cases(c, vecs):
        got = ctx.gens_msm(g, M.ints_to_table(vals), rows, R)
        exp = expected(og, vals, rows, vecs)
        bad = [(i, vecs[i].name if rows == len(vecs) else "") for i in range(rows) if bytes(got[i]) != exp[i]]
        assert not bad, (c, what, bad[:8])


@pytest.mark.parametrize("c", [12, 8, 7])
def test_rows_kernel_takes_every_vector_as_a_blind(ctx, tables, c):
    """the n_extra path of msm_rows_kernel: vpin_hyrax_commit with the vectors as blinds on generator R + 1"""
    g, og = tables[c]
    vecs = vectors_for(g, c)
    rng = np.random.default_rng(2000 + c)
    Ls = 256
    assert len(vecs) <= Ls
    blinds = [v.s for v in vecs] + [full(rng) for _ in range(Ls - len(vecs))]
    vals = [0] * (Ls * R)
    for i in range(0, Ls, 3):                  # every third row has scalars of its own beside the blind
        for j in rng.integers(0, R, size=5):
            vals[i * R + int(j)] = full(rng)
    Z, b = M.ints_to_table(vals), M.ints_to_table(blinds)
    dZ = ctx.upload(Z)
    try:
        got = ctx.hyrax_commit(g, dZ, b, R + 1)
    finally:
        dZ.free()
    exp = O.hyrax_commit(Z, Ls, b, og, R + 1)
    bad = [(i, vecs[i].name if i < len(vecs) else "") for i in range(Ls) if not np.array_equal(got[i], exp[i])]
    assert not bad, (c, bad[:8])
    for i in (1, 2):                           # a row of nothing but the blind is the plain multiple of the blind generator
        assert bytes(got[i]) == compress(mul_bytes(og[R + 1], blinds[i]))


@pytest.mark.parametrize("c", [12, 8, 7])
def test_wide_kernel_splits_every_vector_over_its_lanes(ctx, tables, c):
    """msm_wide_kernel<1> / table_mul_acc_range through vpin_gens_msm_parts: carry_into at every lane boundary"""
    g, og = tables[c]
    vecs = vectors_for(g, c)
    for what, vals, rows in cases(c, vecs):
        parts = ctx.gens_msm_parts(g, M.ints_to_table(vals), rows, R)
        exp = expected(og, vals, rows, vecs)
        bad = [(i, vecs[i].name if rows == len(vecs) else "") for i in range(rows) if sum_parts(parts[i]) != exp[i]]
        assert not bad, (c, what, bad[:8])


def test_long_row_in_both_segments(ctx, big):
    """msm_wide_kernel<4> (>= 8192 columns) and msm_rows_kernel on one row of 32768 columns, all zero except the vectors: those
    of the first segment's width below the split, those of the second segment's width from column 16386 on"""
    g, og = big
    lay = layout(g)
    c, W, split, c_hi, W_hi, bases = lay
    assert bases >= NB_BIG and W == D.windows(c)
    if ctx.device_total_bytes() >= (200 << 30):
        assert split == 16386 and c == 12 and 6 < c_hi < 12 and W_hi == D.windows(c_hi), lay
    ncols = 32768
    lo = D.edge_scalars(c, W)
    hi = D.edge_scalars(c_hi, W_hi) if c_hi else lo      # one segment (a small part): the same width everywhere
    first_hi = 16386
    place = {}
    for i, v in enumerate(lo):
        place[(i * 97 + 5) % first_hi] = v                # 97 and 113 are prime to the ranges: no column twice
    for i, v in enumerate(hi):
        place[first_hi + (i * 113) % (ncols - first_hi)] = v
    assert len(place) == len(lo) + len(hi) and first_hi in place and min(place) < 32
    cols = sorted(place)
    sc = np.zeros((ncols, 4), dtype=np.uint64)
    tab = M.ints_to_table([place[j].s for j in cols])
    sc[cols] = tab
    L = O.lib()
    n = len(cols)
    r = O.Ge()
    L.ge_msm(C.byref(r), O.ptr(np.ascontiguousarray(tab)), (O.Ge * n)(*[og[j] for j in cols]), n)
    exp = compress(r)
    assert exp == compress(_sum([mul_bytes(og[j], place[j].s) for j in cols]))   # the oracle's Pippenger against its double-and-add
    parts = ctx.gens_msm_parts(g, sc, 1, ncols)
    assert sum_parts(parts[0]) == exp, "msm_wide_kernel<4>"
    assert bytes(ctx.gens_msm(g, sc, 1, ncols)[0]) == exp, "msm_rows_kernel over both segments"
    # each segment's vectors on their own, so that a failure names its segment
    for name, keep in (("first segment", [j for j in cols if j < first_hi]), ("second segment", [j for j in cols if j >= first_hi])):
        one = np.zeros_like(sc)
        one[keep] = sc[keep]
        want = compress(_sum([mul_bytes(og[j], place[j].s) for j in keep]))
        assert sum_parts(ctx.gens_msm_parts(g, one, 1, ncols)[0]) == want, name


def _sum(pts):
    acc = O.Ge()
    O.lib().ge_identity(C.byref(acc))
    for p in pts:
        acc = add(acc, p)
    return acc


def check_blind_multiples(ctx, g, h, vals, blind_base):
    """all-zero Za, Zb and the vectors as both blind lists: the outputs are v * g[blind_base] and their sums, through the one-call
    form (msm_rows_kernel, n_extra) and the provers' split-phase form (single_base_mul_kernel)"""
    Ls = 256
    assert len(vals) <= Ls
    a = (vals * (-(-Ls // len(vals))))[:Ls]
    assert len(a) == Ls
    b = a[::-1]
    ta, tb = M.ints_to_table(a), M.ints_to_table(b)
    mult = {s: mul_bytes(h, s) for s in set(a)}
    exp = [[compress(mult[s]) for s in a], [compress(mult[s]) for s in b], [compress(add(mult[x], mult[y])) for x, y in zip(a, b)]]
    dZ = ctx.upload(np.zeros((2 * Ls, 4), dtype=np.uint64))
    try:
        for name, fn in (("pair", ctx.hyrax_commit_pair), ("split", ctx.hyrax_commit_pair_split)):
            outs = fn(g, dZ, dZ, ta, tb, blind_base)
            for k in range(3):
                bad = [i for i in range(Ls) if bytes(outs[k][i]) != exp[k][i]]
                assert not bad, (name, k, bad[:8])
    finally:
        dZ.free()


@pytest.mark.parametrize("c", [12, 8, 7])
def test_single_base_multiples_of_every_vector(ctx, tables, c):
    g, og = tables[c]
    vecs = vectors_for(g, c)
    check_blind_multiples(ctx, g, og[R + 1], [v.s for v in vecs], R + 1)


def test_single_base_multiples_in_the_second_segment(ctx, big):
    g, og = big
    c, W, split, c_hi, W_hi, _ = layout(g)
    if ctx.device_total_bytes() >= (200 << 30):
        assert split == 16386 and c_hi
    base = NB_BIG - 1                                     # h of the 2^15-column stream: beyond the split
    vecs = D.edge_scalars(c_hi, W_hi) if c_hi else D.edge_scalars(c, W)
    check_blind_multiples(ctx, g, og[base], [v.s for v in vecs], base)


@pytest.mark.parametrize("c", [12, 8, 7])
def test_bullet_rounds_with_the_vectors_as_x(ctx, tables, c):
    """bullet_step_kernel / table_mul_acc_range: fused rounds of R = 64 with x = the vectors -- round 0's MSM scalars are x
    itself (s_j = 1), the later rounds' are folded ones; every round against the folding model of tests/test_gpu_bullet.py"""
    g, og = tables[c]
    vals = [v.s for v in vectors_for(g, c)]
    vals += vals[:-len(vals) % R]
    rng = np.random.default_rng(3000 + c)
    G = [og[i] for i in range(R)]
    for k0 in range(0, len(vals), R):
        a = vals[k0:k0 + R]
        b = [full(rng) for _ in range(R)]
        us = [full(rng) % (Q - 1) + 1 for _ in range(R.bit_length() - 1)]
        want_rounds, x_hat, a_hat, g_hat = bullet_model(a, b, G, us)
        cLR, LR, fin, gh = bullet_device(ctx, g, a, b, us, 0)
        for j, (cL, cR, Lc, Rc) in enumerate(want_rounds):
            assert M.table_to_ints(cLR[j]) == [cL, cR], (c, k0, j)
            assert bytes(LR[j, 0]) == Lc and bytes(LR[j, 1]) == Rc, f"c = {c}, vectors {k0}.., L / R of round {j}"
        assert M.table_to_ints(fin) == [x_hat, a_hat] and gh == g_hat, (c, k0)


@pytest.mark.parametrize("c", [12, 8, 7])
def test_hot_column_tables_of_every_vector(ctx, tables, c):
    """scalar_times_bases_kernel / table_mul_acc and add_cached: the derefs commitment of 8 rows of R = 64 with E_ry[hot] = v,
    three vectors (three hot columns, three T tables) per call: a row whose every entry is the hot one, a row with 40 % of them,
    a row with two; once with E_ry[hot] = 0"""
    g, og = tables[c]
    vals = [v.s for v in vectors_for(g, c)]
    rng = np.random.default_rng(4000 + c)
    N, ncol, hot = R, 128, [11, 70, 123]
    e_ry = [full(rng) for _ in range(ncol)]
    col = rng.integers(0, ncol, size=(3, N), dtype=np.uint32)
    col[np.isin(col, hot)] = 5
    col[0][:] = hot[0]
    col[1][rng.random(N) < 0.4] = hot[1]
    col[2][[3, 60]] = hot[2]
    assert (col[1] == hot[1]).sum() >= 8
    head = [full(rng) for _ in range(3 * N)]
    zero_blinds = np.zeros((8, 4), dtype=np.uint64)
    trios = [vals[i:i + 3] for i in range(0, len(vals) - 2, 3)] + [vals[-3:], [0, vals[0], 0]]
    taken0 = ctx.strip_rows_taken()
    for trio in trios:
        for m in range(3):
            e_ry[hot[m]] = trio[m]
        Z = M.ints_to_table(head + [e_ry[int(col[m][i])] for m in range(3) for i in range(N)] + [0] * (2 * N))
        dZ, dE = ctx.upload(Z), ctx.upload(M.ints_to_table(e_ry))
        try:
            got = ctx.hyrax_commit_derefs(g, dZ, 8, N, col, hot, dE)
        finally:
            dZ.free()
            dE.free()
        exp = O.hyrax_commit(Z, 8, zero_blinds, og, R + 1)
        assert np.array_equal(got, exp), (c, [hex(x) for x in trio], [i for i in range(8) if not np.array_equal(got[i], exp[i])])
        if trio[0]:
            assert bytes(got[3]) == compress(mul_bytes(_gsum(og), trio[0])), "the all-hot row is v * (g_0 + .. + g_63)"
        else:
            assert bytes(got[3]) == bytes(32), "E_ry[hot] = 0: the all-hot row is the identity"
    assert ctx.strip_rows_taken() == taken0   # eight rows: msm_rows_hot_kernel alone


_gs = []


def _gsum(og):
    if not _gs:
        _gs.append(_sum([og[j] for j in range(R)]))
    return _gs[0]
