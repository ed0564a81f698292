"""The row-per-lane pipeline of the derefs commitment on its own: strip_classify_kernel, strip_list_kernel, strip_trim_kernel,
msm_strip_kernel, strip_combine_kernel and msm_rows_hot_kernel in its hot_only mode, through vpin_hyrax_commit_derefs with
VPIN_MSM_STRIP_MIN=1 on a table without a row table.  Every case asserts
    1. the bytes of the row kernel alone (VPIN_MSM_STRIP=0),
    2. the bytes of the CPU oracle's commitment (every row; a fixed sample of rows for the one large case),
    3. that vpin_ctx_strip_rows_taken grew by what the rule, restated here from the inputs, predicts: a row is taken iff it is
       not constant and 8 * (zero scalars + hot-index entries) <= R, less what strip_shape trims -- never zero, so a case
       fails when the strip kernel takes no row.
At R = 64 no strip count fits on its own (a strip has at least 128 generators, and the gate asks for 16 strips <= R / 8), so
the small cases force one with VPIN_MSM_STRIP=8: workgroups run free.  Workgroups in step need a shape: VPIN_MSM_STRIP_SHAPE
from R = 128 on, or the library's own choice at R = 1024."""
import ctypes as C
import os

import numpy as np
import pytest

import digit_vectors as D
import oracle_lib as O
import pymodel as M
from test_gpu_cumask import _cus

pytestmark = pytest.mark.gpu
Q = M.Q
NB = 1100     # R up to 1024 + gens_1 base + h; under 1 GiB that is 9-bit windows (c = 10 stops at 840 generators, c = 9 at 1506)
NCOL = 128    # length of E_ry
SWITCHES = ("VPIN_MSM_STRIP", "VPIN_MSM_STRIP_MIN", "VPIN_MSM_STRIP_SHAPE", "VPIN_MSM_STRIP_LAG")


class env:
    """the four per-call switches for the length of a block: those not named are unset, everything is put back afterwards"""

    def __init__(self, **kv):
        assert all(k in SWITCHES for k in kv)
        self.kv = {k: kv.get(k) for k in SWITCHES}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(ctx):
    """(table, oracle generators, vectors of its width); the width is asserted, the vectors are built from the layout read"""
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_gens_layout.argtypes = [C.c_void_p, C.c_void_p]
    L.vpin_gens_row_layout.argtypes = [C.c_void_p, C.c_void_p]
    xyzt, og = O.gens_stream_xyzt(NB)
    g = ctx.gens_shared("test_msm_strip", xyzt, 1)
    lay, row = (C.c_size_t * 6)(), (C.c_size_t * 4)()
    assert L.vpin_gens_layout(g.h, lay) == 0 and L.vpin_gens_row_layout(g.h, row) == 0
    assert list(row) == [0, 0, 0, 0], "a row table would take the commitment"
    assert list(lay)[:2] == [9, 29] and lay[2] == lay[5] >= NB, list(lay)
    return g, og, D.edge_scalars(int(lay[0]), int(lay[1]))


def rand_table(rng, n):
    """n non-zero scalars as Montgomery limbs (any limbs below 2^251 are the Montgomery form of some canonical scalar)"""
    t = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 59) - 1)
    t[:, 0] |= np.uint64(1)
    return t


class Case:
    """a derefs-shaped polynomial: L = 8N / R rows of R -- 3N/R row-derefs rows, N/R col-derefs rows for each of three matrices
    (scalar = E_ry[col index]), 2N/R all-zero padding rows"""

    def __init__(self, rng, R, N, hot):
        self.R, self.N, self.hot = R, N, list(hot)
        self.rpv = N // R
        self.L = 8 * self.rpv
        self.row0 = 3 * self.rpv
        self.e_ry = rand_table(rng, NCOL)
        free = np.array([k for k in range(NCOL) if k not in hot], dtype=np.uint32)
        self.col = free[rng.integers(0, len(free), size=(3, N))]     # no hot entry until a test puts one
        self.head = rand_table(rng, 3 * N).reshape(3 * self.rpv, R, 4)
        self.zeros = []                                               # (row, columns) set to zero after everything else
        self.rows = {}                                                # row -> (R, 4) table replacing a row-derefs row

    def mrow(self, m, r):
        return self.row0 + m * self.rpv + r

    def set_hot(self, m, r, columns):
        self.col[m][r * self.R + np.asarray(columns, dtype=np.int64)] = self.hot[m]

    def build(self):
        R, rpv = self.R, self.rpv
        Z = np.zeros((self.L, R, 4), dtype=np.uint64)
        Z[:3 * rpv] = self.head
        Z[3 * rpv:6 * rpv] = self.e_ry[self.col.reshape(-1)].reshape(3 * rpv, R, 4)
        for row, tab in self.rows.items():
            assert row < 3 * rpv
            Z[row] = tab
        for row, columns in self.zeros:
            Z[row, columns] = 0
        return Z

    def hot_mask(self):
        mask = np.zeros((self.L, self.R), dtype=bool)
        for m in range(3):
            if self.hot[m] is not None:
                mask[self.row0 + m * self.rpv:self.row0 + (m + 1) * self.rpv] = (self.col[m] == self.hot[m]).reshape(self.rpv, self.R)
        return mask

    def eligible(self, Z):
        """the rule of strip_classify_kernel from the inputs"""
        zero = ~Z.any(axis=2)
        constant = (Z == Z[:, :1, :]).all(axis=(1, 2))
        skipped = (zero | self.hot_mask()).sum(axis=1)
        return ~constant & (8 * skipped <= self.R)


def shape_rows(R, eligible, slots, masked, forced=None):
    """strip_shape restated: rows the launch takes of `eligible` listed ones (min_list = 1 under VPIN_MSM_STRIP_MIN)"""
    if 16 > R // 8:
        return 0        # without VPIN_MSM_STRIP the gate in front of the classification asks with the default of 16 strips
    G = -(-eligible // 256)
    cands = [s for s in range(8, 65, 8) if s * 128 <= R]
    bestG = bestS = 0
    for s in cands:
        if G * s <= slots:
            bestG, bestS = G, s
    if masked:
        for s in cands:
            g2 = min(G, slots // s)
            if g2 * 256 >= 1 and g2 * s > bestG * bestS:
                bestG, bestS = g2, s
    if forced:
        eg, es = forced
        if es % 8 == 0 and es <= R // 8 and min(G, eg) * es <= slots:
            bestG, bestS = min(G, eg), es
    return min(eligible, bestG * 256) if bestG else 0


def check(cx, table, case, switches, take=None, sample=None):
    """run `case` with the strip path on (VPIN_MSM_STRIP_MIN=1 + switches) and off; take: rows the shape leaves of the eligible
    ones (None: all); sample: rows to check against the oracle (None: all).  Returns (eligible mask, bytes)."""
    g, og, _ = table
    Z = case.build()
    elig = case.eligible(Z)
    want_taken = int(elig.sum()) if take is None else take(int(elig.sum()))
    assert want_taken > 0, "a strip case must hand rows to the strip kernel"
    flat = Z.reshape(-1, 4)
    dZ, dE = cx.upload(flat), cx.upload(case.e_ry)
    try:
        t0 = cx.strip_rows_taken()
        with env(VPIN_MSM_STRIP=0):
            base = cx.hyrax_commit_derefs(g, dZ, case.L, case.N, case.col, case.hot, dE)
        assert cx.strip_rows_taken() == t0, "VPIN_MSM_STRIP=0 must keep the row kernel"
        runs = []
        for sw in (switches if isinstance(switches, list) else [switches]):
            t0 = cx.strip_rows_taken()
            with env(VPIN_MSM_STRIP_MIN=1, **sw):
                runs.append(cx.hyrax_commit_derefs(g, dZ, case.L, case.N, case.col, case.hot, dE))
            taken = cx.strip_rows_taken() - t0
            print(f"R = {case.R}, L = {case.L}, {sw}: {int(elig.sum())} eligible, {taken} taken")
            assert taken == want_taken, (sw, taken, want_taken)
    finally:
        dZ.free()
        dE.free()
    for sw, got in zip(switches if isinstance(switches, list) else [switches], runs):
        bad = [i for i in range(case.L) if not np.array_equal(got[i], base[i])]
        assert not bad, (sw, "strip path against the row kernel alone", bad[:8], [bool(elig[i]) for i in bad[:8]])
    rows = list(range(case.L)) if sample is None else sorted(set(sample))
    zero_blinds = np.zeros((len(rows), 4), dtype=np.uint64)
    exp = O.hyrax_commit(np.ascontiguousarray(Z[rows]).reshape(-1, 4), len(rows), zero_blinds, og, case.R + 1)
    bad = [r for k, r in enumerate(rows) if not np.array_equal(base[r], exp[k])]
    assert not bad, ("against the oracle", bad[:8], [bool(elig[i]) for i in bad[:8]])
    return elig, base


def base_case(seed, hot=(11, None, 70)):
    return Case(np.random.default_rng(seed), 64, 4096, hot)   # 512 rows: 192 row-derefs, 3 x 64 col-derefs, 128 zero padding


def sparse(case, rng, row, n):
    """n zero scalars in a row, at columns that hold no hot entry"""
    m = case.hot_mask()[row]
    columns = rng.permutation(np.nonzero(~m)[0])[:n]
    case.zeros.append((row, columns))


def test_classification_threshold(ctx, table):
    """8 * skipped <= R at R = 64: eight skipped entries are taken, nine are not -- as zeros, as hot entries, mixed, and with a
    zero scalar AT a hot index counted once; constant rows are never taken, rows that only look constant at the probed positions are"""
    case = base_case(1)
    rng = np.random.default_rng(101)
    R = case.R
    want = {}
    for row in (0, 1, 2, 3):
        sparse(case, rng, row, R // 8)
        want[row] = True
    for row in (4, 5, 6, 7):
        sparse(case, rng, row, R // 8 + 1)
        want[row] = False
    for row in (8, 9):                                    # a non-zero constant row
        case.rows[row] = np.repeat(rand_table(rng, 1), R, axis=0)
        want[row] = False
    for row in (10, 11):                                  # equal at the probed positions 0, 1, R/2, R-1 of the row kernels only
        t = rand_table(rng, R)
        t[[0, 1, R // 2, R - 1]] = t[0]
        case.rows[row] = t
        want[row] = True
    for row in (12, 13):                                  # all zero: constant
        case.rows[row] = np.zeros((R, 4), dtype=np.uint64)
        want[row] = False
    for r in (0, 1, 2, 3):                                # matrix 0: hot entries only
        case.set_hot(0, r, rng.permutation(R)[:R // 8])
        want[case.mrow(0, r)] = True
    for r in (4, 5, 6, 7):                                # five hot entries and three zeros elsewhere
        case.set_hot(0, r, rng.permutation(R)[:5])
        sparse(case, rng, case.mrow(0, r), 3)
        want[case.mrow(0, r)] = True
    for r in (8, 9):                                      # four hot entries, one of them a zero scalar, and four zeros elsewhere: eight
        columns = rng.permutation(R)[:4]
        case.set_hot(0, r, columns)
        sparse(case, rng, case.mrow(0, r), 4)
        case.zeros.append((case.mrow(0, r), columns[:1]))
        want[case.mrow(0, r)] = True
    for r in (10, 11, 12, 13):
        case.set_hot(0, r, rng.permutation(R)[:R // 8 + 1])
        want[case.mrow(0, r)] = False
    for r in (14, 15):                                    # six hot entries and three zeros
        case.set_hot(0, r, rng.permutation(R)[:6])
        sparse(case, rng, case.mrow(0, r), 3)
        want[case.mrow(0, r)] = False
    case.set_hot(0, 16, np.arange(R))                     # every entry the hot one: a constant row
    want[case.mrow(0, 16)] = False
    for r in (0, 1):                                      # matrix 1 has no hot column: matrix 0's hot index means nothing there
        case.col[1][r * R + rng.permutation(R)[:20]] = case.hot[0]
        want[case.mrow(1, r)] = True
    for r in (0, 1):                                      # matrix 2, its own hot column
        case.set_hot(2, r, rng.permutation(R)[:R // 8])
        case.set_hot(2, r + 2, rng.permutation(R)[:R // 8 + 1])
        want[case.mrow(2, r)], want[case.mrow(2, r + 2)] = True, False
    elig = case.eligible(case.build())
    assert {row: bool(elig[row]) for row in want} == want          # the restated rule says what the groups were built to be
    assert not elig[384:].any() and int(elig.sum()) == 384 - sum(1 for v in want.values() if not v)
    check(ctx, table, case, dict(VPIN_MSM_STRIP=8))


@pytest.mark.parametrize("n", [5, 256, 257, 300])
def test_list_lengths(ctx, table, n):
    """n taken rows: less than a wave, exactly one workgroup, one workgroup and a single live lane, and a second workgroup of 44
    live lanes whose dead lanes read the last listed row"""
    case = base_case(2, hot=(11, 5, None))
    rng = np.random.default_rng(200 + n)
    for r in range(0, 64, 3):
        case.set_hot(0, r, rng.permutation(64)[:1 + r % 8])
    keep = set(int(x) for x in rng.permutation(384)[:n])
    for row in range(384):
        if row not in keep:
            sparse(case, rng, row, 20)                    # twenty zeros: the row stays with the row kernel
    elig, _ = check(ctx, table, case, dict(VPIN_MSM_STRIP=8))
    assert int(elig.sum()) == n and set(np.nonzero(elig)[0].tolist()) == keep


@pytest.mark.parametrize("R,S,per,empty_from", [(256, 24, 11, None), (512, 56, 10, 52)])
def test_forced_strip_counts(ctx, table, R, S, per, empty_from):
    """free-running workgroups with a strip count that does not divide R: a short last strip (24 strips of 11 over 256
    generators) and strips that receive no generator at all (56 strips of 10 over 512: those from 52 on)"""
    assert -(-R // S) == per
    if empty_from is None:
        assert (S - 1) * per < R < S * per
    else:
        assert empty_from * per >= R > (empty_from - 1) * per and empty_from < S
    case = Case(np.random.default_rng(R), R, 8 * R, (11, None, 70))   # 64 rows
    rng = np.random.default_rng(R + 1)
    for r in range(8):
        case.set_hot(0, r, rng.permutation(R)[:1 + 4 * r])
        case.set_hot(2, r, rng.permutation(R)[:R // 8 + (r % 2)])      # at the threshold, and one above
    for row in range(0, 24, 5):
        sparse(case, rng, row, R // 16)
    elig, _ = check(ctx, table, case, dict(VPIN_MSM_STRIP=S))
    assert 40 <= int(elig.sum()) < 48


def test_lanes_of_a_wave_that_disagree(ctx, table):
    """every lane of a workgroup walks its own row through the same generator: different vectors of digit_vectors.py in one
    column, a column where one lane of a wave is active, one where none is, and one that is the hot column for some lanes"""
    _, _, vecs = table
    case = base_case(3, hot=(11, None, 70))
    tab = M.ints_to_table([v.s for v in vecs])
    for row in range(192):
        t = case.head[row]
        t[0] = tab[row % len(tab)]                        # column 0: a different vector in every lane
        t[7] = tab[(5 * row + 1) % len(tab)]
        if row != 5:
            t[1] = 0                                      # column 1: lane 5 of the first wave alone walks it
        if row < 64:
            t[2] = 0                                      # column 2: nobody in the first wave, everybody in the second
    for r in range(0, 64, 2):
        case.set_hot(0, r, [3])                           # column 3: the hot one for every other lane of the fourth wave
    for r in range(0, 64, 9):
        case.set_hot(2, r, [3, 0])
    elig, _ = check(ctx, table, case, dict(VPIN_MSM_STRIP=8))
    assert elig[:384].all()                               # so the list is 0 .. 383 and lane k of workgroup 0 is row k


@pytest.mark.parametrize("pick", [0, 1, 2, 3])
def test_hot_entries_of_taken_rows(ctx, table, pick):
    """hot_only: the row kernel adds only the hot entries of a taken row, from T = E_ry[hot] * g_j with E_ry[hot] a vector of
    digit_vectors.py; 1 .. R/8 hot entries per row, a matrix without a hot column beside two that share one (one T table)"""
    _, _, vecs = table
    by = {v.name: v for v in vecs}
    name = ["every digit below bit 251 = half", "q - [every digit below bit 251 = half+1]", "2^251",
            "b=8: run of 2 half below the boundary, carry in from window 5, 1 in window 8"][pick]
    case = base_case(40 + pick, hot=(11, None, 11))
    case.e_ry[11] = M.ints_to_table([by[name].s])[0]
    rng = np.random.default_rng(400 + pick)
    for m in (0, 2):
        for r in range(64):
            case.set_hot(m, r, rng.permutation(64)[:1 + (r + m) % 8])
    elig, _ = check(ctx, table, case, dict(VPIN_MSM_STRIP=8))
    assert elig[:384].all()


def test_the_library_shape_with_workgroups_in_step(ctx, table):
    """R = 1024: strip_shape finds 8 strips of 128 generators on its own and the workgroups of a strip wait for each other;
    the lag (generators a workgroup may run ahead: default 1, 0 = no wait, 2) must not change a byte"""
    case = Case(np.random.default_rng(5), 1024, 16384, (11, None, 70))   # 128 rows
    rng = np.random.default_rng(50)
    for r in range(16):
        case.set_hot(0, r, rng.permutation(1024)[:1 + 9 * r])           # up to 136 hot entries: above R / 8 = 128
        case.set_hot(2, r, rng.permutation(1024)[:128 + r % 2])
    for row in range(0, 48, 7):
        sparse(case, rng, row, 100)
    cus, _ = ctx.device_props()
    elig, _ = check(ctx, table, case, [dict(), dict(VPIN_MSM_STRIP_LAG=0), dict(VPIN_MSM_STRIP_LAG=2)],
                    take=lambda n: shape_rows(1024, n, 3 * cus, False))
    assert shape_rows(1024, int(elig.sum()), 3 * cus, False) == int(elig.sum())
    assert 80 <= int(elig.sum()) < 96


def test_trimming_by_a_forced_shape(ctx, table):
    """VPIN_MSM_STRIP_SHAPE=1,8 with 384 eligible rows: one workgroup of 256 rows, strip_trim_kernel hands rows 256 .. 383 back to
    the row kernel (flags cleared: they must be walked in full there, not hot_only).  The base shape's rows at R = 128, the
    shortest rows for which the library looks for a shape at all (its default of 16 strips must be at most R / 8)"""
    R = 128
    case = Case(np.random.default_rng(6), R, 64 * R, (11, 5, 70))        # 512 rows: 192 + 3 x 64 + 128
    rng = np.random.default_rng(60)
    for m in range(3):
        for r in range(64):
            case.set_hot(m, r, rng.permutation(R)[:r % 17])              # 0 .. R / 8 hot entries, on both sides of the trim
    cus, _ = ctx.device_props()
    assert shape_rows(R, 384, 3 * cus, False, forced=(1, 8)) == 256 and shape_rows(64, 384, 3 * cus, False, forced=(1, 8)) == 0
    elig, _ = check(ctx, table, case, dict(VPIN_MSM_STRIP_SHAPE="1,8"), take=lambda n: shape_rows(R, n, 3 * cus, False, forced=(1, 8)))
    assert int(elig.sum()) == 384


def test_trimming_on_a_cu_masked_context(ctx, table):
    """one CU per XCD: 24 workgroup slots, so strip_shape's masked branch takes 3 groups x 8 strips = 768 of more than 768
    eligible rows of R = 1024 and trims the rest; oracle on a sample: first, last, both sides of the trim, hot rows, padding"""
    import vpin_amd
    cus, _ = ctx.device_props()
    mask = _cus(0, 1)
    enabled = len([k for k in mask if k < cus])
    assert enabled == 8, (cus, mask)
    slots = 3 * enabled
    case = Case(np.random.default_rng(7), 1024, 262144, (11, None, 70))   # 2048 rows: 768 + 3 x 256 + 512
    rng = np.random.default_rng(70)
    for row in range(3, 768, 7):
        sparse(case, rng, row, 200)                                       # not eligible: the trim falls inside the col-derefs rows
    for r in range(0, 256, 5):
        case.set_hot(0, r, rng.permutation(1024)[:1 + r % 128])
        case.set_hot(2, r, rng.permutation(1024)[:128 + r % 2])
    Z = case.build()
    listed = np.nonzero(case.eligible(Z))[0]
    assert len(listed) > 768 and shape_rows(1024, len(listed), slots, True) == 768
    sample = [0, 3, case.L - 1, int(listed[767]), int(listed[768]), int(listed[255]), int(listed[256]), int(listed[-1]),
              case.mrow(0, 5), case.mrow(2, 5), case.mrow(2, 10), case.mrow(1, 255), 6 * case.rpv]
    with vpin_amd.Context(0, cu_mask=mask) as small:   # the table is the registry's: one per device and label, whatever the context
        check(small, table, case, dict(), take=lambda n: shape_rows(1024, n, slots, True), sample=sample)
