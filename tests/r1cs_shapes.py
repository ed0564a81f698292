"""Named R1CS instances whose structure no gadget produces, and a plain Python-integer reference of the three sparse loops.

The gadget builders (gadgets_model.py) emit one sparsity pattern: one hot column (the constant 1), short rows, triplets in
the builder's order.  The sparse path of the product (vpin_amd/csrc/r1cs.hip, spark.hip's hot-column search, trace.hip) has
branches that pattern never reaches: the cases here are built, deterministically from their names, to reach them.  Every
case is an `inst` dict in exactly the form gadgets_model.instance_new returns, so oracle_lib.make_r1cs, Context.sat_prove,
Context.snark_prove and Context.r1cs_upload take it unchanged.  tests/test_r1cs_shapes.py asserts that each case has the
property it is named for.

The reference states the definitions of the Spartan source that r1cs.hip cites, by scatter in plain `% q` integers:
    SparseMatPolynomial::multiply_vec               (Mz)[row] += val * z[col]
    SparseMatPolynomial::compute_eval_table_sparse  M(rx, .)[col] += rx[row] * val, then r_A*A + r_B*B + r_C*C
    SparseMatPolynomial::evaluate_with_tables       M(rx, ry) = sum rx[row] * ry[col] * val
It works on sparse dictionaries (index -> integer), so an instance of 2^22 rows with a few thousand entries stays cheap.
"""
import zlib

import numpy as np

import pymodel as M

Q = M.Q

# the constants of r1cs.hip / spark.hip the cases are laid out against
WAVE = 64
LONG_COL = 256       # kLongCol: a column with MORE entries is split into chunks
CHUNK = 2048         # kChunk
SCAN_ELEMS = 2048    # one block of the prefix sum
GRID_ROUND = 4096 * 256  # triplets one round of the histogram / scatter grid covers
HOT_MIN_N = 1 << 20  # spark_find_hot_cols acts from here; threshold count >= N / 64


def _fixed_randoms(n, tag):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return [int.from_bytes(rng.bytes(40), "little") % Q for _ in range(n)]


# the small value table: 0, 1, q-1, a cancelling pair of small and of random elements, a few more random ones
_R = _fixed_randoms(4, "value table")
TABLE_INTS = [0, 1, Q - 1, 2, Q - 2, _R[0], Q - _R[0], _R[1], _R[2], _R[3]]
TABLE = M.ints_to_table(TABLE_INTS)
V_ZERO, V_ONE, V_MINUS_ONE = 0, 1, 2
CANCEL = {1: 2, 2: 1, 3: 4, 4: 3, 5: 6, 6: 5}  # table index -> index of its negative
_Q_LIMBS = np.array([(Q >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def add_mod_q(a, b):
    """(n,4) u64 limb tables of values < q -> a + b mod q, limb-wise (Montgomery form is linear, so this is the field sum)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    s = np.empty_like(a)
    carry = np.zeros(a.shape[0], dtype=np.uint64)
    for i in range(4):
        t = a[:, i] + b[:, i]
        c1 = t < a[:, i]
        u = t + carry
        c2 = u < t
        s[:, i] = u
        carry = (c1 | c2).astype(np.uint64)
    # a, b < q < 2^253: no carry out of the top limb.  s >= q ?
    ge = np.ones(a.shape[0], dtype=bool)
    decided = np.zeros(a.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        gt, lt = s[:, i] > _Q_LIMBS[i], s[:, i] < _Q_LIMBS[i]
        ge = np.where(~decided & lt, False, ge)
        decided |= gt | lt
    out = s.copy()
    borrow = np.zeros(a.shape[0], dtype=np.uint64)
    for i in range(4):
        t = s[:, i] - _Q_LIMBS[i]
        b1 = s[:, i] < _Q_LIMBS[i]
        u = t - borrow
        b2 = t < borrow
        out[:, i] = np.where(ge, u, s[:, i])
        borrow = (b1 | b2).astype(np.uint64)
    return out


def random_table(rng, n):
    """n random field elements as Montgomery limbs: any value < 2^252 < q is the Montgomery form of some element."""
    t = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 60) - 1)
    return np.ascontiguousarray(t)


def _mat(rows, cols, vidx):
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    vals = np.ascontiguousarray(TABLE[np.asarray(vidx, dtype=np.int64)]) if len(rows) else np.zeros((0, 4), dtype=np.uint64)
    assert rows.shape == cols.shape and vals.shape == (len(rows), 4)
    return rows, cols, vals


def _empty():
    return _mat([], [], [])


def _vidx(rng, n, zeros=True):
    return rng.integers(0 if zeros else 1, len(TABLE_INTS), size=n)


def _inst(name, nc, nv, ni, mats, zero_vars=()):
    """the instance_new dict: random witness halves, vars = vars_para + vars_input mod q, random inputs"""
    assert nc >= 2 and nc & (nc - 1) == 0 and nv & (nv - 1) == 0 and ni < nv
    rng = rng_of(name + "/witness")
    para, inp = random_table(rng, nv), random_table(rng, nv)
    if len(zero_vars):
        zv = np.asarray(sorted(zero_vars), dtype=np.int64)
        para[zv] = 0
        inp[zv] = 0
    out = dict(num_cons=nc, num_vars=nv, num_inputs=ni, num_cons_unpadded=nc, num_vars_unpadded=nv)
    for k, m in zip("ABC", mats):
        rows, cols, vals = m
        assert rows.max(initial=0) < nc and cols.max(initial=0) < 2 * nv
        out[k] = (rows, cols, vals)
    out["vars_para"], out["vars_input"], out["vars"] = para, inp, add_mod_q(para, inp)
    out["inputs"] = random_table(rng, ni) if ni else np.zeros((0, 4), dtype=np.uint64)
    return out


def _shuffled(rng, rows, cols, vidx):
    p = rng.permutation(len(rows))
    return np.asarray(rows)[p], np.asarray(cols)[p], np.asarray(vidx)[p]


# ---- column lengths ---------------------------------------------------------------------------------------------------------

COL_LENGTHS_NV = 512
# matrix -> {column: length}.  A has every length of the list; column 512 = num_vars is long in B only, 1023 = 2*num_vars - 1
# in C only, 700 in A only, 0 and 701 in all three; 700 and 701 are adjacent long columns
COL_LENGTHS = {
    "A": {0: 64 * CHUNK + 1, 5: 1, 6: 2048, 7: 2049, 8: 4097, 512: 255, 700: 257, 701: 2047, 1023: 256},
    "B": {0: 4097, 300: 256, 512: 2048, 701: 257, 1023: 1},
    "C": {0: 2049, 9: 255, 512: 1, 701: 4097, 1023: 2049},
}


def _col_lengths(name):
    nc, nv = 1 << 18, COL_LENGTHS_NV
    rng = rng_of(name)
    mats = []
    for k in "ABC":
        rows, cols = [], []
        for c, n in COL_LENGTHS[k].items():
            start = int(rng.integers(0, nc))
            rows.append((start + 7 * np.arange(n, dtype=np.int64)) % nc)  # distinct rows: 7 is odd, nc a power of two
            cols.append(np.full(n, c, dtype=np.int64))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        mats.append(_mat(*_shuffled(rng, rows, cols, _vidx(rng, len(rows)))))
    return _inst(name, nc, nv, 1, mats)


# ---- wave patterns ----------------------------------------------------------------------------------------------------------

FOUR_GROUPS = (10, 8, 5, 3)          # exactly four repeated keys, the rest of the wave singletons
SIX_GROUPS = (20, 11, 7, 4, 3, 2)    # six repeated keys: at least two of them are left for the one-atomic-per-lane path
HOT_TAIL = 40                        # entries of the partial last wave that share the matrix's hottest key


def _wave_keys(rng, kind, fresh):
    """64 keys of one wave; fresh() hands out keys used nowhere else in the matrix"""
    if kind == "equal":
        return np.full(WAVE, fresh(), dtype=np.int64)
    if kind == "distinct":
        return np.array([fresh() for _ in range(WAVE)], dtype=np.int64)
    sizes = FOUR_GROUPS if kind == "four" else SIX_GROUPS
    keys = []
    for s in sizes:
        keys += [fresh()] * s
    keys += [fresh() for _ in range(WAVE - len(keys))]
    return rng.permutation(np.array(keys, dtype=np.int64))  # the groups' lanes interleave


WAVE_KINDS = ("equal", "distinct", "four", "six")


def _wave_side(rng, n_keys, tail):
    """(patterned keys, plain keys) of 4 full waves + `tail` more entries"""
    unused = list(rng.permutation(n_keys))
    fresh = unused.pop
    pat = np.concatenate([_wave_keys(rng, kind, fresh) for kind in WAVE_KINDS] + [np.array([fresh() for _ in range(tail)], dtype=np.int64)])
    plain = rng.integers(0, n_keys, size=len(pat))
    return pat, plain


def _wave_patterns(name, shuffle=False):
    nc, nv = 1 << 10, 1 << 9
    rng = rng_of("wave_patterns")
    # A: the layouts on the row side, nnz % 64 == 1.  B: on the column side, nnz % 64 == 63.
    ra, ca = _wave_side(rng, nc, 1)
    cb, rb = _wave_side(rng, 2 * nv, 63)
    # C: three waves of keys that occur once each, then a partial wave where the hottest row and column first appear
    unused_r, unused_c = list(rng.permutation(nc)), list(rng.permutation(2 * nv))
    hot_r, hot_c = unused_r.pop(), unused_c.pop()
    rc = [unused_r.pop() for _ in range(3 * WAVE)] + [hot_r] * HOT_TAIL + [unused_r.pop() for _ in range(5)]
    cc = [unused_c.pop() for _ in range(3 * WAVE)] + [unused_c.pop() for _ in range(5)] + [hot_c] * HOT_TAIL
    mats = []
    for r, c in ((ra, ca), (rb, cb), (rc, cc)):
        t = (np.asarray(r), np.asarray(c), _vidx(rng, len(r)))
        mats.append(_mat(*(_shuffled(rng, *t) if shuffle else t)))
    return _inst(name, nc, nv, 3, mats)


# ---- scan sizes -------------------------------------------------------------------------------------------------------------

SCAN_DIMS = {  # name -> (num_cons, num_vars): nrows or ncols = 2*num_vars at 2, 2048, 4096 and 2^22
    "scan_2x2048": (2, 1 << 10),
    "scan_2048x2": (1 << 11, 1),
    "scan_4096x4096": (1 << 12, 1 << 11),
    "scan_2x4m": (2, 1 << 21),
    "scan_4mx4": (1 << 22, 2),
}
SCAN_EDGES = (0, 2047, 2048, 2049)


def _edges(n):
    return sorted({e for e in SCAN_EDGES + (n - 1,) if e < n})


def _scan(name):
    nc, nv = SCAN_DIMS[name]
    ncols = 2 * nv
    rng = rng_of(name)
    er, ec = _edges(nc), _edges(ncols)
    k = 3000
    # A: every edge row with every edge column, then random entries
    ra = np.concatenate([np.repeat(er, len(ec)), rng.integers(0, nc, size=k)])
    ca = np.concatenate([np.tile(ec, len(er)), rng.integers(0, ncols, size=k)])
    # B: every entry in row 0.  C: every entry in the last column.
    cb = np.concatenate([ec, rng.integers(0, ncols, size=k)])
    rb = np.zeros(len(cb), dtype=np.int64)
    rc = np.concatenate([er, rng.integers(0, nc, size=k)])
    cc = np.full(len(rc), ncols - 1, dtype=np.int64)
    mats = [_mat(*_shuffled(rng, r, c, _vidx(rng, len(r)))) for r, c in ((ra, ca), (rb, cb), (rc, cc))]
    return _inst(name, nc, nv, 0 if nv == 1 else 1, mats)


# ---- second grid-stride round -----------------------------------------------------------------------------------------------

GRID_NNZ = GRID_ROUND + 4097
GRID_HOT_COL = 12345


def _grid_stride(name):
    nc, nv = 1 << 16, 1 << 15
    rng = rng_of(name)
    n = GRID_NNZ
    rows = rng.integers(0, nc, size=n)
    cols = rng.integers(0, 2 * nv, size=n)
    cols[cols == GRID_HOT_COL] = GRID_HOT_COL + 1
    cols[rng.permutation(n)[: n // 3]] = GRID_HOT_COL  # a third of the entries, spread over both rounds
    a = _mat(rows, cols, _vidx(rng, n))
    small = [_mat(rng.integers(0, nc, size=k), rng.integers(0, 2 * nv, size=k), _vidx(rng, k)) for k in (3001, 2999)]
    return _inst(name, nc, nv, 2, [a] + small)


# ---- degenerate content -----------------------------------------------------------------------------------------------------

def _random_mat(rng, nc, ncols, n, zeros=True):
    return _mat(rng.integers(0, nc, size=n), rng.integers(0, ncols, size=n), _vidx(rng, n, zeros))


def _c_empty(name):
    rng = rng_of(name)
    return _inst(name, 64, 64, 2, [_random_mat(rng, 64, 128, 150), _random_mat(rng, 64, 128, 97), _empty()])


def _all_empty(name):
    return _inst(name, 64, 64, 2, [_empty(), _empty(), _empty()])


def _dup_cancel(name):
    """every (row, col) of A occurs twice with values v and -v (A z = 0, A's eval table = 0); B has duplicates that do not
    cancel; C has a pair that cancels next to entries that stay"""
    rng = rng_of(name)
    nc, nv, n = 128, 64, 300
    r, c = rng.integers(0, nc, size=n), rng.integers(0, 2 * nv, size=n)
    v = rng.integers(1, 7, size=n)
    neg = np.array([CANCEL[int(x)] for x in v])
    a = _mat(*_shuffled(rng, np.concatenate([r, r]), np.concatenate([c, c]), np.concatenate([v, neg])))
    rb, cb = rng.integers(0, nc, size=40), rng.integers(0, 2 * nv, size=40)
    b = _mat(*_shuffled(rng, np.tile(rb, 5), np.tile(cb, 5), _vidx(rng, 200, zeros=False)))
    c_ = _mat([3, 9, 3, 9, 9], [70, 5, 70, 5, 5], [5, 7, 6, 8, 9])
    return _inst(name, nc, nv, 1, [a, b, c_])


def _explicit_zeros(name):
    """A holds explicit zeros only, B about half zeros, C one zero"""
    rng = rng_of(name)
    nc, nv = 128, 64
    a = _mat(rng.integers(0, nc, size=200), rng.integers(0, 2 * nv, size=200), np.zeros(200, dtype=np.int64))
    vb = _vidx(rng, 200, zeros=False)
    vb[rng.permutation(200)[:100]] = V_ZERO
    b = _mat(rng.integers(0, nc, size=200), rng.integers(0, 2 * nv, size=200), vb)
    c = _mat([5], [64], [V_ZERO])
    return _inst(name, nc, nv, 1, [a, b, c])


ZERO_WITNESS_COLS = tuple(range(3, 64, 4))


def _zero_witness(name):
    """A reads only columns where z is zero (the skip in the SpMV); B and C read them among others"""
    rng = rng_of(name)
    nc, nv = 128, 64
    zc = np.array(ZERO_WITNESS_COLS)
    a = _mat(rng.integers(0, nc, size=200), zc[rng.integers(0, len(zc), size=200)], _vidx(rng, 200, zeros=False))
    return _inst(name, nc, nv, 1, [a, _random_mat(rng, nc, 2 * nv, 200, False), _random_mat(rng, nc, 2 * nv, 200, False)],
                 zero_vars=ZERO_WITNESS_COLS)


# ---- whole-proof shapes -----------------------------------------------------------------------------------------------------

def _proof_random(name, nc, nv, nnz, ni=1):
    rng = rng_of(name)
    return _inst(name, nc, nv, ni, [_random_mat(rng, nc, 2 * nv, n) for n in nnz])


def _sat_small(name):
    """genuinely satisfied: A and B random, C = one entry per row on the constant-1 column with value (Az)_i * (Bz)_i"""
    rng = rng_of(name)
    nc, nv = 64, 64
    a, b = _random_mat(rng, nc, 2 * nv, 150, False), _random_mat(rng, nc, 2 * nv, 170, False)
    inst = _inst(name, nc, nv, 2, [a, b, _empty()])
    z = build_z(inst)
    az, bz, _ = ref_multiply_vec(inst, z)
    order = rng.permutation(nc)
    inst["C"] = (order.astype(np.uint32), np.full(nc, nv, dtype=np.uint32),
                 M.ints_to_table([az.get(int(i), 0) * bz.get(int(i), 0) % Q for i in order]))
    return inst


TINY = {  # name -> nnz of (A, B, C): total 0..4 (N = next_pow2(max nnz) < 4), and the smallest the SPARK encoding takes
    "tiny_0": (0, 0, 0), "tiny_1": (1, 0, 0), "tiny_2": (1, 1, 0), "tiny_3": (1, 1, 1), "tiny_4": (2, 1, 1),
    "tiny_4_one_matrix": (0, 4, 0), "tiny_3_one_matrix": (0, 0, 3),
}


def _tiny(name):
    return _proof_random(name, 4, 4, TINY[name])


# ---- N = 2^20: spark_find_hot_cols ------------------------------------------------------------------------------------------

HOT_N = 1 << 20
HOT_T = HOT_N // 64
HOT_DIM = 1 << 10
# name -> per matrix (nnz, count of column num_vars, count of column num_vars + 1), and what hot_cols() must return
# (0 = num_vars, 1 = num_vars + 1, None)
HOT_CASES = {
    "hot_none": (((HOT_N, None, None), (HOT_N - 1, None, None), (HOT_N // 2 + 1, None, None)), (None, None, None)),
    "hot_threshold": (((HOT_N, 0, 20000), (HOT_N - 1, HOT_T, 0), (HOT_N // 2 + 1, HOT_T - 1, 0)), (1, 0, None)),
    "hot_both": (((HOT_N, 40000, 30000), (HOT_N - 1, 30000, 40000), (HOT_N // 2 + 1, 25000, 25000)), (0, 1, 0)),
}


def _hot(name, dim=HOT_DIM):
    rng = rng_of(name)
    nc = nv = dim
    mats = []
    for nnz, n0, n1 in HOT_CASES[name][0]:
        rows = rng.integers(0, nc, size=nnz)
        cols = rng.integers(0, 2 * nv, size=nnz)  # uniform: about nnz / (2 nv) per column
        if n0 is not None:
            other = rng.integers(0, nv, size=nnz)  # the witness half: neither candidate
            cand = (cols == nv) | (cols == nv + 1)
            cols[cand] = other[cand]
            p = rng.permutation(nnz)
            cols[p[:n0]] = nv
            cols[p[n0:n0 + n1]] = nv + 1
        mats.append(_mat(rows, cols, _vidx(rng, nnz)))
    return _inst(name, nc, nv, 2, mats)


# ---- several ranks ----------------------------------------------------------------------------------------------------------

# long columns in the residue classes 0, 1 and 3 mod 4 and a long last column; long in B only (8), in C only (513).
# The provers split the sat proof's tables by residue only when a rank's share has 2^12 entries: 2^14 rows and columns for 4 ranks
RANK_NC, RANK_NV, RANK_SPLIT_MIN = 1 << 14, 1 << 13, 12
RANK_LAST = 2 * RANK_NV - 1
RANK_COLS = {
    "A": {4: 300, 8: 100, 513: 7, RANK_LAST: 257, 2: 256},
    "B": {8: 300, 513: 256, RANK_LAST: 2100, 77: 3},
    "C": {513: 2100, 8: 1, RANK_LAST: 258, 6: 255},
}


def _ranks(name):
    nc, nv = RANK_NC, RANK_NV
    rng = rng_of(name)
    mats = []
    for k in "ABC":
        rows, cols = [rng.integers(0, nc, size=500)], [rng.integers(16, 500, size=500)]
        for c, n in RANK_COLS[k].items():
            rows.append(rng.integers(0, nc, size=n))
            cols.append(np.full(n, c, dtype=np.int64))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        mats.append(_mat(*_shuffled(rng, rows, cols, _vidx(rng, len(rows)))))
    return _inst(name, nc, nv, 2, mats)


# ---- the registry -----------------------------------------------------------------------------------------------------------

CASES = {
    "col_lengths": _col_lengths,
    "wave_patterns": _wave_patterns,
    "wave_patterns_shuffled": lambda name: _wave_patterns(name, shuffle=True),
    "grid_stride": _grid_stride,
    "c_empty": _c_empty,
    "all_empty": _all_empty,
    "dup_cancel": _dup_cancel,
    "explicit_zeros": _explicit_zeros,
    "zero_witness": _zero_witness,
    "proof_2x2048": lambda name: _proof_random(name, 2, 1 << 11, (300, 211, 2)),
    "proof_4096x2": lambda name: _proof_random(name, 1 << 12, 2, (300, 211, 129)),
    "proof_n_lt_m": lambda name: _proof_random(name, 1 << 10, 1 << 9, (40, 33, 17)),       # N = 64 < M = 1024
    "proof_n_eq_m": lambda name: _proof_random(name, 1 << 10, 1 << 9, (1000, 513, 600)),   # N = M = 1024
    "proof_n_16m": lambda name: _proof_random(name, 16, 8, (250, 129, 200)),               # N = 256 = 16 M: duplicates
    "sat_small": _sat_small,
    "ranks": _ranks,
}
CASES.update({k: _scan for k in SCAN_DIMS})
CASES.update({k: _tiny for k in TINY})
CASES.update({k: _hot for k in HOT_CASES})

SMALL_PROOF_CASES = ("wave_patterns_shuffled", "proof_2x2048", "proof_4096x2", "proof_n_lt_m", "proof_n_eq_m", "proof_n_16m",
                     "sat_small")


def build(name):
    return CASES[name](name)


def shape_of(inst):
    """(N, M) of the SPARK encoding: N = next_pow2(max nnz) (at least 1), M = 2^max(log2 num_cons, log2 2*num_vars)"""
    n = 1
    while n < max(len(inst[k][0]) for k in "ABC"):
        n *= 2
    return n, max(inst["num_cons"], 2 * inst["num_vars"])


# ---- the Python-integer reference -------------------------------------------------------------------------------------------

def ints_at(table, idx):
    """{i: canonical integer of table[i]} for the distinct i of idx"""
    return {int(i): M.from_mont_limbs(table[int(i)]) for i in np.unique(np.asarray(idx, dtype=np.int64))}


def _val_ints(vals):
    cache, out = {}, []
    for b in np.ascontiguousarray(vals).view(np.dtype((np.void, 32))).ravel():
        k = b.tobytes()
        if k not in cache:
            cache[k] = M.from_mont_limbs(np.frombuffer(k, dtype=np.uint64))
        out.append(cache[k])
    return out


def triplets(inst, k):
    rows, cols, vals = inst[k]
    return [int(r) for r in rows], [int(c) for c in cols], _val_ints(vals)


def build_z(inst):
    """z = [vars | 1 | inputs | 0 ..] as a (2*num_vars, 4) table"""
    nv, ni = inst["num_vars"], inst["num_inputs"]
    z = np.zeros((2 * nv, 4), dtype=np.uint64)
    z[:nv] = inst["vars"]
    z[nv] = M.to_mont_limbs(1)
    z[nv + 1:nv + 1 + ni] = inst["inputs"]
    return z


def ref_multiply_vec(inst, z):
    """[Az, Bz, Cz] as {row: integer}: (Mz)[row] += val * z[col]"""
    out = []
    for k in "ABC":
        rows, cols, vals = triplets(inst, k)
        zi = ints_at(z, cols)
        mz = {}
        for r, c, v in zip(rows, cols, vals):
            mz[r] = (mz.get(r, 0) + v * zi[c]) % Q
        out.append(mz)
    return out


def ref_eval_tables(inst, evals_rx):
    """[A(rx, .), B(rx, .), C(rx, .)] as {col: integer}: M(rx, .)[col] += rx[row] * val"""
    out = []
    for k in "ABC":
        rows, cols, vals = triplets(inst, k)
        ri = ints_at(evals_rx, rows)
        t = {}
        for r, c, v in zip(rows, cols, vals):
            t[c] = (t.get(c, 0) + ri[r] * v) % Q
        out.append(t)
    return out


def ref_eval_table(inst, evals_rx, r_abc):
    """{col: integer} of r_A * A(rx, .) + r_B * B(rx, .) + r_C * C(rx, .)"""
    comb = {}
    for t, rm in zip(ref_eval_tables(inst, evals_rx), r_abc):
        for c, x in t.items():
            comb[c] = (comb.get(c, 0) + rm * x) % Q
    return comb


def ref_evaluate(inst, evals_rx, evals_ry):
    """[A(rx, ry), B(rx, ry), C(rx, ry)]: sum of rx[row] * ry[col] * val"""
    out = []
    for k in "ABC":
        rows, cols, vals = triplets(inst, k)
        ri, ci = ints_at(evals_rx, rows), ints_at(evals_ry, cols)
        out.append(sum(ri[r] * ci[c] * v for r, c, v in zip(rows, cols, vals)) % Q)
    return out


def dense(d, n):
    """{index: integer} -> (n,4) table"""
    out = np.zeros((n, 4), dtype=np.uint64)
    for i, x in d.items():
        out[i] = M.to_mont_limbs(x)
    return out


# ---- the oracle's C loops (the reference of the cases too large for Python integers; test_r1cs_shapes.py licenses them) --------

def oracle_multiply_vec(inst, z):
    import ctypes as C
    import oracle_lib as O
    r = O.make_r1cs(inst)
    out = [np.zeros((inst["num_cons"], 4), dtype=np.uint64) for _ in range(3)]
    O.lib().oracle_r1cs_multiply_vec(C.byref(r), O.ptr(np.ascontiguousarray(z)), *[O.ptr(e) for e in out])
    return out


def oracle_eval_tables(inst, evals_rx):
    import ctypes as C
    import oracle_lib as O
    r = O.make_r1cs(inst)
    out = [np.zeros((2 * inst["num_vars"], 4), dtype=np.uint64) for _ in range(3)]
    O.lib().oracle_r1cs_eval_table_sparse(C.byref(r), O.ptr(np.ascontiguousarray(evals_rx)), *[O.ptr(t) for t in out])
    return out


def oracle_evaluate(inst, rx, ry):
    import ctypes as C
    import oracle_lib as O
    r = O.make_r1cs(inst)
    ev = np.zeros((3, 4), dtype=np.uint64)
    O.lib().oracle_r1cs_evaluate(C.byref(r), O.ptr(np.ascontiguousarray(rx)), O.ptr(np.ascontiguousarray(ry)), O.ptr(ev))
    return ev


def combine_tables(tabs, r_abc):
    """r_A * tabs[0] + r_B * tabs[1] + r_C * tabs[2] as a table (Python integers on the rows that are not all zero)"""
    nz = np.flatnonzero(np.any(tabs[0] != 0, axis=1) | np.any(tabs[1] != 0, axis=1) | np.any(tabs[2] != 0, axis=1))
    out = np.zeros_like(tabs[0])
    for i in nz:
        out[i] = M.to_mont_limbs(sum(rm * M.from_mont_limbs(t[i]) for rm, t in zip(r_abc, tabs)) % Q)
    return out


def challenge_points(name, inst):
    """random rx (log2 num_cons), ry (log2 2*num_vars) and (r_A, r_B, r_C) as tables and integers"""
    rng = rng_of(name + "/points")
    nx, ny = inst["num_cons"].bit_length() - 1, (2 * inst["num_vars"]).bit_length() - 1
    rx, ry, rabc = random_table(rng, nx), random_table(rng, ny), random_table(rng, 3)
    return rx, ry, rabc, M.table_to_ints(rabc)


# ---- the properties the cases are named for, from the triplets alone ---------------------------------------------------------

def col_histogram(inst, k):
    return np.bincount(inst[k][1].astype(np.int64), minlength=2 * inst["num_vars"])


def row_histogram(inst, k):
    return np.bincount(inst[k][0].astype(np.int64), minlength=inst["num_cons"])


def wave_group_sizes(keys):
    """per wave of 64 consecutive triplets: the sorted sizes (largest first) of the keys that occur more than once in it"""
    out = []
    for w in range(0, len(keys), WAVE):
        _, cnt = np.unique(np.asarray(keys[w:w + WAVE]), return_counts=True)
        out.append(tuple(sorted((int(x) for x in cnt if x > 1), reverse=True)))
    return out
