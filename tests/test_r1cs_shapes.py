"""The structural instances of r1cs_shapes.py have the properties they are named for, computed from their triplets alone, and
the plain Python-integer reference of the three sparse loops agrees exactly with the oracle's C loops on every case small
enough -- which is what licenses the C loops as the reference of the large cases (test_gpu_r1cs_shapes.py).  CPU only: these
are requirements on the inputs and the references, not measurements of the code under test."""
import json
import os

import numpy as np
import pytest

import gadgets_model as GM
import oracle_lib as O
import pymodel as M
import r1cs_shapes as S

Q = M.Q
PY_REF_MAX = 200_000  # entries up to which the Python-integer reference is affordable


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = S.build(name)
        return cache[name]
    return get


def test_value_table_and_field_sum():
    assert S.TABLE_INTS[:3] == [0, 1, Q - 1] and len(set(S.TABLE_INTS)) == len(S.TABLE_INTS)
    assert all((S.TABLE_INTS[a] + S.TABLE_INTS[b]) % Q == 0 for a, b in S.CANCEL.items())
    rng = S.rng_of("add_mod_q")
    a, b = S.random_table(rng, 300), S.random_table(rng, 300)
    a[:4] = M.ints_to_table([0, Q - 1, Q - 1, 1])
    b[:4] = M.ints_to_table([0, Q - 1, 1, Q - 1])
    ai, bi = (M.from_mont_limbs(r) * M.R % Q for r in a), (M.from_mont_limbs(r) * M.R % Q for r in b)  # the limbs' own values
    got = S.add_mod_q(a, b)
    for x, y, g in zip(ai, bi, got):
        assert sum(int(l) << (64 * i) for i, l in enumerate(g)) == (x + y) % Q


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_instance_form(name, cases):
    """the dict of gadgets_model.instance_new: keys, dtypes, dimensions Instance::new can emit, vars = para + input"""
    inst = cases(name)
    model = GM.instance_new(GM.build_point_add(GM.synthetic_add_ops(1, 1)))
    assert set(inst) == set(model)
    nc, nv, ni = inst["num_cons"], inst["num_vars"], inst["num_inputs"]
    assert nc >= 2 and nc & (nc - 1) == 0 and nv & (nv - 1) == 0 and ni < nv
    for k in "ABC":
        rows, cols, vals = inst[k]
        for got, ref in zip(inst[k], model[k]):
            assert got.dtype == ref.dtype and got.flags["C_CONTIGUOUS"]
        assert len(rows) == len(cols) == len(vals) and vals.shape == (len(rows), 4)
        assert rows.max(initial=0) < nc and cols.max(initial=0) < 2 * nv
    for k in ("vars_para", "vars_input", "vars", "inputs"):
        assert inst[k].dtype == model[k].dtype and inst[k].shape == ((ni if k == "inputs" else nv), 4)
    pick = S.rng_of(name + "/pick").integers(0, nv, size=min(nv, 50))
    for i in pick:
        p, x, v = (M.from_mont_limbs(inst[k][i]) for k in ("vars_para", "vars_input", "vars"))
        assert (p + x) % Q == v
    assert S.build(name)["A"][0].tobytes() == inst["A"][0].tobytes()  # deterministic from the name


def test_col_lengths(cases):
    inst = cases("col_lengths")
    nv = inst["num_vars"]
    assert inst["num_cons"] == 1 << 18 and nv == S.COL_LENGTHS_NV
    hist = {k: S.col_histogram(inst, k) for k in "ABC"}
    for k in "ABC":
        assert {c: int(n) for c, n in enumerate(hist[k]) if n} == S.COL_LENGTHS[k]
        rows, cols, _ = inst[k]
        assert len(np.unique(rows.astype(np.int64) * 2 * nv + cols)) == len(rows)  # distinct rows within every column
    assert set(hist["A"]) >= {1, 255, 256, 257, 2047, 2048, 2049, 4097, 64 * S.CHUNK + 1}
    long_in = lambda c: {k for k in "ABC" if hist[k][c] > S.LONG_COL}  # noqa: E731
    assert long_in(700) == {"A"} and long_in(nv) == {"B"} and long_in(2 * nv - 1) == {"C"}
    assert long_in(0) == long_in(701) == {"A", "B", "C"}
    assert 0 < hist["A"][nv] <= S.LONG_COL and 0 < hist["C"][nv] <= S.LONG_COL          # short where it is not long,
    assert hist["A"][2 * nv - 1] == S.LONG_COL and 0 < hist["B"][2 * nv - 1]            # not absent
    assert (64 * S.CHUNK + 1 + S.CHUNK - 1) // S.CHUNK == 65                             # a second step of the 64-lane sum


@pytest.mark.parametrize("name", ["wave_patterns", "wave_patterns_shuffled"])
def test_wave_patterns(name, cases):
    inst = cases(name)
    assert inst["num_cons"] == 1 << 10 and 2 * inst["num_vars"] == 1 << 10
    nnz = [len(inst[k][0]) for k in "ABC"]
    assert nnz[0] % 64 == 1 and nnz[1] % 64 == 63
    rh, ch = S.row_histogram(inst, "C"), S.col_histogram(inst, "C")
    assert rh.max() == ch.max() == S.HOT_TAIL
    if name.endswith("shuffled"):
        return  # the same triplets in another order
    for side, k in ((0, "A"), (1, "B")):
        groups = S.wave_group_sizes(inst[k][side])
        assert groups[0] == (64,) and groups[1] == () and groups[2] == S.FOUR_GROUPS and groups[3] == S.SIX_GROUPS
        assert sum(S.SIX_GROUPS) < 64 and len(S.SIX_GROUPS) - 4 >= 2 and min(S.SIX_GROUPS) == 2 and max(S.SIX_GROUPS) == 20
    # the hottest row and column of C occur in the last, partial wave only
    last = (nnz[2] // 64) * 64
    assert 0 < nnz[2] - last < 64
    for side, h in ((0, rh), (1, ch)):
        keys = inst["C"][side]
        hot = int(np.argmax(h))
        assert hot not in set(keys[:last].tolist()) and int(np.sum(keys[last:] == hot)) == S.HOT_TAIL
        assert S.wave_group_sizes(keys)[:-1] == [()] * (last // 64)


@pytest.mark.parametrize("name", sorted(S.SCAN_DIMS))
def test_scan_sizes(name, cases):
    inst = cases(name)
    nc, ncols = inst["num_cons"], 2 * inst["num_vars"]
    assert (nc, inst["num_vars"]) == S.SCAN_DIMS[name]
    assert sorted({d for v in S.SCAN_DIMS.values() for d in (v[0], 2 * v[1])}) == [2, 4, 2048, 4096, 1 << 22]
    rows, cols, _ = inst["A"]
    have = set(zip(rows.tolist(), cols.tolist()))
    for r in S.SCAN_EDGES + (nc - 1,):
        for c in S.SCAN_EDGES + (ncols - 1,):
            if r < nc and c < ncols:
                assert (r, c) in have
    assert set(inst["B"][0].tolist()) == {0} and set(inst["C"][1].tolist()) == {ncols - 1}
    assert all(len(inst[k][0]) < 4000 for k in "ABC")
    blocks = lambda n: (n + S.SCAN_ELEMS - 1) // S.SCAN_ELEMS  # noqa: E731
    if max(nc, ncols) == 1 << 22:
        assert blocks(max(nc, ncols)) > 1024  # scan_sums_kernel: more than one block total per thread


def test_grid_stride(cases):
    inst = cases("grid_stride")
    assert inst["num_cons"] == 1 << 16 and 2 * inst["num_vars"] == 1 << 16
    assert len(inst["A"][0]) == S.GRID_ROUND + 4097 == S.GRID_NNZ
    hot = np.flatnonzero(inst["A"][1] == S.GRID_HOT_COL)
    assert len(hot) == S.GRID_NNZ // 3 and hot.min() < S.GRID_ROUND <= hot.max()


def test_degenerate_content(cases):
    assert [len(cases("c_empty")[k][0]) for k in "ABC"][2] == 0 and len(cases("c_empty")["A"][0]) > 0
    assert [len(cases("all_empty")[k][0]) for k in "ABC"] == [0, 0, 0]
    inst = cases("dup_cancel")
    rows, cols, vals = S.triplets(inst, "A")
    sums = {}
    for r, c, v in zip(rows, cols, vals):
        sums[(r, c)] = (sums.get((r, c), 0) + v) % Q
    assert len(sums) < len(rows) and set(sums.values()) == {0} and 0 not in vals
    rows, cols, vals = S.triplets(inst, "B")
    assert len(set(zip(rows, cols))) < len(rows)
    inst = cases("explicit_zeros")
    assert set(S.triplets(inst, "A")[2]) == {0} and 0 < S.triplets(inst, "B")[2].count(0) < 200
    inst = cases("zero_witness")
    z = S.build_z(inst)
    assert not z[np.unique(inst["A"][1])].any() and z[inst["num_vars"]].any()
    assert set(inst["B"][1].tolist()) & set(S.ZERO_WITNESS_COLS) and z[np.unique(inst["B"][1])].any()


def test_proof_shapes(cases):
    nm = {name: S.shape_of(cases(name)) for name in S.SMALL_PROOF_CASES + tuple(S.TINY)}
    assert nm["proof_n_lt_m"] == (64, 1024) and nm["proof_n_eq_m"] == (1024, 1024) and nm["proof_n_16m"] == (256, 16)
    assert sum(len(cases("proof_n_lt_m")[k][0]) for k in "ABC") < 100
    rows, cols, _ = cases("proof_n_16m")["A"]
    assert len(set(zip(rows.tolist(), cols.tolist()))) < len(rows)
    assert (cases("proof_2x2048")["num_cons"], cases("proof_2x2048")["num_vars"]) == (2, 1 << 11)
    assert (cases("proof_4096x2")["num_cons"], cases("proof_4096x2")["num_vars"]) == (1 << 12, 2)
    assert all(n <= 1 << 12 for n, _ in nm.values())
    assert [sum(S.TINY[f"tiny_{t}"]) for t in range(5)] == [0, 1, 2, 3, 4]
    assert all(nm[f"tiny_{t}"][0] < 4 for t in range(5)) and nm["tiny_4_one_matrix"][0] == nm["tiny_3_one_matrix"][0] == 4
    assert all(m >= 4 for _, m in nm.values())
    # exactly one of them is satisfied by its random witness: the one built to be
    assert [name for name in S.SMALL_PROOF_CASES if O.is_sat(cases(name))] == ["sat_small"]


@pytest.mark.parametrize("name", sorted(S.HOT_CASES))
def test_hot_column_counts(name, cases):
    inst = cases(name)
    nv = inst["num_vars"]
    n, m = S.shape_of(inst)
    assert n == S.HOT_N >= S.HOT_MIN_N and m == 2 * S.HOT_DIM and S.HOT_T == n // 64
    spec, expect = S.HOT_CASES[name]
    for k, (nnz, n0, n1), want in zip("ABC", spec, expect):
        h = S.col_histogram(inst, k)
        assert len(inst[k][0]) == nnz
        c0, c1 = int(h[nv]), int(h[nv + 1])
        if n0 is not None:
            assert (c0, c1) == (n0, n1)
        # the rule of spark_find_hot_cols, stated on the counts: the larger candidate (the first on a tie) if it has N/64
        best = 1 if c1 > c0 else 0
        assert (best if (c1, c0)[1 - best] >= S.HOT_T else None) == want
    if name == "hot_none":
        assert all(max(S.col_histogram(inst, k)[nv:nv + 2]) < S.HOT_T // 8 for k in "ABC")
    if name == "hot_threshold":
        assert S.col_histogram(inst, "A")[nv] == 0
        assert S.col_histogram(inst, "B")[nv] == S.HOT_T and S.col_histogram(inst, "C")[nv] == S.HOT_T - 1
    if name == "hot_both":
        c = [S.col_histogram(inst, k)[nv:nv + 2] for k in "ABC"]
        assert all(x.min() >= S.HOT_T for x in c) and c[0][0] > c[0][1] and c[1][1] > c[1][0] and c[2][0] == c[2][1]


def test_rank_columns(cases):
    inst = cases("ranks")
    hist = {k: S.col_histogram(inst, k) for k in "ABC"}
    longs = {k: set(np.flatnonzero(hist[k] > S.LONG_COL).tolist()) for k in "ABC"}
    last = 2 * inst["num_vars"] - 1
    for dim in (inst["num_cons"], 2 * inst["num_vars"]):  # worlds 2 and 4 split by residue from here on
        assert dim.bit_length() - 1 - 2 >= S.RANK_SPLIT_MIN
    assert longs == {"A": {4, last}, "B": {8, last}, "C": {513, last}}
    assert {c % 4 for v in longs.values() for c in v} == {0, 1, 3}
    assert 0 < hist["A"][8] <= S.LONG_COL and 0 < hist["C"][8] <= S.LONG_COL      # long in B only
    assert 0 < hist["A"][513] <= S.LONG_COL and hist["B"][513] == S.LONG_COL      # long in C only
    assert hist["B"][last] > S.CHUNK and hist["C"][513] > S.CHUNK                 # more than one chunk


PY_VS_C = sorted(n for n in S.CASES if n not in S.HOT_CASES and n != "grid_stride")


@pytest.mark.parametrize("name", PY_VS_C)
def test_python_reference_agrees_with_the_c_loops(name, cases):
    inst = cases(name)
    assert sum(len(inst[k][0]) for k in "ABC") <= PY_REF_MAX
    nc, ncols = inst["num_cons"], 2 * inst["num_vars"]
    z = S.build_z(inst)
    for got, exp in zip(S.ref_multiply_vec(inst, z), S.oracle_multiply_vec(inst, z)):
        assert np.array_equal(S.dense(got, nc), exp)
    rx, ry, _, _ = S.challenge_points(name, inst)
    erx, ery = O.eq_evals(rx), O.eq_evals(ry)
    for got, exp in zip(S.ref_eval_tables(inst, erx), S.oracle_eval_tables(inst, erx)):
        assert np.array_equal(S.dense(got, ncols), exp)
    assert np.array_equal(M.ints_to_table(S.ref_evaluate(inst, erx, ery)), S.oracle_evaluate(inst, rx, ry))


def test_combine_tables():
    inst = S.build("dup_cancel")
    rx, _, _, rabc = S.challenge_points("dup_cancel", inst)
    erx = O.eq_evals(rx)
    exp = S.dense(S.ref_eval_table(inst, erx, rabc), 2 * inst["num_vars"])
    assert np.array_equal(S.combine_tables(S.oracle_eval_tables(inst, erx), rabc), exp)


def test_eq_table_of_the_python_model_is_the_oracles():
    """the eq tables the references are fed with: the tensor-product statement of pymodel against the oracle's"""
    rng = S.rng_of("eq")
    r = S.random_table(rng, 5)
    assert np.array_equal(M.ints_to_table(M.eq_evals(M.table_to_ints(r))), O.eq_evals(r))


# ---- the committed digests ----------------------------------------------------------------------------------------------------

def test_shape_digests_regenerate(golden_dir):
    """make_r1cs_shape_digests.py reproduces the committed file byte for byte: the small entries always, the N = 2^20 ones
    (minutes of oracle time each) with VPIN_SHAPE_DIGESTS_FULL=1"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_r1cs_shape_digests", os.path.join(golden_dir, "make_r1cs_shape_digests.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    with open(mk.OUT) as f:
        text = f.read()
    doc = json.loads(text)
    assert set(doc) == set(mk.SMALL) | set(mk.LARGE) | {"_source"}
    assert "s" in doc["_source"] and all(k in doc["_source"] for k in mk.LARGE)  # the measured oracle time per large case
    again = dict(doc)
    names = mk.SMALL + (mk.LARGE if os.environ.get("VPIN_SHAPE_DIGESTS_FULL") == "1" else ())
    for name in names:
        again[name] = mk.entry(name, threads=4)[0]
    assert mk.render(again) == text
    assert [k for k in mk.SMALL + mk.LARGE if doc[k]["is_sat"]] == ["sat_small", "tiny_4_one_matrix"]
