"""Whole proofs (Context.sat_prove and Context.snark_prove from host triplets) on the structural instances of r1cs_shapes.py:
shuffled triplet order (an address's accesses interleave across A, B and C in trace.hip's sort), num_cons against num_vars at
both extremes, N < M, N = M, N = 16 M, the smallest encodings, the N = 2^20 cases where spark_find_hot_cols acts, and an
instance with long columns in several residue classes proved by 2, 3 and 4 ranks.  Small cases against the oracle run live,
byte for byte; the N = 2^20 ones against tests/golden/r1cs_shape_digests.json (the oracle needs most of a minute for each)."""
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import oracle_lib as O
import r1cs_shapes as S

pytestmark = pytest.mark.gpu

VPIN_ESHAPE = -5
SEED_C = bytes(range(64))
SEED_P = bytes((7 * i + 3) % 256 for i in range(64))
SEEDS_2 =(bytes(range(64)), bytes((5 * i + 1) % 256 for i in range(64)))  # the second fixed pair of the suite (smoke)


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def digests(golden_dir):
    with open(os.path.join(golden_dir, "r1cs_shape_digests.json")) as f:
        return json.load(f)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _digest(res):
    return dict(proof=_sha(res["proof"]), comm=_sha(res["comm"]), comm_para=_sha(np.ascontiguousarray(res["comm_para"]).tobytes()),
                comm_input=_sha(np.ascontiguousarray(res["comm_input"]).tobytes()), proof_len=len(res["proof"]))


def check_snark(ctx, inst, seeds):
    got = ctx.snark_prove(inst, *seeds)
    exp = O.snark_prove(inst, *seeds)
    assert len(exp["proof"]) > 0 and len(exp["comm"]) > 0
    assert got["comm"] == exp["comm"]
    assert np.array_equal(got["comm_para"], exp["comm_para"]) and np.array_equal(got["comm_input"], exp["comm_input"])
    assert got["proof"] == exp["proof"]
    return got


@pytest.mark.parametrize("name", S.SMALL_PROOF_CASES)
def test_small_shapes_against_the_live_oracle(ctx, digests, name):
    inst = S.build(name)
    sat = O.is_sat(inst)
    assert sat == (name == "sat_small")
    for seeds in ((SEED_C, SEED_P), SEEDS_2):
        got, exp = ctx.sat_prove(inst, *seeds), O.sat_prove(inst, *seeds)  # every field, as test_gpu_sat.check
        for k in ("comm_para", "comm_input", "rx", "ry", "inst_evals"):
            assert np.array_equal(got[k], exp[k]), k
        assert got["proof"] == exp["proof"] and len(exp["proof"]) > 0
        assert O.sat_verify(inst, got) == (1 if sat else 0)
        res = check_snark(ctx, inst, seeds)
        assert O.snark_verify(inst, res) == (1 if sat else 0)
        assert ctx.snark_verify(inst, res) == bool(sat)
    d = _digest(ctx.snark_prove(inst, SEED_C, SEED_P))
    assert d == {k: digests[name][k] for k in d}


@pytest.mark.parametrize("name", ["tiny_4_one_matrix", "tiny_3_one_matrix"])
def test_smallest_encodings_that_prove(ctx, name):
    """N = 4: the smallest SPARK encoding the library takes"""
    inst = S.build(name)
    assert S.shape_of(inst)[0] == 4
    res = check_snark(ctx, inst, (SEED_C, SEED_P))
    assert O.snark_verify(inst, res) == O.is_sat(inst)


@pytest.mark.parametrize("name", ["tiny_0", "tiny_1", "tiny_2", "tiny_3", "tiny_4"])
def test_fewer_than_three_entries_per_matrix_is_refused(ctx, name):
    """total nnz 0..4 with N = next_pow2(max nnz) < 4.  The sat proof does not depend on N and equals the oracle's.  The SPARK
    encoding is refused with VPIN_ESHAPE (include/vpin_hip.h, vpin_spark_encode): at N = 1 (tiny_0 .. tiny_3) the oracle has
    no proof either -- its product circuit, like the reference's, has no layer for a one-entry table and it faults -- so it is
    not run here; at N = 2 (tiny_4) the oracle proves and the library does not.  The refusal leaves the context working."""
    from vpin_amd import VpinError
    inst = S.build(name)
    n, m = S.shape_of(inst)
    assert n < 4 <= m
    got, exp = ctx.sat_prove(inst, SEED_C, SEED_P), O.sat_prove(inst, SEED_C, SEED_P)
    assert got["proof"] == exp["proof"] and np.array_equal(got["inst_evals"], exp["inst_evals"])
    with pytest.raises(VpinError) as e:
        ctx.spark_encode(inst)
    assert e.value.code == VPIN_ESHAPE
    with pytest.raises(VpinError) as e:
        ctx.snark_prove(inst, SEED_C, SEED_P)
    assert e.value.code == VPIN_ESHAPE
    if n == 2:
        assert len(O.snark_prove(inst, SEED_C, SEED_P)["proof"]) > 0
    check_snark(ctx, S.build("tiny_4_one_matrix"), (SEED_C, SEED_P))


@pytest.mark.parametrize("name", sorted(S.HOT_CASES))
def test_hot_column_search(ctx, digests, name):
    """N = 2^20: no hot column; one exactly at the threshold N / 64, one just below, one candidate absent; both candidates
    above it with another winner per matrix and a tie"""
    inst = S.build(name)
    nv = inst["num_vars"]
    assert S.shape_of(inst)[0] == 1 << 20
    want = [None if w is None else nv + w for w in S.HOT_CASES[name][1]]
    dec, comm = ctx.spark_encode(inst)
    try:
        assert dec.hot_cols() == want
    finally:
        dec.free()
    res = ctx.snark_prove(inst, SEED_C, SEED_P)
    assert res["comm"] == comm
    d = _digest(res)
    assert d == {k: digests[name][k] for k in d}
    assert digests[name]["is_sat"] == 0


# ---- several ranks ------------------------------------------------------------------------------------------------------------

def _prove_ranks(world, inst, new_ctx=None):
    """as test_gpu_dist._prove_threads, from host triplets: -> (single-GPU proof, [proof of rank r]); new_ctx: what makes a rank's context"""
    import vpin_amd
    from vpin_amd import Comm
    ctxs = [(new_ctx or vpin_amd.Context)(0) for _ in range(world)]
    di = ctxs[0].r1cs_upload(inst)
    dec, comm = ctxs[0].spark_encode(inst)
    tabs = [ctxs[0].upload(inst[k]) for k in ("vars_para", "vars_input", "vars")]
    single = ctxs[0].snark_prove_resident(di, dec, *tabs, inst["inputs"], SEED_C, SEED_P)
    single["comm"] = comm
    comms = Comm.local(world)
    out, errs = [None] * world, []

    def body(r):
        try:
            ctxs[r].set_comm(comms[r])
            out[r] = ctxs[r].snark_prove_resident(di, dec, *tabs, inst["inputs"], SEED_C, SEED_P)
            ctxs[r].set_comm(None)
        except BaseException as e:  # noqa: BLE001
            errs.append((r, repr(e)))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(120) for t in ts]
    alive = [t.is_alive() for t in ts]
    for t in tabs:
        t.free()
    dec.free()
    di.free()
    for cm in comms:
        cm.destroy()
    for c in ctxs:
        c.close()
    assert not any(alive) and not errs, (alive, errs)
    return single, out


@pytest.fixture(scope="module")
def ranks_case():
    inst = S.build("ranks")
    return inst, O.snark_prove(inst, SEED_C, SEED_P)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_long_columns_over_several_ranks(ranks_case, digests, world):
    """worlds 2 and 4 split by residue (the strided SpMV, eval table and long-column finish); 3 deals whole circuits"""
    inst, exp = ranks_case
    single, out = _prove_ranks(world, inst)
    assert single["proof"] == exp["proof"] and single["comm"] == exp["comm"]
    assert _digest(single)["proof"] == digests["ranks"]["proof"]
    for r, res in enumerate(out):
        assert res is not None, f"rank {r} returned nothing"
        assert res["proof"] == exp["proof"], f"rank {r}: proof differs from the single-GPU proof"
        assert np.array_equal(res["comm_para"], exp["comm_para"]) and np.array_equal(res["comm_input"], exp["comm_input"])
