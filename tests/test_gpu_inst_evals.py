"""inst_evals of a whole SNARK on one GPU come from the SPARK prover's derefs pass (spark.cpp spark_inst_evals: the sum of each
matrix's two dot-product halves over the gathered E_rx[row] * E_ry[col] * val) and no longer from vpin_r1cs_evaluate.  The 96
bytes the SNARK carries behind its sat proof must be what vpin_r1cs_evaluate gives at the proof's (rx, ry) -- the sat-only
entry point still takes that path and returns (rx, ry) -- and what the CPU oracle gives; the proofs keep their digests.

Instances: two gadget instances of the benchmark's families, a structural instance whose matrices have 1000, 513 and 600
entries (N = M = 1024: padding entries in every matrix), and the N = 2^20 instance with a hot column in every matrix (its
derefs commitment takes the hot-column kernel, which reads the same eq(ry, .) table)."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import r1cs_shapes as S
from test_gpu_cumask import GOLD, SEED_C, SEED_P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shape_digests(golden_dir):
    with open(os.path.join(golden_dir, "r1cs_shape_digests.json")) as f:
        return json.load(f)


def _gadget(key):
    from vpin_amd import gadgets as G
    g = GOLD[key]
    inst = G.synthetic_mult_instance(g["label"]) if g["kind"] == "mult" else G.synthetic_add_instance(g["label"])
    return inst.as_dict(), inst


def check(ctx, inst, want_sha):
    sat = ctx.sat_prove(inst, SEED_C, SEED_P)            # vpin_r1cs_evaluate's path; returns rx, ry
    osat = O.sat_prove(inst, SEED_C, SEED_P)
    assert sat["proof"] == osat["proof"]
    assert np.array_equal(sat["inst_evals"], osat["inst_evals"])
    snark = ctx.snark_prove(inst, SEED_C, SEED_P)        # the fused path
    n = len(sat["proof"])
    assert snark["proof"][:n] == sat["proof"], "the sat half of the SNARK is the sat proof"
    ie = snark["proof"][n:n + 96]
    assert ie == np.ascontiguousarray(osat["inst_evals"]).tobytes(), "inst_evals differ from the oracle's"
    assert ie == np.ascontiguousarray(sat["inst_evals"]).tobytes()
    di = ctx.r1cs_upload(inst)
    erx, ery = ctx.eq_table(sat["rx"]), ctx.eq_table(sat["ry"])
    try:
        assert ie == ctx.r1cs_evaluate(di, erx, ery).tobytes(), "inst_evals differ from vpin_r1cs_evaluate at the proof's (rx, ry)"
    finally:
        erx.free()
        ery.free()
        di.free()
    assert hashlib.sha256(snark["proof"]).hexdigest() == want_sha


@pytest.mark.parametrize("key", ["3_32-mult", "A-add"])
def test_gadget_instances(ctx, key):
    d, inst = _gadget(key)
    try:
        check(ctx, d, GOLD[key]["snark_sha256"])
    finally:
        inst.free()


@pytest.mark.parametrize("name", ["proof_n_eq_m", "hot_both"])
def test_structural_instances(ctx, shape_digests, name):
    inst = S.build(name)
    if name == "hot_both":
        dec, _ = ctx.spark_encode(inst)
        try:
            assert all(h is not None for h in dec.hot_cols())
        finally:
            dec.free()
    check(ctx, inst, shape_digests[name]["proof"])
