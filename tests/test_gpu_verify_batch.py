"""Batch verification (vpin_snark_verify_batch): every deferrable group equation of several SNARKs in one random linear
combination.  Accepts what vpin_snark_verify accepts whatever the seed; a batch with tampered proofs, a tampered commitment,
witness commitment or input, or an unsatisfied witness comes back VPIN_EVERIFY with exactly those proofs marked; proofs of
different shapes (different generator tables) share a batch.

One test here is NOT marked gpu although the file is named test_gpu_*: test_tamper_offsets_are_rejected_by_the_oracle_verifier
checks on the CPU, with the oracle alone, that the 19 tamper cases the GPU test uses are cases a verifier rejects.  It runs in
the "not gpu" suite (one test more there)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_config_variants as MV  # noqa: E402  (the definition of the variant inputs; nothing of it runs the oracle here)

SEED_C = bytes(range(64))
SEED_P = bytes((7 * i + 3) % 256 for i in range(64))
KEYS = ["3_32-mult", "3_32-add", "A-mult", "A-add"]  # conv f=3 and CNN A
VICTIM = 0                                             # the proof the tamper cases change: conv f=3's point multiplications
SEEDS = [bytes(32), bytes(range(32)), hashlib.sha256(b"batch").digest(), None]

with open(os.path.join(HERE, "golden", "config_digests.json")) as _f:
    GOLD = json.load(_f)["cases"]
with open(os.path.join(HERE, "golden", "config_variants.json")) as _f:
    VARIANTS = json.load(_f)["cases"]


def proof_offsets(n):
    """16 offsets spread evenly over a proof of n bytes, from 0 to n - 1"""
    return [round(i * (n - 1) / 15) for i in range(16)]


def tamper_cases(meta, res):
    """the 19 (name, meta, res) cases: one byte of the proof at each of 16 offsets, one byte of comm, comm_para and inputs"""
    out = []
    for off in proof_offsets(len(res["proof"])):
        b = bytearray(res["proof"])
        b[off] ^= 1
        out.append((f"proof[{off}]", meta, dict(res, proof=bytes(b))))
    b = bytearray(res["comm"])
    b[len(b) // 2] ^= 1
    out.append((f"comm[{len(b) // 2}]", meta, dict(res, comm=bytes(b))))
    cp = res["comm_para"].copy()
    cp[cp.shape[0] // 2, 3] ^= 4
    out.append(("comm_para", meta, dict(res, comm_para=cp)))
    inp = np.ascontiguousarray(meta["inputs"], dtype=np.uint64).copy()
    inp.reshape(-1).view(np.uint8)[8] ^= 1
    out.append(("inputs", dict(meta, inputs=inp), res))
    assert len(out) == 19
    return out


def test_tamper_offsets_are_rejected_by_the_oracle_verifier():
    """not gpu: the oracle's verifier on the oracle's own conv f=3 proof rejects the tamper cases the GPU test uses (at most 2
    of the 19 may be accepted: a byte no check reads)"""
    import gadgets_model as GM
    from vpin_amd import gadgets as G
    inp = G.synthetic_mult_inputs("3_32")
    ints = lambda a: [int.from_bytes(bytes(r), "little") for r in a]
    inst = GM.instance_new(GM.build_point_mult(list(zip([int(v) for v in inp[0]], ints(inp[1]), ints(inp[2])))))
    res = O.snark_prove(inst, SEED_C, SEED_P)
    assert hashlib.sha256(res["proof"]).hexdigest() == GOLD["3_32-mult"]["snark_sha256"]
    meta = {"inputs": inst["inputs"], "num_inputs": inst["num_inputs"]}
    assert O.snark_verify(meta, res) == 1
    accepted = [name for name, m, r in tamper_cases(meta, res) if O.snark_verify(m, r) != 0]
    print("accepted by the oracle's verifier:", accepted)
    assert len(accepted) <= 2, accepted


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def prove_dev(ctx, kind, inp, seed_c=SEED_C, seed_p=SEED_P):
    d = ctx.gadget_point_mult_dev(*inp) if kind == "mult" else ctx.gadget_point_add_dev(*inp)
    try:
        got = d.snark_prove(seed_c, seed_p)
        meta = {"inputs": np.array(d.inputs, copy=True), "num_inputs": d.num_inputs}
    finally:
        d.free()
    return meta, got


@pytest.fixture(scope="module")
def batch(ctx):
    """conv f=3 (mult, add) and CNN A (mult, add) under the seeds of tests/golden/config_digests.json"""
    from vpin_amd import gadgets as G
    items = []
    for key in KEYS:
        g = GOLD[key]
        inp = G.synthetic_mult_inputs(g["label"]) if g["kind"] == "mult" else G.synthetic_add_inputs(g["label"])
        meta, got = prove_dev(ctx, g["kind"], inp)
        assert hashlib.sha256(got["proof"]).hexdigest() == g["snark_sha256"], key
        assert hashlib.sha256(got["comm"]).hexdigest() == g["comm_sha256"], key
        items.append((meta, got))
    return items


@pytest.mark.gpu
def test_batch_accepts_under_every_seed(ctx, batch):
    import vpin_amd
    for seed in SEEDS:
        assert ctx.snark_verify_batch(batch, seed) == [True] * 4, seed
    # the C return code itself: VPIN_OK
    assert ctx.snark_verify_batch(batch[:2], SEEDS[1]) == [True, True]
    assert vpin_amd.lib().vpin_snark_verify_batch(ctx.h, None, 0, None, None) == 0  # n = 0
    assert ctx.snark_verify_batch([], None) == []
    for item in batch:  # n = 1 is snark_verify's verdict
        assert ctx.snark_verify_batch([item], SEEDS[2]) == [ctx.snark_verify(*item)] == [True]


@pytest.mark.gpu
def test_every_tamper_case_is_rejected_and_localised(ctx, batch):
    """one byte of one proof (16 offsets), of its comm, comm_para and inputs: the single verifier rejects, the batch returns
    VPIN_EVERIFY with that index alone marked; a case the single verifier accepts (at most 2 of the 19) is named and the batch
    must agree with it"""
    meta, res = batch[VICTIM]
    not_rejected, wrong = [], []
    for k, (name, m, r) in enumerate(tamper_cases(meta, res)):
        single = ctx.snark_verify(m, r)
        items = list(batch)
        items[VICTIM] = (m, r)
        got = ctx.snark_verify_batch(items, SEEDS[k % 3])
        want = [True] * 4
        want[VICTIM] = bool(single)
        print(f"{name}: single verifier {'accepts' if single else 'rejects'}, batch {got}")
        if single:
            not_rejected.append(name)
        if got != want:
            wrong.append((name, got, want))
        if not single:  # the verdict of n = 1 as well
            assert ctx.snark_verify_batch([(m, r)], SEEDS[k % 3]) == [False], name
    assert not wrong, wrong
    assert len(not_rejected) <= 2, not_rejected
    assert ctx.snark_verify_batch(batch, SEEDS[0]) == [True] * 4  # the context is fine afterwards


@pytest.mark.gpu
def test_two_bad_proofs(ctx, batch):
    def flipped(item, frac):
        m, r = item
        b = bytearray(r["proof"])
        b[int(len(b) * frac)] ^= 1
        assert not ctx.snark_verify(m, dict(r, proof=bytes(b)))
        return m, dict(r, proof=bytes(b))
    # two different proofs: one broken in its sat part (a sigma-protocol response), one in its evaluation proofs
    items = list(batch)
    items[1] = flipped(batch[1], 0.3)
    items[2] = flipped(batch[2], 0.95)
    for seed in SEEDS:
        assert ctx.snark_verify_batch(items, seed) == [True, False, False, True]
    # the same tampered proof twice (their equations must not cancel each other)
    bad = flipped(batch[0], 0.97)
    items = [batch[0], bad, batch[1], bad]
    for seed in SEEDS:
        assert ctx.snark_verify_batch(items, seed) == [True, False, True, False]
    # every proof bad
    assert ctx.snark_verify_batch([bad, bad], SEEDS[1]) == [False, False]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["3_32-mult#yzero", "3_32-add#RequalsP"])
def test_unsatisfied_witness_is_the_only_reject(ctx, batch, name):
    g = VARIANTS[name]
    assert g["oracle_is_sat"] == 0
    kind, inp, _ = MV.variant_inputs(name)
    meta, got = prove_dev(ctx, kind, inp, bytes.fromhex(g["seed_commit_hex"]), bytes.fromhex(g["seed_proof_hex"]))
    assert hashlib.sha256(got["proof"]).hexdigest() == g["snark_sha256"]
    oracle = O.snark_verify(meta, got)
    assert oracle == g["oracle_verifier_accepts"] == 0
    items = [batch[1], (meta, got), batch[0]]
    for seed in SEEDS:
        assert ctx.snark_verify_batch(items, seed) == [True, bool(oracle), True]


@pytest.mark.gpu
def test_mixed_shapes_share_a_batch(ctx, batch):
    """a 2^16-constraint point-mult instance and conv f=3's additions: different generator tables, one combined equation"""
    from vpin_amd import gadgets as G
    inst = G.synthetic_mult_instance("3_32", 18)
    d = inst.as_dict()
    inst.free()
    assert d["num_cons"] == 1 << 16
    res = ctx.snark_prove(d, SEED_C, SEED_P)
    big = ({"inputs": d["inputs"], "num_inputs": d["num_inputs"]}, res)
    assert ctx.snark_verify(*big)
    for seed in SEEDS:
        assert ctx.snark_verify_batch([big, batch[1]], seed) == [True, True]
    cp = res["comm_para"].copy()
    cp[5, 3] ^= 4
    assert ctx.snark_verify_batch([batch[1], (big[0], dict(res, comm_para=cp)), big], SEEDS[1]) == [True, False, True]


@pytest.mark.gpu
def test_batch_through_the_bucket_kernel(ctx, batch, monkeypatch):
    """VPIN_VERIFY_BATCH_BUCKET_MIN (read per call) sends the combined sum to vpin_msm_bucket from that many terms on; the default
    is never (profiles/r07_ab_msm_var_bucket.txt).  Same verdicts through it: accept, reject and localise."""
    monkeypatch.setenv("VPIN_VERIFY_BATCH_BUCKET_MIN", "1")
    assert ctx.snark_verify_batch(batch, SEEDS[1]) == [True] * 4
    m, r = batch[2]
    b = bytearray(r["proof"])
    b[int(len(b) * 0.3)] ^= 1
    bad = (m, dict(r, proof=bytes(b)))
    assert not ctx.snark_verify(*bad)
    assert ctx.snark_verify_batch([batch[0], bad, batch[3], bad], SEEDS[2]) == [True, False, True, False]
    monkeypatch.delenv("VPIN_VERIFY_BATCH_BUCKET_MIN")
    assert ctx.snark_verify_batch(batch, SEEDS[1]) == [True] * 4
