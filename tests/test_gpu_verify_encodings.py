"""The verifiers on hostile ENCODINGS: vpin_sat_verify, vpin_snark_verify and vpin_snark_verify_batch on proofs in which one
field at a time is replaced by an encoding class a bit flip essentially never lands on -- a point written as s = p, with bit 255
set, as its negative root, as a non-square, as s = p - 1, as 32 zero bytes, as another valid point; a scalar written as v + q;
a length prefix of 0, n - 1, n + 1, 2^63, 2^64 - 1; a proof cut at a field boundary or one byte longer.  Every case is a
well-formed call with bad DATA, which the verifier is specified to refuse: VPIN_EVERIFY, never another code.

Two proofs: one whose witness commitment has 64 rows (every point decoded by the host's Point::decompress) and one with 128
rows (the row commitments decoded by the device's ge_decompress, verify.cpp: `L >= 128`); the second runs once more in a child
process under VPIN_VERIFY_HOST_MSM=1, and the verdicts of the two paths on the same bytes must be identical.  Field positions
come from the schema of tests/bincode_layout.py.

Two tests here are NOT marked gpu: test_the_oracle_rejects_every_point_prefix_and_truncation_case checks on the CPU that the
oracle's verifier rejects every such case (on the oracle's own proofs of the same instances, which the provers reproduce byte
for byte), so no case may be tolerated on the GPU; test_case_lists_name_every_kind_and_class holds the case lists to the schema.  The non-canonical scalars are not asserted on the oracle, which like the
reference deserialises raw limbs; the product must reject them (Reader::scalar)."""
import functools
import json
import os
import pickle
import re
import struct
import subprocess
import sys
from collections import OrderedDict, namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bincode_layout as BL  # noqa: E402
import host_vectors as HV  # noqa: E402
import pymodel_group as PG  # noqa: E402

P, Q = HV.P, HV.Q
SEED_C = bytes(range(64))
SEED_P = bytes((7 * i + 3) % 256 for i in range(64))
SMALL_OPS, LARGE_OPS = 1, 4   # point multiplications: 2^12 variables (64 commitment rows) and 2^14 (128 rows)

# target: which buffer of the call changes (proof, comm, comm_para, comm_input); off / data: bytes replaced; cut: new length of
# the proof (None: unchanged); tail: bytes appended
Case = namedtuple("Case", "name group target off data cut tail")


def leaves(buf, schema, path="", off=0):
    """every scalar ('S'), point ('P') and Vec length ('V') of a bincode value: (path, kind, offset, count); returns the end"""
    kind = schema[0]
    if kind in ("S", "P"):
        yield (path, kind, off, None)
        return off + 32
    if kind == "V":
        (n,) = struct.unpack_from("<Q", buf, off)
        yield (path + ".len", "V", off, n)
        off += 8
        for i in range(n):
            off = yield from leaves(buf, schema[1], f"{path}.{i}", off)
        return off
    if kind == "A":
        for i in range(schema[2]):
            off = yield from leaves(buf, schema[1], f"{path}.{i}", off)
        return off
    for fname, ftype in schema[1]:
        off = yield from leaves(buf, ftype, f"{path}.{fname}" if path else fname, off)
    return off


def kind_of(path):
    return re.sub(r"\.\d+", ".*", path)


def representatives(buf, schema):
    """kind -> one field of that kind (the middle one of its occurrences): {'P': {...}, 'S': {...}, 'V': {...}}"""
    seen = {"P": OrderedDict(), "S": OrderedDict(), "V": OrderedDict()}
    for path, kind, off, n in leaves(buf, schema):
        seen[kind].setdefault(kind_of(path), []).append((path, off, n))
    assert BL.walk(buf, schema).end == len(buf)
    return {k: OrderedDict((name, v[len(v) // 2]) for name, v in d.items()) for k, d in seen.items()}


def _le(x):
    return x.to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def _refused_small():
    cl = HV.decompress_classes()
    return cl["non-square"][0], cl["negative t"][0]


def point_substitutions(cur, other):
    """(name, 32 bytes) for a field that holds the valid encoding cur: the refused classes, then valid encodings of other
    points.  A substitution equal to cur is left out (the identity for a field that is the identity)."""
    s0 = int.from_bytes(cur, "little")
    non_square, negative_t = _refused_small()
    base = int.from_bytes(PG.basepoint().encode(), "little")
    pt = PG.decode(cur)
    assert pt is not None, "the field does not hold a valid encoding"
    subs = [("s = p", P), ("s = p + 2", P + 2), ("s = 2^255 - 1", 2**255 - 1), ("s = p + 1 (even)", P + 1),
            ("bit 255 set", (s0 or base) | 2**255), ("negative root", P - (s0 or base)), ("s = p - 1 (y = 0)", P - 1),
            ("non-square", non_square), ("negative t", negative_t),
            ("32 zero bytes", 0), ("the basepoint", base), ("-P", int.from_bytes((-pt).encode(), "little")),
            ("another field's point", int.from_bytes(other, "little"))]
    for name, s in subs[:9]:
        assert PG.decode(_le(s)) is None, name
    for name, s in subs[9:]:
        assert PG.decode(_le(s)) is not None, name
    return [(name, _le(s)) for name, s in subs if _le(s) != cur]


def scalar_substitutions(cur):
    v = int.from_bytes(cur, "little")
    assert v < Q
    return [("v + q", _le(v + Q)), ("v + 2q", _le(v + 2 * Q)), ("2^256 - 1", _le(2**256 - 1)), ("q", _le(Q))]


def prefix_substitutions(n):
    return [(str(name), struct.pack("<Q", v)) for name, v in (("0", 0), ("n - 1", n - 1), ("n + 1", n + 1), ("2^63", 1 << 63), ("2^64 - 1", (1 << 64) - 1))
            if 0 <= v != n]


def comm_rows(comm):
    """the row commitments of bincode(R1CSCommitment): six u64, Vec of c_ops, Vec of c_mem -> {kind: offset of the middle row}"""
    (n_ops,) = struct.unpack_from("<Q", comm, 48)
    (n_mem,) = struct.unpack_from("<Q", comm, 56 + 32 * n_ops)
    assert 64 + 32 * (n_ops + n_mem) == len(comm)
    return OrderedDict([("comm.c_ops.*", 56 + 32 * (n_ops // 2)), ("comm.c_mem.*", 64 + 32 * n_ops + 32 * (n_mem // 2))])


_CASES = {}


def cases_of(res, schema=BL.SNARK, point_kinds=None, with_comm=True):
    """every case of one proof: (points, scalars, prefixes, cuts).  point_kinds: a filter on the kinds of point (None: all)"""
    key = (res["proof"], res["comm_para"].tobytes(), id(schema), tuple(point_kinds or ()), with_comm)
    if key not in _CASES:
        _CASES[key] = _cases_of(res, schema, point_kinds, with_comm)
    return _CASES[key]


def _cases_of(res, schema, point_kinds, with_comm):
    proof = res["proof"]
    reps = representatives(proof, schema)
    pts = [(k, "proof", off) for k, (_, off, _) in reps["P"].items()]
    if with_comm:
        pts += [(k, "comm", off) for k, off in comm_rows(res["comm"]).items()]
    rows = res["comm_para"].shape[0]
    pts += [("comm_para.*", "comm_para", 32 * (rows // 2 + 1)), ("comm_input.*", "comm_input", 32 * (rows - 1))]
    buf = lambda t: proof if t == "proof" else res["comm"] if t == "comm" else res[t].tobytes()
    points, scalars, prefixes, cuts = [], [], [], []
    for i, (kind, target, off) in enumerate(pts):
        if point_kinds is not None and not any(re.search(p, kind) for p in point_kinds):
            continue
        cur = buf(target)[off:off + 32]
        k2, t2, o2 = pts[(i + 1) % len(pts)]
        other = buf(t2)[o2:o2 + 32]
        if other == cur:
            other = (3 * PG.basepoint()).encode()
        for name, data in point_substitutions(cur, other):
            points.append(Case(f"{kind} <- {name}", kind, target, off, data, None, b""))
    for kind, (_, off, _) in reps["S"].items():
        for name, data in scalar_substitutions(proof[off:off + 32]):
            scalars.append(Case(f"{kind} <- {name}", kind, "proof", off, data, None, b""))
    for kind, (_, off, n) in reps["V"].items():
        for name, data in prefix_substitutions(n):
            prefixes.append(Case(f"{kind} <- {name}", kind, "proof", off, data, None, b""))
    bounds = sorted({off for d in reps.values() for (_, off, _) in d.values()} | {len(proof) - 1, len(proof) - 32})
    cuts = [Case(f"cut at {off}", "cut", "proof", 0, b"", off, b"") for off in bounds]
    cuts.append(Case("one byte longer", "cut", "proof", 0, b"", None, b"\0"))
    return points, scalars, prefixes, cuts


def apply(case, res):
    out = dict(res)
    if case.target == "proof":
        b = bytearray(res["proof"])
        b[case.off:case.off + len(case.data)] = case.data
        if case.cut is not None:
            del b[case.cut:]
        out["proof"] = bytes(b) + case.tail
    elif case.target == "comm":
        b = bytearray(res["comm"])
        b[case.off:case.off + 32] = case.data
        out["comm"] = bytes(b)
    else:
        a = res[case.target].copy()
        a.reshape(-1)[case.off:case.off + 32] = np.frombuffer(case.data, dtype=np.uint8)
        out[case.target] = a
    same = out[case.target] == res[case.target] if isinstance(out[case.target], bytes) else np.array_equal(out[case.target], res[case.target])
    changed = not same
    assert changed, case.name
    return out


# the larger proof's share: the fields the device decodes when there are 128 rows or more (every row commitment), and two kinds
# the host decodes whatever the size
LARGE_POINT_KINDS = [r"comm_vars\.C", r"^comm_para", r"^comm_input", r"comm_derefs", r"^comm\.", r"sc_proof_phase1\.comm_polys",
                     r"proof_eval_vars_at_ry.*L_vec"]


def large_cases(res):
    points, scalars, prefixes, cuts = cases_of(res, point_kinds=LARGE_POINT_KINDS)
    return points + scalars[:8] + prefixes[:10] + cuts[:2] + cuts[-2:]


def model_instance(ops):
    """the synthetic point-multiplication instance of `ops` operations from the Python gadget model (no GPU, no product code
    but the input generator)"""
    import gadgets_model as GM
    from vpin_amd import gadgets as G
    inp = G.synthetic_mult_inputs("3_32", ops)
    ints = lambda a: [int.from_bytes(bytes(r), "little") for r in a]
    return GM.instance_new(GM.build_point_mult(list(zip([int(v) for v in inp[0]], ints(inp[1]), ints(inp[2])))))


# ---- the oracle's part (CPU) ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_proofs():
    import oracle_lib as O
    out = {}
    for name, ops in (("small", SMALL_OPS), ("large", LARGE_OPS)):
        inst = model_instance(ops)
        res = O.snark_prove(inst, SEED_C, SEED_P)
        assert O.snark_verify(inst, res) == 1
        out[name] = (inst, res)
    assert out["small"][1]["comm_para"].shape[0] == 64 and out["large"][1]["comm_para"].shape[0] == 128
    return out


def test_case_lists_name_every_kind_and_class(oracle_proofs):
    """from the proof's bytes and the schema alone: every kind of point, scalar and prefix is there with every substitution"""
    inst, res = oracle_proofs["small"]
    points, scalars, prefixes, cuts = cases_of(res)
    kinds = {c.group for c in points}
    for want in ("r1cs_sat_proof.comm_vars.C.*", "comm_para.*", "comm_input.*", "comm.c_ops.*", "comm.c_mem.*",
                 "r1cs_sat_proof.sc_proof_phase1.comm_polys.*", "r1cs_sat_proof.sc_proof_phase1.comm_evals.*",
                 "r1cs_sat_proof.sc_proof_phase2.comm_polys.*", "r1cs_sat_proof.sc_proof_phase2.comm_evals.*",
                 "r1cs_sat_proof.sc_proof_phase1.proofs.*.delta", "r1cs_sat_proof.sc_proof_phase2.proofs.*.beta",
                 "r1cs_sat_proof.claims_phase2.*", "r1cs_sat_proof.pok_claims_phase2.knowledge.alpha",
                 "r1cs_sat_proof.pok_claims_phase2.product.alpha", "r1cs_sat_proof.pok_claims_phase2.product.beta",
                 "r1cs_sat_proof.pok_claims_phase2.product.delta", "r1cs_sat_proof.proof_eq_sc_phase1.alpha",
                 "r1cs_sat_proof.proof_eq_sc_phase2.alpha", "r1cs_sat_proof.comm_vars_at_ry",
                 "r1cs_sat_proof.proof_eval_vars_at_ry.proof.bullet_reduction_proof.L_vec.*",
                 "r1cs_sat_proof.proof_eval_vars_at_ry.proof.bullet_reduction_proof.R_vec.*",
                 "r1cs_sat_proof.proof_eval_vars_at_ry.proof.delta", "r1cs_sat_proof.proof_eval_vars_at_ry.proof.beta",
                 "r1cs_eval_proof.proof.comm_derefs.comm_ops_val.C.*"):
        assert want in kinds, want
    hash_layer = "r1cs_eval_proof.proof.poly_eval_network_proof.proof_hash_layer."
    for pe in ("proof_ops.proof", "proof_mem.proof", "proof_derefs.proof_derefs.proof"):
        for f in ("bullet_reduction_proof.L_vec.*", "bullet_reduction_proof.R_vec.*", "delta", "beta"):
            assert hash_layer + pe + "." + f in kinds
    # every kind of point in the schema, by the schema itself
    assert kinds == {kind_of(p) for p, k, _, _ in leaves(res["proof"], BL.SNARK) if k == "P"} | {"comm_para.*", "comm_input.*", "comm.c_ops.*", "comm.c_mem.*"}
    names = lambda cs, g: {c.name.split(" <- ")[1] for c in cs if c.group == g}
    for g in kinds:
        got = names(points, g)
        assert {"s = p", "s = p + 2", "s = 2^255 - 1", "bit 255 set", "negative root", "s = p - 1 (y = 0)", "non-square", "negative t",
                "the basepoint", "-P", "another field's point"} <= got, (g, got)
        cur = next(c for c in points if c.group == g)
        assert "32 zero bytes" in got or (res["proof"] if cur.target == "proof" else b"")[cur.off:cur.off + 32] == bytes(32), g
    assert {c.group for c in scalars} == {kind_of(p) for p, k, _, _ in leaves(res["proof"], BL.SNARK) if k == "S"}
    assert all(names(scalars, g) == {"v + q", "v + 2q", "2^256 - 1", "q"} for g in {c.group for c in scalars})
    assert {c.group for c in prefixes} == {kind_of(p) for p, k, _, _ in leaves(res["proof"], BL.SNARK) if k == "V"}
    assert all({"n + 1", "2^63", "2^64 - 1"} <= names(prefixes, g) for g in {c.group for c in prefixes})
    assert any(c.tail for c in cuts) and len(cuts) > 50
    # the larger proof: its row commitments are the device's to decode
    inst, res = oracle_proofs["large"]
    lk = {c.group for c in large_cases(res)}
    assert {"r1cs_sat_proof.comm_vars.C.*", "comm_para.*", "comm_input.*", "comm.c_ops.*", "comm.c_mem.*",
            "r1cs_eval_proof.proof.comm_derefs.comm_ops_val.C.*"} <= lk
    assert len(BL.walk(res["proof"], BL.SNARK)["r1cs_eval_proof"]) > 0


@pytest.mark.parametrize("which", ["small: points of the sat proof", "small: points of the evaluation proof and the commitments",
                                   "small: prefixes", "small: cuts", "large"])
def test_the_oracle_rejects_every_point_prefix_and_truncation_case(oracle_proofs, which):
    """not gpu: every case the GPU tests use is one the oracle's verifier rejects -- none, not 'nearly all'"""
    import oracle_lib as O
    inst, res = oracle_proofs["large" if which == "large" else "small"]
    if which == "large":
        todo = [c for c in large_cases(res) if " <- v + " not in c.name and not c.name.endswith(("<- q", "<- 2^256 - 1"))]
    else:
        points, _, prefixes, cuts = cases_of(res)
        sat = [c for c in points if c.group.startswith("r1cs_sat_proof")]
        todo = {"points of the sat proof": sat, "points of the evaluation proof and the commitments": [c for c in points if c not in sat],
                "prefixes": prefixes, "cuts": cuts}[which.split(": ")[1]]
    assert todo
    # the oracle's verifier keeps no state between calls (two arrays of timings apart) and ctypes releases the GIL
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        verdicts = list(pool.map(lambda c: O.snark_verify(inst, apply(c, res)), todo))
    accepted = [c.name for c, v in zip(todo, verdicts) if v != 0]
    assert not accepted, accepted
    assert O.snark_verify(inst, res) == 1


# ---- the product (GPU) ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def _prove(ctx, inst):
    d = inst.as_dict()
    inst.free()
    res = ctx.snark_prove(d, SEED_C, SEED_P)
    meta = {"inputs": d["inputs"], "num_inputs": d["num_inputs"], "num_cons": d["num_cons"], "num_vars": d["num_vars"]}
    sat = ctx.sat_prove(d, SEED_C, SEED_P)
    return meta, res, sat


@pytest.fixture(scope="module")
def proofs(ctx):
    from vpin_amd import gadgets as G
    out = {"small": _prove(ctx, G.synthetic_mult_instance("3_32", SMALL_OPS)), "large": _prove(ctx, G.synthetic_mult_instance("3_32", LARGE_OPS)),
           "other": _prove(ctx, G.synthetic_add_instance("3_32", 4))}
    assert out["small"][1]["comm_para"].shape[0] == 64 and out["large"][1]["comm_para"].shape[0] == 128
    for meta, res, sat in out.values():
        assert ctx.snark_verify(meta, res) and ctx.sat_verify(meta, sat)
    return out


def _one_per_kind(cases):
    """one case of every kind, the substitutions taken in turn, so that every kind and every substitution is met"""
    by = OrderedDict()
    for c in cases:
        by.setdefault(c.group, []).append(c)
    return [v[i % len(v)] for i, v in enumerate(by.values())]


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["points", "scalars", "prefixes", "cuts"])
def test_snark_verify_rejects_every_case(ctx, proofs, part):
    meta, res, _ = proofs["small"]
    cases = dict(zip(("points", "scalars", "prefixes", "cuts"), cases_of(res)))[part]
    accepted = [c.name for c in cases if ctx.snark_verify(meta, apply(c, res))]   # any code but VPIN_EVERIFY raises
    print(f"{part}: {len(cases)} cases")
    assert not accepted, accepted
    assert ctx.snark_verify(meta, res), "the context verifies an honest proof afterwards"


@pytest.mark.gpu
def test_sat_verify_rejects_every_case(ctx, proofs):
    meta, _, sat = proofs["small"]
    points, scalars, prefixes, cuts = cases_of(sat, schema=BL.R1CSProof, with_comm=False)
    cases = points + scalars + prefixes + cuts[::8] + cuts[-1:]
    accepted = [c.name for c in cases if ctx.sat_verify(meta, apply(c, sat))]
    print(f"{len(cases)} cases")
    assert not accepted, accepted
    assert ctx.sat_verify(meta, sat)


@pytest.mark.gpu
def test_batch_verifier_points_at_the_victim(ctx, proofs):
    """one case of every kind of field (each substitution in turn) in a batch of three: the victim alone is marked"""
    meta, res, _ = proofs["small"]
    honest = [proofs["other"][:2], proofs["large"][:2]]
    points, scalars, prefixes, cuts = cases_of(res)
    cases = _one_per_kind(points) + _one_per_kind(scalars) + _one_per_kind(prefixes) + cuts[::16] + cuts[-1:]
    wrong = []
    for k, c in enumerate(cases):
        items = [honest[0], (meta, apply(c, res)), honest[1]]
        got = ctx.snark_verify_batch(items, bytes([k % 256]) * 32)
        if got != [True, False, True]:
            wrong.append((c.name, got))
    print(f"{len(cases)} cases")
    assert not wrong, wrong
    assert ctx.snark_verify_batch([honest[0], (meta, res), honest[1]], bytes(32)) == [True, True, True]


@pytest.mark.gpu
def test_device_path_and_host_path_give_the_same_verdicts(ctx, proofs, tmp_path):
    """the proof with 128 rows: every case through this process (row commitments decoded on the device) and once more through a
    child process under VPIN_VERIFY_HOST_MSM=1 (the switch is read once per process): the same verdict on every case, all
    rejections, and the device path was indeed the one taken here"""
    meta, res, _ = proofs["large"]
    assert "VPIN_VERIFY_HOST_MSM" not in os.environ, "this process must verify on the device path"
    cases = large_cases(res)
    here = [bool(ctx.snark_verify(meta, apply(c, res))) for c in cases]
    assert not any(here), [c.name for c, v in zip(cases, here) if v]
    assert ctx.snark_verify(meta, res)
    job = tmp_path / "job.pkl"
    with open(job, "wb") as f:
        pickle.dump((meta, res, [tuple(c) for c in cases]), f)
    env = dict(os.environ, VPIN_VERIFY_HOST_MSM="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(job)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    child = json.loads(p.stdout.decode().strip().split("\n")[-1])
    assert child["honest"] is True and child["host_only"] is True
    assert child["verdicts"] == here, [c.name for c, a, b in zip(cases, here, child["verdicts"]) if a != b]
    print(f"{len(cases)} cases, identical verdicts")


def _child(job):
    """VPIN_VERIFY_HOST_MSM=1: the same cases with every point decoded by the host"""
    import vpin_amd
    with open(job, "rb") as f:
        meta, res, cases = pickle.load(f)
    with vpin_amd.Context(0) as c:
        verdicts = [bool(c.snark_verify(meta, apply(Case(*t), res))) for t in cases]
        honest = bool(c.snark_verify(meta, res))
    print(json.dumps({"verdicts": verdicts, "honest": honest, "host_only": "VPIN_VERIFY_HOST_MSM" in os.environ}))


if __name__ == "__main__":
    _child(sys.argv[1])
