"""Writes tests/golden/r1cs_shape_digests.json: the CPU oracle's SNARK for the structural instances of tests/r1cs_shapes.py,
as sha256 digests (the same arrangement as fuzz_mid_digests.json: the N = 2^20 cases cost the oracle minutes, a GPU test
cannot run it live).

    python tests/golden/make_r1cs_shape_digests.py            every case (the N = 2^20 ones take minutes each)
    python tests/golden/make_r1cs_shape_digests.py NAME ...   these cases only, merged into the existing file

Every case is rebuilt from its name alone through r1cs_shapes.build.  tests/test_r1cs_shapes.py regenerates the small
entries and compares the rendered file byte for byte; with VPIN_SHAPE_DIGESTS_FULL=1 it regenerates the large ones too.
The file holds case names, hashes and the measured oracle time: nothing of the instances or the proofs themselves.
"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import oracle_lib as O  # noqa: E402
import r1cs_shapes as S  # noqa: E402

OUT = os.path.join(HERE, "r1cs_shape_digests.json")
SEED_C = bytes(range(64))
SEED_P = bytes((7 * i + 3) % 256 for i in range(64))

SMALL = S.SMALL_PROOF_CASES + ("ranks", "tiny_4", "tiny_4_one_matrix", "tiny_3_one_matrix")
LARGE = tuple(S.HOT_CASES)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def entry(name, threads=None):
    """-> (digests of the oracle's SNARK for the case, seconds the oracle took)"""
    inst = S.build(name)
    t0 = time.time()
    res = O.snark_prove(inst, SEED_C, SEED_P, threads=threads or int(os.environ.get("VPIN_ORACLE_THREADS", os.cpu_count() or 1)))
    dt = time.time() - t0
    n, m = S.shape_of(inst)
    return dict(N=n, M=m, is_sat=int(O.is_sat(inst)), proof_len=len(res["proof"]), proof=_sha(res["proof"]), comm=_sha(res["comm"]),
                comm_para=_sha(np.ascontiguousarray(res["comm_para"]).tobytes()),
                comm_input=_sha(np.ascontiguousarray(res["comm_input"]).tobytes())), dt


def render(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


def source_line(secs):
    t = ", ".join(f"{k} {secs[k]:.0f} s" for k in LARGE if k in secs)
    return ("oracle/ (CPU) SNARK::encode + prove of r1cs_shapes.build(name), seeds of test_gpu_sat.py; written by "
            "tests/golden/make_r1cs_shape_digests.py; oracle time per N = 2^20 case on %d cores: %s" % (os.cpu_count() or 1, t))


def main(names):
    doc = {}
    if names and os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    secs = {}
    for name in names or SMALL + LARGE:
        doc[name], secs[name] = entry(name)
        print(f"{name}: {secs[name]:.1f} s", flush=True)
    if any(k in secs for k in LARGE) or "_source" not in doc:
        doc["_source"] = source_line(secs)
    with open(OUT, "w") as f:
        f.write(render(doc))


if __name__ == "__main__":
    main(sys.argv[1:])
