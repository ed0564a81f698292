"""Recycled device blocks never reach a result: every scenario below runs on ONE context per poison word whose pool fills each
block it hands out -- its whole size class, fresh or recycled -- with that word (vpin_ctx_set_pool_poison, tests/pool_poison_cases.py),
in an order that alternates large and small shapes, so that a block usually arrives larger than asked for (the pool's "up to twice
the size" rule) and holds another call's bytes behind the poison's.  A kernel that reads a slot before writing it, reads past its
length into the tail of the size class, or relies on a zero-fill that is not there (DESIGN.md 2.5 lists what every allocation
site relies on) changes the bytes of a proof, a commitment, a ciphertext or a decrypted value here.

No expected value comes from the library: the live oracle, the Python models and the committed digests, exactly as in the test
each scenario is borrowed from.  After every scenario the context's poison counters must have moved."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import e2_msm_shared_model as SM
import elgamal_model as EL
import enc_conv_model as EM
import enc_fc_model as FM
import fcs_model as TM
import gadgets_model as GM
import lenet_model as LM
import net_isolate_model as IM
import oracle_lib as O
import pool_poison_cases as PP
import pymodel as M
import r1cs_shapes as S
from test_gpu_enc_conv import assert_lists, point_at, points_of, run_log_layer, to_arrays

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_C = bytes(range(64))
SEED_P = bytes((7 * i + 3) % 256 for i in range(64))
with open(os.path.join(HERE, "golden", "config_digests.json")) as _f:
    GOLD = json.load(_f)["cases"]
BATCH_KEYS = ["A-mult", "3_32-mult", "3_32-add", "A-add"]  # a 2^20 instance first, then the 2^16 ones in its blocks


@pytest.fixture(scope="module", params=PP.WORDS, ids=["word_%#010x" % w for w in PP.WORDS])
def ctx(request):
    c = PP.poisoned_context(request.param)
    c.word = request.param
    yield c
    c.close()


def test_the_switch_fills_whole_size_classes_and_can_be_turned_off(ctx):
    """a table of 2^10 scalars is a 32 KiB class: one block, 32768 bytes; the zero-filled table (the same block again, poisoned and
    then filled by vpin_table_alloc itself) reads back as zeros; with the switch off the counters stand still"""
    b0, n0 = ctx.pool_poison_stats()
    t = ctx.upload(np.zeros((1 << 10, 4), dtype=np.uint64))
    assert ctx.pool_poison_stats() == (b0 + 1, n0 + (1 << 15))
    t.free()
    z = ctx.alloc(1 << 10)
    assert ctx.pool_poison_stats() == (b0 + 2, n0 + (2 << 15)) and not z.read().any()
    z.free()
    ctx.set_pool_poison(ctx.word, False)
    t = ctx.upload(np.ones((1 << 10, 4), dtype=np.uint64))
    t.free()
    assert ctx.pool_poison_stats() == (b0 + 2, n0 + (2 << 15))
    ctx.set_pool_poison(ctx.word)


# ---- whole proofs ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def config_proofs(ctx):
    """CNN A's point multiplications (2^20 constraints), then conv f=3's instances (2^16) in the blocks it left, then CNN A's
    additions: (meta, result) per key of BATCH_KEYS, built and proven on the device"""
    from test_gpu_verify_batch import prove_dev
    from vpin_amd import gadgets as G
    out = {}
    for key in BATCH_KEYS:
        g = GOLD[key]
        inp = G.synthetic_mult_inputs(g["label"]) if g["kind"] == "mult" else G.synthetic_add_inputs(g["label"])
        with PP.filled(ctx):
            out[key] = prove_dev(ctx, g["kind"], inp)
    return out


def test_configuration_sizes_against_the_oracles_digests(ctx, config_proofs):
    for key in BATCH_KEYS:
        g, (_, got) = GOLD[key], config_proofs[key]
        assert hashlib.sha256(got["comm"]).hexdigest() == g["comm_sha256"], key
        assert hashlib.sha256(got["comm_para"].tobytes()).hexdigest() == g["comm_para_sha256"], key
        assert hashlib.sha256(got["comm_input"].tobytes()).hexdigest() == g["comm_input_sha256"], key
        assert len(got["proof"]) == g["snark_len"] and hashlib.sha256(got["proof"]).hexdigest() == g["snark_sha256"], key


def test_snark_from_device_gadgets_and_the_sat_proof_alone(ctx):
    """64 point additions (N = 2^10) and 2 point multiplications with the weights 5 and 2^200 + 77 (as test_gpu_spark): the
    instance from host triplets and the one built on the device give the oracle's bytes; the sat proof alone too"""
    from test_gpu_sat import check as sat_check
    from test_gpu_spark import check as spark_check
    le = lambda vals: np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32)
    ops = GM.synthetic_add_ops(0x5650494E + 5, 64, rz_one_every=3)
    inst = GM.instance_new(GM.build_point_add(ops))
    with PP.filled(ctx):
        exp = spark_check(ctx, inst)  # the oracle's bytes, as asserted there
    assert ctx.snark_verify(inst, exp)
    with PP.filled(ctx):
        d = ctx.gadget_point_add_dev(*[le([o[k] for o in ops]) for k in range(4)], np.array([o[4] for o in ops], np.uint8))
        try:
            got = d.snark_prove(SEED_C, SEED_P)
        finally:
            d.free()
    assert got["proof"] == exp["proof"] and got["comm"] == exp["comm"]
    with PP.filled(ctx):
        sat = sat_check(ctx, inst)
    assert ctx.sat_verify(inst, sat)
    inst = GM.instance_new(GM.build_point_mult(GM.synthetic_mult_ops(0x5650494E + 3, 2, weights=[5, (1 << 200) + 77])))
    with PP.filled(ctx):
        got = spark_check(ctx, inst)
    assert ctx.snark_verify(inst, got)


def test_verification_of_the_batch_accepts_rejects_and_localises(ctx, config_proofs, monkeypatch):
    items = [config_proofs[k] for k in BATCH_KEYS]
    meta, res = items[1]
    b = bytearray(res["proof"])
    b[len(b) // 3] ^= 1
    bad = (meta, dict(res, proof=bytes(b)))
    for bucket_min in (None, "1"):  # the combined sum by the one-lane kernel, then by vpin_msm_bucket
        if bucket_min:
            monkeypatch.setenv("VPIN_VERIFY_BATCH_BUCKET_MIN", bucket_min)
        with PP.filled(ctx):
            assert ctx.snark_verify_batch(items, bytes(range(32))) == [True] * 4
        with PP.filled(ctx):
            assert not ctx.snark_verify(*bad)
            assert ctx.snark_verify_batch([items[0], bad, items[2], items[3]], hashlib.sha256(b"batch").digest()) == [True, False, True, True]
    monkeypatch.delenv("VPIN_VERIFY_BATCH_BUCKET_MIN")


@pytest.mark.parametrize("name", ["sat_small", "wave_patterns_shuffled"])
def test_snark_from_host_triplets_against_the_live_oracle(ctx, name):
    """trace.hip's sort, r1cs.hip's histogram / scatter / scans, spark_find_hot_cols: a satisfied instance and an unsatisfied one
    whose triplets come shuffled"""
    from test_gpu_snark_shapes import check_snark
    inst = S.build(name)
    sat = O.is_sat(inst)
    assert sat == (name == "sat_small")
    with PP.filled(ctx):
        got, exp = ctx.sat_prove(inst, SEED_C, SEED_P), O.sat_prove(inst, SEED_C, SEED_P)
    for k in ("comm_para", "comm_input", "rx", "ry", "inst_evals"):
        assert np.array_equal(got[k], exp[k]), k
    assert got["proof"] == exp["proof"] and len(exp["proof"]) > 0
    with PP.filled(ctx):
        res = check_snark(ctx, inst, (SEED_C, SEED_P))
    assert O.snark_verify(inst, res) == (1 if sat else 0) and ctx.snark_verify(inst, res) == bool(sat)


def test_ranks_instance_over_two_poisoned_ranks(ctx):
    from test_gpu_snark_shapes import _prove_ranks
    inst = S.build("ranks")
    exp = O.snark_prove(inst, SEED_C, SEED_P)
    ranks = PP.Ranks(ctx.word)
    single, out = _prove_ranks(2, inst, new_ctx=ranks)
    assert single["proof"] == exp["proof"] and single["comm"] == exp["comm"]
    for r, res in enumerate(out):
        assert res is not None and res["proof"] == exp["proof"], f"rank {r}"
        assert np.array_equal(res["comm_para"], exp["comm_para"]) and np.array_equal(res["comm_input"], exp["comm_input"])
    assert len(ranks.stats) == 2 and all(blocks > 0 for blocks, _ in ranks.stats)


def test_configuration_sizes_without_the_resident_tail_in_a_child(ctx):
    """VPIN_SPARK_TAIL_PAIRS=0 is read once per process: every round one launch and every layer ended by the collect kernel, on a
    poisoned context of the child's own (the word goes in through the child's code)"""
    keys = ("A-mult", "3_32-mult", "3_32-add")
    code = PP.CHILD % dict(root=os.path.dirname(HERE), word=ctx.word, cases=[(GOLD[k]["label"], GOLD[k]["kind"]) for k in keys])
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VPIN_SPARK_TAIL_PAIRS="0"), capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-len(keys):] == [GOLD[k]["snark_sha256"] for k in keys]


# ---- row commitments ---------------------------------------------------------------------------------------------------------------

def test_strip_pipeline_of_the_derefs_commitment(ctx):
    """test_gpu_msm_strip's list of 300 taken rows (a second workgroup of 44 live lanes) against the row kernel and the oracle"""
    import ctypes as C
    import digit_vectors as D
    import test_gpu_msm_strip as T
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_gens_layout.argtypes = [C.c_void_p, C.c_void_p]
    xyzt, og = O.gens_stream_xyzt(T.NB)
    g = ctx.gens_shared("test_msm_strip", xyzt, 1)
    lay = (C.c_size_t * 6)()
    assert L.vpin_gens_layout(g.h, lay) == 0
    table = (g, og, D.edge_scalars(int(lay[0]), int(lay[1])))
    n = 300
    case = T.base_case(2, hot=(11, 5, None))
    rng = np.random.default_rng(200 + n)
    for r in range(0, 64, 3):
        case.set_hot(0, r, rng.permutation(64)[:1 + r % 8])
    keep = set(int(x) for x in rng.permutation(384)[:n])
    for row in range(384):
        if row not in keep:
            T.sparse(case, rng, row, 20)
    with PP.filled(ctx):
        elig, _ = T.check(ctx, table, case, dict(VPIN_MSM_STRIP=8))
    assert int(elig.sum()) == n


def test_row_table_commitment_around_a_segment(ctx):
    """test_gpu_row_table at c = 5 and 481 columns (one past a segment): one row, and nine rows in three column chunks"""
    import ctypes as C
    import test_gpu_row_table as T
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_gens_row_layout.argtypes = [C.c_void_p, C.c_void_p]
    c, ncols = 5, 481
    xyzt, og = O.gens_stream_xyzt(T.NB[c])
    with T.env(VPIN_ROW_TABLE_C=c):
        g = ctx.gens_shared(f"test_row_table_c{c}", xyzt, 1)
    lay = (C.c_size_t * 4)()
    assert L.vpin_gens_row_layout(g.h, lay) == 0 and list(lay) == [c, T.windows(c), T.NB[c], T.SEG[c]]
    rng = np.random.default_rng(1000 * c + ncols)

    def mix(n):
        k = rng.random(n)
        return [0 if k[i] < 0.3 else int(rng.integers(0, 2)) if k[i] < 0.4 else M.Q - 1 - int(rng.integers(0, 3)) if k[i] < 0.45
                else T.full(rng) for i in range(n)]
    with PP.filled(ctx):
        T.check_commit(ctx, g, og, mix(ncols), 1)
    with PP.filled(ctx):
        T.check_commit(ctx, g, og, mix(9 * ncols), 9, chunks=3)
    with PP.filled(ctx):
        T.check_commit(ctx, g, og, mix(8 * 256), 8, blinds=[T.full(rng) for _ in range(8)], chunks=3)


def test_bucket_method_rows(ctx):
    """test_gpu_msm_pippenger's small rows at the default width: bucket arrays and digit buffers against the oracle"""
    import test_gpu_msm_pippenger as T
    Rs, Ls, c_bits = 32, 8, 0
    xyzt, og = O.gens_stream_xyzt(Rs + 2)
    g = ctx.gens_create(xyzt)
    rng = np.random.default_rng(100 + c_bits)
    vals = T._witness_like(rng, Ls * Rs)
    edges = T._edge_scalars(9)
    vals[:len(edges)] = edges
    Z = M.ints_to_table(vals)
    blinds = M.ints_to_table(T._full_width(rng, Ls))
    dZ = ctx.upload(Z)
    with PP.filled(ctx):
        assert np.array_equal(ctx.hyrax_commit_pippenger(g, dZ, blinds, Rs + 1, c_bits=c_bits), O.hyrax_commit(Z, Ls, blinds, og, Rs + 1))
    zero = np.zeros((Ls, 4), dtype=np.uint64)
    with PP.filled(ctx):
        assert np.array_equal(ctx.hyrax_commit_pippenger(g, dZ, None, 0, Ls=Ls, c_bits=c_bits), O.hyrax_commit(Z, Ls, zero, og, Rs + 1))
    # 512 columns: more than 256 entries behind every sorted index
    Rs, Ls = 512, 4
    xyzt2, og2 = O.gens_stream_xyzt(Rs + 2)
    g2 = ctx.gens_create(xyzt2)
    Z2 = M.ints_to_table(T._full_width(rng, Ls * Rs))
    blinds2 = M.ints_to_table(T._full_width(rng, Ls))
    dZ2 = ctx.upload(Z2)
    with PP.filled(ctx):
        assert np.array_equal(ctx.hyrax_commit_pippenger(g2, dZ2, blinds2, Rs + 1, c_bits=9), O.hyrax_commit(Z2, Ls, blinds2, og2, Rs + 1))
    for h in (dZ, dZ2, g, g2):
        h.free()


@pytest.mark.parametrize("n", [65, 1000])
def test_variable_base_bucket_msm(ctx, n):
    """vpin_msm_bucket (digits, bucket starts, sorted positions, bucket sums) against the oracle's MSM: just past a wave, and 1000
    points so that every sorted index addresses more than 256 entries"""
    import ctypes as C
    import test_gpu_msm_var_bucket as T
    cnt = 1000
    _, og = O.gens_stream_xyzt(cnt, b"var-msm-bucket-test")
    L = O.lib()
    enc = np.zeros((cnt, 32), dtype=np.uint8)
    for i in range(cnt):
        L.ge_compress(enc[i].ctypes.data_as(C.c_void_p), C.byref(og[i]))
    ints = T.rand_scalars(n, n)
    ints[0:8] = [0, 1, 2, M.Q - 1, M.Q - 2, (M.Q - 1) // 2, 2**128 + 129, 2**252 - 1]
    with PP.filled(ctx):
        got = ctx.msm_bucket(M.ints_to_table(ints), enc[:n])
    acc = O.Ge()
    pts = (O.Ge * n)(*[og[i] for i in range(n)])
    L.ge_msm(C.byref(acc), O.ptr(np.ascontiguousarray(M.ints_to_table(ints))), pts, n)
    out = (C.c_uint8 * 32)()
    L.ge_compress(out, C.byref(acc))
    assert bytes(got) == bytes(out)


def test_bullet_reduction_at_its_smallest_fused_and_classic_sizes(ctx):
    import test_gpu_bullet as T
    xyzt, og = O.gens_stream_xyzt(T.NB, b"test bullet gens")
    g = ctx.gens_create(xyzt)
    try:
        for R, case, classic in ((32, "random", 0), (16, "sparse", 1)):
            rng = np.random.default_rng(R * 7 + len(case) + classic)
            a, b = T.vectors(rng, R, case)
            us = [int.from_bytes(rng.bytes(40), "little") % (M.Q - 1) + 1 for _ in range(R.bit_length() - 1)]
            want_rounds, x_hat, a_hat, g_hat = T.model(a, b, [og[i] for i in range(R)], us)
            with PP.filled(ctx):
                cLR, LR, fin, gh = T.device(ctx, g, a, b, us, classic)
            for j, (cL, cR, Lc, Rc) in enumerate(want_rounds):
                assert M.table_to_ints(cLR[j]) == [cL, cR], f"inner products of round {j}"
                assert bytes(LR[j, 0]) == Lc and bytes(LR[j, 1]) == Rc, f"L / R of round {j}"
            assert M.table_to_ints(fin) == [x_hat, a_hat] and gh == g_hat
    finally:
        g.free()


# ---- the encrypted layers against their Python models --------------------------------------------------------------------------------

def check_conv(ctx, P, H, W, f, walk):
    filt = [(5 * k + 1) % 7 for k in range(f * f)]
    before = ctx.rlc_shared_sums()
    with PP.filled(ctx):
        tr, exp = run_log_layer(ctx, 0xABCD + H, P, H, W, filt, f, f, 1, 1, 16)
    assert (ctx.rlc_shared_sums() > before) == walk, "the other RLC path took the layer"
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], EM.log_point)
    ox, oy, oi = tr.output()
    for p in range(P):
        for t in range(0, tr.oh * tr.ow, 7):
            assert point_at(ox[p], oy[p], oi[p], t) == EM.log_point(exp["out"][p][t]), f"output {t} of plane {p}"
    tr.free()


def test_conv_layer_through_the_shared_scalar_walk(ctx):
    """P = 2, 18 x 18: 324 outputs a plane, past a workgroup.  f = 4 gives a plane 17 sums over its r, which is where
    e2_rlc_shared_wins sends a layer to the walk (wins, order, tile_vec, the offsets); f = 3 has 10 sums a plane and stays on
    the one-lane-per-term kernels with a second-launch reduction over two blocks of partials"""
    check_conv(ctx, 2, 18, 18, 4, True)
    check_conv(ctx, 2, 18, 18, 3, False)


def test_fc_layers_past_a_wave(ctx):
    from test_gpu_enc_fc import assert_output, run_log_fc
    from test_gpu_enc_fc_signed import run_log_fcs, signed_matrix
    P, K, N = 2, 65, 3
    with PP.filled(ctx):
        tr, exp = run_log_fc(ctx, 0xFC00 + K, P, K, [[1 + 7 * (k * N + j) for j in range(N)] for k in range(K)], N, 13)
    assert_output(tr, exp["out"], FM.base_point)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], FM.base_point)
    tr.free()
    with PP.filled(ctx):
        tr, exp = run_log_fcs(ctx, 0xF500 + K, P, K, signed_matrix(K, N), N, 13)
    assert_output(tr, exp["out"], FM.base_point)
    assert_lists(tr, exp["mults"], exp["adds"], exp["left"], FM.base_point)
    tr.free()


def test_conv_layer_on_the_one_lane_per_term_kernels(ctx):
    """P = 2, 9 x 8, f = 3: 72 outputs a plane, below the walk's threshold"""
    check_conv(ctx, 2, 9, 8, 3, False)


def test_avgpool_small_and_past_one_workgroup(ctx):
    from test_gpu_enc_fc import assert_output, run_log_pool
    with PP.filled(ctx):
        tr, exp, (x, y) = run_log_pool(ctx, 0x9003, 1, 34, 34, 2, 2, 256)
    assert (tr.oh, tr.ow, tr.n_add) == (17, 17, 867)
    ox, oy, oi = tr.output()
    px, py, rx, ry, rz = tr.adds()
    rng = np.random.default_rng(34)
    for t in [0, 16, 16 * 17, 288] + [int(v) for v in rng.choice(np.arange(1, 288), 40, replace=False)]:
        assert point_at(ox, oy, oi, t) == FM.base_point(exp["out"][0][t]), f"output {t}"
        for m in range(3):
            acc, e = exp["adds"][3 * t + m]
            assert point_at(px, py, None, 3 * t + m) == FM.base_point(acc) and point_at(rx, ry, rz, 3 * t + m) == FM.base_point(e)
    src = np.array([(2 * (t // 17) + m // 2) * 34 + 2 * (t % 17) + m % 2 for t in range(289) for m in (1, 2, 3)])
    assert np.array_equal(rx, x[src]) and np.array_equal(ry, y[src]) and not rz.any()
    tr.free()
    with PP.filled(ctx):
        tr, exp, _ = run_log_pool(ctx, 0x9000 + 25, 2, 5, 5, 2, 2, 256)
    assert_output(tr, exp["out"], FM.base_point)
    assert_lists(tr, [], exp["adds"], [], FM.base_point)
    tr.free()


def test_trained_conv_with_a_bias_under_a_connection_table(ctx):
    from test_gpu_enc_convmc import W_2x2x2, pixels
    from test_gpu_enc_convmc_bias import check_log_layer
    x, y, inf, logs = pixels(0xB1, 4, 4, 4)
    with PP.filled(ctx):
        tr, _ = check_log_layer(ctx, x, y, inf, logs, EM.synthetic_logs(0xB10, 4), 2, 2, 2, 4, 4, W_2x2x2, [[1, 0], [1, 1]], 2)
    tr.free()


def test_mul_chain_past_a_tile(ctx):
    """three unequal-looking chains of K = 257 terms (one past the scan's tile) with identity terms, against the affine model"""
    import test_gpu_mul_chain as T
    D = EM.log_point(0x9E3779B97F4A7C15F39CC0605CEDC835)
    pool, acc = [], None
    for _ in range(700):
        acc = GM.e2_add(acc, D)
        pool.append(acc)
    P, K = 3, 257
    scalars = [(5 * p + 3 * k + k // 7) % 8 for p in range(P) for k in range(K)]
    points = [pool[(211 * p + k) % 700] for p in range(P) for k in range(K)]
    for p in range(P):
        for k in (0, 5, 64, 255, 256):
            if (k + p) % 2 == 0:
                points[p * K + k], scalars[p * K + k] = None, 3
    with PP.filled(ctx):
        T.check(ctx, scalars, points, P, K)


def test_plane_sums_batch(ctx):
    """three groups of four 10 x 10 planes under a table with overlapping rows: 300 lanes an output row, against the model"""
    groups, n_in, H, W = 3, 4, 10, 10
    connect = [[1, 0, 1, 1], [0, 0, 1, 0], [1, 1, 1, 1]]
    logs = [[EM.synthetic_logs(0x100 + 16 * g + j, H * W) for j in range(n_in)] for g in range(groups)]
    x, y, inf = to_arrays(LM.logs_to_points([k for g in logs for p in g for k in p]))
    with PP.filled(ctx):
        ox, oy, oi = ctx.e2_plane_sums_batch(x, y, inf, groups, n_in, H, W, connect)
    for g in range(groups):
        want = LM.logs_to_points([k for p in LM.plane_sums(EM.LOGS, logs[g], connect) for k in p])
        assert points_of(ox[g], oy[g], oi[g]) == want, "group %d" % g


def test_shared_scalar_msm_in_segments_and_in_chunks(ctx):
    """65 + 3 sums over 513 terms (two segments of terms); then 130 + 3 sums under a cap of two tiles, where the per-window
    results of the first chunk are still in the block when the second chunk writes it"""
    import test_gpu_e2_msm_shared as T
    pool = T.make_pool()
    spv, n_terms = 65, 513
    scalars = [T.rand_scalars(spv * 1000 + n_terms, n_terms), T.rand_scalars(spv * 1000 + n_terms + 500, n_terms)]
    sums = [(0, s % 3, s % 40) for s in range(spv)]
    for at, s in ((0, 0), (len(sums) // 2 + 1, 1), (len(sums) + 2, 2)):
        sums.insert(at, (1, s, 11 + s))
    with PP.filled(ctx):
        T.check(ctx, pool, scalars, T.patterns(n_terms), [s[0] for s in sums], [s[1] for s in sums], [s[2] for s in sums])
    n_terms = 3
    ctx.set_rlc_shared_cap(2 * 64 * SM.n_windows(128) * 96)
    try:
        scalars = [T.rand_scalars(31, n_terms), T.rand_scalars(32, n_terms)]
        with PP.filled(ctx):
            T.check(ctx, pool, scalars, T.patterns(n_terms), [0] * 130 + [1] * 3, [s % 3 for s in range(133)], [s % 100 for s in range(133)])
    finally:
        ctx.set_rlc_shared_cap(0)


# ---- the client ----------------------------------------------------------------------------------------------------------------------

SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER


def test_client_tables_encrypt_decrypt_round_and_wire(ctx):
    """the base tables and the baby-step table are built with the poison already on (the table's idx slots must be empty, its
    parity bytes zero); 257 values met at giant steps 0 .. 3; one ReLU + shift-26 round on the pinned inputs; 300 packed points"""
    import test_gpu_client_round as R
    import test_gpu_e2_wire as Wt
    import wire_model as WM
    from vpin_amd import elgamal as E
    with PP.filled(ctx):
        g = E.BaseTable(ctx)
        h = E.BaseTable(ctx, E.keygen(g, SK))
    assert E.keygen(g, SK) == EL.keygen(SK)
    with PP.filled(ctx):
        t = E.DlogTable(ctx, 1000)
    try:
        vs = [(i * 37) % 7999 - 3999 for i in range(257)]
        rs = EL.splitmix_scalars(0x257, 257)
        with PP.filled(ctx):
            c1, c2 = E.encrypt(g, h, vs, rs)
        H = EL.keygen(SK)
        for i in (0, 1, 128, 255, 256):
            m1, m2 = EL.encrypt(H, vs[i], rs[i])
            assert point_at(c1[0], c1[1], c1[2], i) == m1 and point_at(c2[0], c2[1], c2[2], i) == m2
        with PP.filled(ctx):
            v, found = E.decrypt(t, SK, c1, c2, 3)
        assert found.all() and [int(a) for a in v] == vs
        pts = [EL.mul(v) for v in (0, 1, -1, 999, 1000, -1001, 3999, -3999, 4000, -4000)]
        with PP.filled(ctx):
            v, found = t.solve(to_arrays(pts), 3)
        assert [int(f) for f in found] == [1] * 8 + [0, 0] and [int(a) for a in v] == [0, 1, -1, 999, 1000, -1001, 3999, -3999, 0, 0]
    finally:
        t.free()
    with PP.filled(ctx):
        t = E.DlogTable(ctx, R.NB)
    try:
        pins = R.pinned("shifting_26")
        with PP.filled(ctx):
            exp = R.one_round((ctx, g, h, t), [v for v, _ in pins], True, 26)
        assert exp == [r if v > 0 else 0 for v, r in pins]
    finally:
        t.free()
        h.free()
        g.free()
    mult, P = [], None
    for _ in range(64):
        P = GM.e2_add(P, WM.G)
        mult.append(P)
    base = mult + [Wt.neg(p) for p in mult] + [None]
    with PP.filled(ctx):
        Wt.check_round_trip(ctx, [base[(7 * i + 3) % len(base)] for i in range(300)])


# ---- the inference: images that leave a batch ---------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
@pytest.mark.parametrize("refused", [True, False], ids=["middle_image_refused", "nothing_refused"])
def test_isolated_inference_against_the_model(ctx, refused):
    """B = 3 on the two-round network 8 -> 4 -> 2, every context poisoned: the middle image's c1 carries an identity, the first
    layer refuses it and the survivors are compacted into slots that held it; and the same batch with nothing refused.  Every
    image's share of every layer call, the statuses and the clients' values against tests/net_isolate_model.py on logarithms"""
    import test_gpu_net_isolate as T
    from test_net_isolate_model import run_isolated
    from vpin_amd import elgamal as E
    d = IM.two_round_inputs()
    clients = [PP.poisoned_context(ctx.word) for _ in range(3)]
    ctxs = [ctx] + clients
    base_g = E.BaseTable(ctx)
    two = dict(d, cfg=TM.device_config(d["model"], [4, 4]), base_g=base_g, pubs=[E.keygen(base_g, sk) for sk in d["sks"]])
    run = trace = None
    try:
        with PP.filled(*ctxs):
            run = T.InProcess(ctxs, two)
            if refused:
                run.c1 = T.identity_at(run.c1, 8 + 3)
            trace, status = run.run(ctx, "infer_isolated")

        def plant(c1, c2):
            c1[1][3] = 0

        calls, want, seen = run_isolated(d, 3, plant if refused else None)
        assert [s["code"] for s in status] == [0 if w is None else w[0] for w in want] == ([0, T.ESHAPE, 0] if refused else [0, 0, 0])
        assert [(s["layer"], s["round"]) for s, w in zip(status, want) if w is not None] == [w[1:3] for w in want if w is not None]
        assert trace.n_layers == len(calls) == 2
        for i, call in enumerate(calls):
            assert trace.layer_images(i) == call["slots"] == ([0, 2] if refused else [0, 1, 2])
            for b in call["slots"]:
                part = {k: IM.image_part(call, b, k) for k in ("out", "mults", "adds", "left")}
                flat = [v for plane in part["out"] for v in plane] + [m[1] for m in part["mults"]] + \
                    [a[k] for a in part["adds"] for k in (0, 1)] + list(part["left"])
                table = dict(zip(flat, LM.logs_to_points(flat)))
                got = trace.image_layer(b, i)
                assert points_of(*got.output()) == [table[v] for plane in part["out"] for v in plane], "slot %d layer %d: output" % (b, i)
                assert_lists(got, part["mults"], part["adds"], part["left"], table.__getitem__)
        for b in calls[-1]["slots"]:
            got = [([int(a) for a in v], [int(a) for a in act]) for v, act in (run.clients[b].values(r) for r in range(2))]
            assert got == [(list(v), list(a)) for v, a in seen[b]], "slot %d: the client's values" % b
    finally:
        if trace is not None:
            trace.free()
        if run is not None:
            run.free()
        base_g.free()
        for c in clients:
            c.close()
