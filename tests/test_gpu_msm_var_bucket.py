"""GPU parity of the bucket-method variable-base MSM (vpin_msm_bucket) with the one-lane-per-term kernel (vpin_msm) and with
the oracle's group arithmetic: the compressed results are byte-equal at every size from one point to 2^16, for random
scalars, zero scalars, q - 1, one point repeated n times (it meets itself in every bucket it lands in), P and -P under equal
scalars (they meet in one bucket and cancel), the identity encoding among the inputs, and an encoding that does not decode at
the first, a middle and the last position (VPIN_EVERIFY, as vpin_msm answers)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pymodel as M
import pymodel_group as PG

pytestmark = pytest.mark.gpu
Q = M.Q
SIZES = [1, 2, 63, 64, 65, 1000, 4096, 1 << 15, 1 << 16]
ORACLE_MAX = 65  # the oracle's MSM is a Python loop of scalar multiplications: seconds up to here


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def points():
    """4100 group elements (a generator stream) as oracle points and as compressed encodings; larger lists repeat them"""
    n = 4100
    _, og = O.gens_stream_xyzt(n, b"var-msm-bucket-test")
    L = O.lib()
    enc = np.zeros((n, 32), dtype=np.uint8)
    for i in range(n):
        L.ge_compress(enc[i].ctypes.data_as(C.c_void_p), C.byref(og[i]))
    return og, enc


def oracle_msm(og, ints, idx):
    L = O.lib()
    acc = O.Ge()
    L.ge_identity(C.byref(acc))
    for k, i in zip(ints, idx):
        t = O.Ge()
        L.ge_scalarmul_bytes(C.byref(t), (C.c_uint8 * 32)(*int(k % Q).to_bytes(32, "little")), C.byref(og[i]))
        L.ge_add(C.byref(acc), C.byref(acc), C.byref(t))
    out = (C.c_uint8 * 32)()
    L.ge_compress(out, C.byref(acc))
    return bytes(out)


def rand_scalars(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % Q for _ in range(n)]


def pick(enc, n, shift=0):
    return enc[(np.arange(n) + shift) % enc.shape[0]]


@pytest.mark.parametrize("n", SIZES)
def test_random_scalars_match_msm_and_oracle(ctx, points, n):
    og, enc = points
    ints = rand_scalars(n, n)
    if n >= 8:  # edge values among them
        ints[0:8] = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, 2**128 + 129, 2**252 - 1]
    pts = pick(enc, n, 7)
    s = M.ints_to_table(ints)
    got, xyzt = ctx.msm_bucket(s, pts, want_xyzt=True)
    assert bytes(got) == bytes(ctx.msm(s, pts))
    if n <= ORACLE_MAX:
        assert bytes(got) == oracle_msm(og, ints, [(i + 7) % enc.shape[0] for i in range(n)])
    # X|Y|Z|T is that group element too: canonical coordinates on the curve's extended form, compressing to the same bytes
    X, Y, Z, T = (int.from_bytes(bytes(xyzt[32 * k:32 * k + 32]), "little") for k in range(4))
    assert max(X, Y, Z, T) < PG.P and (X * Y - Z * T) % PG.P == 0
    assert PG.Pt(X, Y, Z, T).encode() == bytes(got)


@pytest.mark.parametrize("n", SIZES)
def test_all_zero_scalars_give_the_identity(ctx, points, n):
    _, enc = points
    assert bytes(ctx.msm_bucket(np.zeros((n, 4), dtype=np.uint64), pick(enc, n))) == bytes(32)


@pytest.mark.parametrize("n", SIZES)
def test_scalar_q_minus_one_everywhere(ctx, points, n):
    """every scalar the same: each window puts all n points into one bucket"""
    og, enc = points
    s = np.tile(M.ints_to_table([Q - 1]), (n, 1))
    pts = pick(enc, n, 3)
    got = ctx.msm_bucket(s, pts)
    assert bytes(got) == bytes(ctx.msm(s, pts))
    if n <= ORACLE_MAX:
        assert bytes(got) == oracle_msm(og, [Q - 1] * n, [(i + 3) % enc.shape[0] for i in range(n)])


@pytest.mark.parametrize("n", SIZES)
def test_one_point_repeated(ctx, points, n):
    """the same point n times: it meets itself wherever two of its digits agree; the sum is (sum of the scalars) * P"""
    og, enc = points
    ints = rand_scalars(n, 1000 + n)
    if n >= 4:
        ints[1] = ints[0]           # equal scalars: a doubling inside a bucket in every window
        ints[3] = (Q - ints[2]) % Q  # opposite scalars: P meets -P
    s = M.ints_to_table(ints)
    pts = np.tile(enc[11], (n, 1))
    got = ctx.msm_bucket(s, pts)
    assert bytes(got) == bytes(ctx.msm(s, pts))
    assert bytes(got) == bytes(ctx.msm(M.ints_to_table([sum(ints) % Q]), enc[11:12]))
    assert bytes(got) == oracle_msm(og, [sum(ints) % Q], [11])


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 2])
def test_p_and_minus_p_cancel(ctx, points, n):
    """a list of P_i and -P_i under equal scalars: every pair shares its buckets and the sum is the identity"""
    _, enc = points
    half = n // 2
    nd = min(half, 64)  # distinct points; -P_i = (q - 1) P_i through the one-lane kernel
    minus_one = M.ints_to_table([Q - 1])
    neg = np.stack([ctx.msm(minus_one, enc[40 + i:41 + i]).copy() for i in range(nd)])
    base, negs = enc[40 + np.arange(half) % nd], neg[np.arange(half) % nd]
    ints = rand_scalars(half, 2000 + n)
    pts = np.concatenate([base, negs])
    s = M.ints_to_table(ints + ints)
    if n % 2:  # odd sizes: one more term with a zero scalar
        pts = np.concatenate([pts, enc[:1]])
        s = np.concatenate([s, np.zeros((1, 4), dtype=np.uint64)])
    assert pts.shape[0] == n
    assert bytes(ctx.msm_bucket(s, pts)) == bytes(32)


@pytest.mark.parametrize("n", SIZES)
def test_identity_encoding_among_the_inputs(ctx, points, n):
    og, enc = points
    ints = [v or 5 for v in rand_scalars(n, 3000 + n)]
    pts = pick(enc, n, 100).copy()
    where = sorted({0, n // 2, n - 1})
    for w in where:
        pts[w] = 0
    s = M.ints_to_table(ints)
    got = ctx.msm_bucket(s, pts)
    assert bytes(got) == bytes(ctx.msm(s, pts))
    if n <= ORACLE_MAX:
        keep = [i for i in range(n) if i not in where]
        assert bytes(got) == oracle_msm(og, [ints[i] for i in keep], [(i + 100) % enc.shape[0] for i in keep])


@pytest.mark.parametrize("n", SIZES)
def test_an_encoding_that_does_not_decode_is_refused(ctx, points, n):
    import vpin_amd
    _, enc = points
    s = M.ints_to_table(rand_scalars(n, 4000 + n))
    bad = np.frombuffer(bytes([0xED] + [0xFF] * 30 + [0x7F]), dtype=np.uint8)  # s = p: not canonical
    g = O.Ge()
    assert not O.lib().ge_decompress(C.byref(g), (C.c_uint8 * 32)(*bytes(bad)))
    for pos in sorted({0, n // 2, n - 1}):
        pts = pick(enc, n, 9).copy()
        pts[pos] = bad
        for call in (ctx.msm_bucket, ctx.msm):
            with pytest.raises(vpin_amd.VpinError) as ei:
                call(s, pts)
            assert ei.value.code == -6, (pos, call.__name__)
    assert bytes(ctx.msm_bucket(s, pick(enc, n, 9))) == bytes(ctx.msm(s, pick(enc, n, 9)))  # and the context is fine afterwards
