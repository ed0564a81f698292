"""GPU parity of vpin_e2_msm_shared (the shared-scalar bucket walk of e2_msm_shared.hip) with tests/e2_msm_shared_model.py on
discrete logarithms: the points are k_p * G from vpin_synthetic_points, the expected sums are logarithms mod the order, and
every expected point comes from one batched conversion (lenet_model.logs_to_points).  The shapes are the smallest at which the
walk can go wrong: 1, 63, 64 and 65 sums of a vector (a lane, a wave less one, a wave, a wave and a lane), two vectors of unequal
size in one call with their sums interleaved, 1, 2 and 100 terms, and 513 and 800 (segments of terms); the scalars at every window edge; the cases of the complete
addition inside a bucket; the chunking; the rejections.  vpin_ctx_rlc_shared_sums shows that the walk took the sums."""
import ctypes

import numpy as np
import pytest

import e2_msm_shared_model as SM
import enc_conv_model as EM
import gadgets_model as GM
import lenet_model as LM

pytestmark = pytest.mark.gpu

Q = GM.Q
N_POINTS = 160


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def make_pool():
    """N_POINTS synthetic points and their logarithms; point 5 repeats point 4, point 7 is -point 6, points 9 and 20 are flagged"""
    from vpin_amd import gadgets as G
    x, y = G.synthetic_points(0x5348, N_POINTS)
    x, y = x.reshape(-1, 32).copy(), y.reshape(-1, 32).copy()
    logs = EM.synthetic_logs(0x5348, N_POINTS)
    inf = np.zeros(N_POINTS, np.uint8)
    x[5], y[5], logs[5] = x[4], y[4], logs[4]
    x[7], logs[7] = x[6], (-logs[6]) % EM.ORDER
    y[7] = np.frombuffer((Q - int.from_bytes(bytes(y[6]), "little")).to_bytes(32, "little"), np.uint8)
    for i in (9, 20):
        inf[i], logs[i] = 1, 0
    return x, y, inf, logs


@pytest.fixture(scope="module")
def pool():
    return make_pool()


def rand_scalars(seed, n, bits=128):
    out, st = [], seed
    for _ in range(n):
        st, a = GM.splitmix64(st)
        st, b = GM.splitmix64(st)
        out.append(((a << 64) | b) & ((1 << bits) - 1))
    return out


def check(ctx, pool, scalars, off, vec, pat, base, bits=128):
    """one call against the model; the counter moves by the number of sums.  Returns the points"""
    x, y, inf, logs = pool
    before = ctx.rlc_shared_sums()
    got = ctx.e2_msm_shared(scalars, x, y, inf, off, vec, pat, base, bits)
    assert ctx.rlc_shared_sums() - before == len(vec)
    exp = SM.msm_shared(EM.LOGS, scalars, logs, off, vec, pat, base)
    assert got == LM.logs_to_points(exp)
    return got


def patterns(n_terms):
    """the points in order (round the first 100); a walk with repeats; one with holes (every fifth entry is no term)"""
    return [[t % 100 for t in range(n_terms)], [(7 * t + 3) % 40 for t in range(n_terms)], [-1 if t % 5 == 0 else t % 100 for t in range(n_terms)]]


@pytest.mark.parametrize("n_terms", [1, 2, 100, 513, 800])
@pytest.mark.parametrize("spv", [1, 63, 64, 65])
def test_sums_per_vector_and_terms(ctx, pool, spv, n_terms):
    """vector 0 has spv sums, vector 1 has three; the sums come interleaved.  513 and 800 terms: two and three segments of terms, the last one shorter"""
    scalars = [rand_scalars(spv * 1000 + n_terms, n_terms), rand_scalars(spv * 1000 + n_terms + 500, n_terms)]
    sums = [(0, s % 3, s % 40) for s in range(spv)]
    for at, s in ((0, 0), (len(sums) // 2 + 1, 1), (len(sums) + 2, 2)):  # vector 1 before, amid and after vector 0
        sums.insert(at, (1, s, 11 + s))
    assert sums[0][0] == 1 and sums[-1][0] == 1 and sum(v for v, _, _ in sums) == 3
    check(ctx, pool, scalars, patterns(n_terms), [s[0] for s in sums], [s[1] for s in sums], [s[2] for s in sums])


def edge_case(name):
    if name == "zero":
        return [0] * 6, 128
    if name == "equal":
        return [0x1234_5678_9ABC_DEF0_0FED_CBA9_8765_4321] * 6, 128  # every term lands in the same bucket of every window
    if name == "ones":
        return [(1 << 128) - 1] * 6, 128
    bits = int(name[4:])
    return SM.edge_values(bits), bits


@pytest.mark.parametrize("name", ["zero", "equal", "ones", "edge128", "edge127", "edge8"])
def test_scalars_at_the_window_edges(ctx, pool, name):
    """all zero; all equal; 2^128 - 1 at every term; 0, 1, 2^k - 1, 2^k, 2^k + 1 around every window edge with scalar_bits 128,
    127 and 8 (one-byte scalars).  The points walk round the first 40 with repeats, so most edge scalars meet several points"""
    vals, bits = edge_case(name)
    n_terms = len(vals)
    scalars = [vals, list(reversed(vals))]
    off = [[t % 40 for t in range(n_terms)], [(3 * t + 1) % 40 for t in range(n_terms)]]
    got = check(ctx, pool, scalars, off, [0, 1, 0, 1, 0], [0, 0, 1, 1, 0], [0, 17, 40, 100, 119], bits)
    if name == "zero":
        assert got == [None] * 5


def test_one_point_at_every_term_doubles_inside_a_bucket(ctx, pool):
    """off = 0 throughout and equal scalars: every bucket that is hit receives the same point again and again: P, 2 P (the
    doubling branch of the mixed addition), 3 P, ..; with unequal scalars the point spreads over the buckets"""
    n_terms = 9
    same = [[0x0B5E_0000_0000_0000_0000_0000_0000_0B5E] * n_terms, rand_scalars(77, n_terms)]
    off = [[0] * n_terms]
    check(ctx, pool, same, off, [0, 1, 0, 1], [0, 0, 0, 0], [3, 3, 4, 8])


def test_opposite_points_repeats_identities_and_empty_patterns(ctx, pool):
    """P and -P under equal scalars give the identity; point 5 repeats point 4; flagged identities add nothing; a pattern that is
    negative throughout is a sum with no term; a pattern with holes as pad = 1 leaves them (the window rule of a 4 x 4 plane)"""
    eq = [0xFEDC_BA98_7654_3210_0123_4567_89AB_CDEF] * 4
    off = [[6, 7, -1, -1], [4, 5, 4, 5], [9, 20, 9, 20], [-1, -1, -1, -1], [9, 6, 20, 7]]
    got = check(ctx, pool, [eq, rand_scalars(3, 4)], off, [0, 0, 0, 0, 0, 1, 1, 1], [0, 1, 2, 3, 4, 0, 3, 4], [0] * 8)
    assert got[0] is None and got[1] is not None and got[2] is None and got[3] is None and got[4] is None
    assert got[5] is not None and got[6] is None
    win = SM.window_offsets(4, 4, 3, 3, 1, 1)  # 9 taps over 16 outputs, and the outputs themselves
    assert any(o < 0 for o in win[0]) and all(o >= 0 for o in win[4]) and win[9] == list(range(16))
    n = len(win)
    check(ctx, pool, [rand_scalars(5, 16), rand_scalars(6, 16)], win, [s % 2 for s in range(2 * n)], [s // 2 for s in range(2 * n)],
          [16 * (s % 2) + 50 for s in range(2 * n)])


def test_every_sum_against_the_single_sum_entry_point(ctx, pool):
    """vpin_e2_msm runs the one-lane-per-term kernel: an independent device-side check, sum by sum"""
    x, y, inf, _ = pool
    n_terms = 10
    scalars = [rand_scalars(21, n_terms), rand_scalars(22, n_terms)]
    off = patterns(n_terms)
    vec, pat, base = [0, 1, 1, 0, 1], [0, 1, 2, 1, 0], [0, 2, 4, 6, 100]
    got = ctx.e2_msm_shared(scalars, x, y, inf, off, vec, pat, base)
    for s in range(5):
        idx = [base[s] + o for o in off[pat[s]] if o >= 0]
        sc = [scalars[vec[s]][t] for t, o in enumerate(off[pat[s]]) if o >= 0]
        assert got[s] == ctx.e2_msm(sc, x[idx], y[idx], inf[idx]), s


def test_chunks_just_past_the_cap(ctx, pool):
    """the cap set to two tiles of per-window results (a test hook): 130 + 3 sums are three tiles of vector 0 and one of vector 1,
    so the walk takes two chunks and the second begins inside vector 0"""
    n_terms = 3
    per_tile = 64 * SM.n_windows(128) * 96
    ctx.set_rlc_shared_cap(2 * per_tile)
    try:
        scalars = [rand_scalars(31, n_terms), rand_scalars(32, n_terms)]
        vec = [0] * 130 + [1] * 3
        check(ctx, pool, scalars, patterns(n_terms), vec, [s % 3 for s in range(133)], [s % 100 for s in range(133)])
        ctx.set_rlc_shared_cap(1)  # below one tile: a tile a chunk
        check(ctx, pool, scalars, patterns(n_terms), vec[60:], [s % 3 for s in range(73)], [s for s in range(73)])
    finally:
        ctx.set_rlc_shared_cap(0)


def test_a_warm_context_stays_out_of_the_driver(ctx, pool):
    import vpin_amd
    args = ([rand_scalars(41, 5), rand_scalars(42, 5)], patterns(5), [0, 1] * 40, [0, 1, 2, 0] * 20, list(range(80)))
    check(ctx, pool, *args)
    calls = vpin_amd.Context.driver_alloc_stats()[0]
    check(ctx, pool, *args)
    assert vpin_amd.Context.driver_alloc_stats()[0] == calls


def test_rejections(ctx, pool):
    """every rule of the header, by its text; a rejected call does not move the counter"""
    import vpin_amd
    from vpin_amd import capi
    x, y, inf, _ = pool
    good = dict(scalars=[[1, 2, 3], [4, 5, 255]], x=x, y=y, inf=inf, off=[[0, 1, 2], [-1, 5, N_POINTS - 1]], vec=[0, 1], pat=[0, 1], base=[0, 0],
                scalar_bits=8)
    before = ctx.rlc_shared_sums()

    def rejected(**kw):
        a = dict(good, **kw)
        with pytest.raises(vpin_amd.VpinError) as ei:
            ctx.e2_msm_shared(a["scalars"], a["x"], a["y"], a["inf"], a["off"], a["vec"], a["pat"], a["base"], a["scalar_bits"])
        assert ei.value.code == -1
        return str(ei.value)

    assert "vec[s] is not below n_vec" in rejected(vec=[0, 2])
    assert "pat[s] is not below n_pat" in rejected(pat=[2, 0])
    assert "outside the points" in rejected(base=[0, 1])
    assert "outside the points" in rejected(off=[[0, 1, N_POINTS], [0, 0, 0]])
    assert "at or above scalar_bits" in rejected(scalars=[[1, 2, 3], [4, 5, 256]])
    assert "at or above scalar_bits" in rejected(scalars=[[1, 2, 1 << 127], [4, 5, 6]], scalar_bits=127)
    assert "scalar_bits must be in 1 .. 128" in rejected(scalar_bits=0)
    assert "scalar_bits must be in 1 .. 128" in rejected(scalar_bits=129)
    off_curve = y.copy()
    off_curve[3, 0] ^= 1
    assert "not on the curve" in rejected(y=off_curve)
    big = x.copy()
    big[8] = np.frombuffer(Q.to_bytes(32, "little"), np.uint8)
    assert "not below q" in rejected(x=big)
    # the counts and the null arguments: the C ABI itself
    L = capi.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = ctx._u128s([1, 2, 3, 4, 5, 6])
    off = np.array(good["off"], np.int32).reshape(-1)
    u = np.zeros(2, np.uint32)
    ox, oy, oi = np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)

    def raw(n_vec=2, n_terms=3, n_points=N_POINTS, n_pat=2, n_sums=2, null=None):
        ptr = [p(s), p(x), p(y), p(inf), p(off), p(u), p(u), p(u), p(ox), p(oy), p(oi)]
        if null is not None:
            ptr[null] = None
        rc = L.vpin_e2_msm_shared(ctx.h, ptr[0], n_vec, n_terms, 8, ptr[1], ptr[2], ptr[3], n_points, ptr[4], n_pat, ptr[5], ptr[6], ptr[7], n_sums,
                                  ptr[8], ptr[9], ptr[10])
        return rc, L.vpin_last_error()

    assert raw()[0] == 0
    assert ctx.rlc_shared_sums() == before + 2
    for i in range(11):
        rc, msg = raw(null=i)
        assert rc == -1 and b"null argument" in msg, i
    rc = L.vpin_e2_msm_shared(None, p(s), 2, 3, 8, p(x), p(y), p(inf), N_POINTS, p(off), 2, p(u), p(u), p(u), 2, p(ox), p(oy), p(oi))
    assert rc == -1
    for kw in (dict(n_vec=0), dict(n_terms=0), dict(n_points=0), dict(n_pat=0), dict(n_sums=0)):
        rc, msg = raw(**kw)
        assert rc == -1 and b"a count is zero" in msg, kw
    for kw in (dict(n_sums=1 << 31), dict(n_sums=1 << 20, n_terms=1 << 11)):
        rc, msg = raw(**kw)
        assert rc == -1 and b"above 2^31 - 1" in msg, kw
    assert ctx.rlc_shared_sums() == before + 2
    ctx.e2_msm_shared(**{k: good[k] for k in ("scalars", "x", "y", "inf", "off", "vec", "pat", "base", "scalar_bits")})  # unspoilt: accepted
