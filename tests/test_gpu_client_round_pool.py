"""GPU tests of the client's round with max pooling as one launch chain (vpin_e2_client_round_pool, e2_act_pool_kernel): the raw
decryptions, the pooled and activated values and the re-encrypted points against tests/maxpool_model.py, tests/lenet_model.py and
tests/elgamal_model.py.  Every comparison is exact.

The baby-step table has 2^12 entries and the values stay within +-2^20 (max_giant = 2^8: a walk four shared inversions deep), so
every case takes a fraction of a second."""
import numpy as np
import pytest

import elgamal_model as EM
import lenet_model as LM
import maxpool_model as MM
from test_gpu_enc_conv import points_of

pytestmark = pytest.mark.gpu

N = EM.ORDER
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % N
NB = 1 << 12
GIANT = 1 << 8
BOUND = 1 << 19
EINVAL, ESHAPE = -1, -5
# remainders dropped and planes adjacent; overlapping windows; gaps; one output per plane; 63, 64, 65 and 257 outputs (around a
# wavefront and past a workgroup of the activation and of the encryption)
SHAPES = [(1, 4, 4, 2, 2), (3, 5, 7, 2, 2), (2, 5, 5, 3, 1), (2, 6, 6, 2, 3), (3, 3, 3, 3, 1),
          (1, 18, 14, 2, 2), (1, 16, 16, 2, 2), (5, 26, 2, 2, 2), (1, 2, 514, 2, 2)]


def tables(ctx):
    from vpin_amd import elgamal as E
    g = E.BaseTable(ctx)
    return g, E.BaseTable(ctx, E.keygen(g, SK)), E.DlogTable(ctx, NB)


@pytest.fixture(scope="module")
def env():
    import vpin_amd
    ctx = vpin_amd.Context(0)
    g, h, t = tables(ctx)
    yield ctx, g, h, t
    t.free()
    h.free()
    g.free()
    ctx.close()


def values(seed, n, bound=BOUND):
    """n seeded values of both signs below `bound` in magnitude"""
    return [(seed * 2654435761 + i * 40503 * 65537 + i * i * 977) % (2 * bound - 1) - (bound - 1) for i in range(n)]


def pooled(env, vals, shape, relu, bits, reencrypt=True, seed=0x9001, exact_points=(0,)):
    """encrypt vals, run the pooled round, check v and act against the model and the ciphertexts against vpin_e2_encrypt of the model's
    act under the same r (and, at exact_points, against the model's own encryption).  Returns everything the round returned"""
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    planes, H, W, k, stride = shape
    c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(seed, len(vals)))
    exp = MM.pooled_round(vals, planes, H, W, k, stride, relu, bits)
    rs = EM.splitmix_scalars(seed + 1, len(exp)) if reencrypt else None
    v, act, o1, o2 = ctx.e2_client_round_pool(t.h, g.h, h.h, SK, c1, c2, planes, H, W, k, stride, GIANT, relu, bits, rs)
    assert [int(a) for a in v] == list(vals), "every raw decryption"
    assert [int(a) for a in act] == exp
    if not reencrypt:
        assert o1 is None and o2 is None
        return v, act, o1, o2
    e1, e2 = E.encrypt(g, h, exp, rs)
    for got, want in zip(o1 + o2, e1 + e2):
        assert got.shape == want.shape and np.array_equal(got, want)
    pub = EM.keygen(SK)
    for i in exact_points:
        m1, m2 = EM.encrypt(pub, exp[i], rs[i])
        assert points_of(o1[0][i], o1[1][i], o1[2][i:i + 1]) == [m1] and points_of(o2[0][i], o2[1][i], o2[2][i:i + 1]) == [m2]
    return v, act, o1, o2


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_model(env, shape):
    planes, H, W, k, stride = shape
    Ho, Wo = MM.out_dims(H, W, k, stride)
    n_out = planes * Ho * Wo
    assert shape not in SHAPES[5:] or n_out == (63, 64, 65, 257)[SHAPES.index(shape) - 5]
    relu, bits = (1, 18) if sum(shape) % 2 else (0, 0)
    vals = values(sum(shape) + 31 * H, planes * H * W)
    assert min(vals) < 0 < max(vals)
    pooled(env, vals, shape, relu, bits, seed=0x9000 + 16 * sum(shape), exact_points=sorted({0, n_out - 1}))


def test_the_maximum_at_each_corner_of_a_window(env):
    """plane p of four holds every window's maximum at corner p (top left, top right, bottom left, bottom right); negative elsewhere"""
    H = W = 4
    vals = []
    for p in range(4):
        for y in range(H):
            for x in range(W):
                corner = 2 * (y % 2) + x % 2
                vals.append(1000 + 10 * (y // 2 * 2 + x // 2) + p if corner == p else -(50 + 7 * y + x))
    _, act, _, _ = pooled(env, vals, (4, 4, 4, 2, 2), 0, 0)
    assert [int(a) for a in act] == [1000 + 10 * w + p for p in range(4) for w in range(4)]


@pytest.mark.parametrize("shape", [(2, 2, 2, 2, 2), (2, 3, 3, 2, 1)])
def test_a_window_never_crosses_a_plane(env, shape):
    """the maximum of plane 0 in its last element, next to a larger value in the first element of plane 1"""
    planes, H, W, k, stride = shape
    per = H * W
    vals = [-(3 + i) for i in range(2 * per)]
    vals[per - 1] = 77
    vals[per] = 5000
    _, act, _, _ = pooled(env, vals, shape, 0, 0)
    Ho, Wo = MM.out_dims(H, W, k, stride)
    assert int(act[Ho * Wo - 1]) == 77 and int(act[Ho * Wo]) == 5000 and 5000 not in [int(a) for a in act[:Ho * Wo]]


@pytest.mark.parametrize("relu,bits", [(1, 0), (0, 18)])
def test_k_1_stride_1_is_the_plain_round_byte_for_byte(env, relu, bits):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    vals = values(0x51, 3 * 5 * 7)
    c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(0x52, len(vals)))
    rs = EM.splitmix_scalars(0x53, len(vals))
    plain = ctx.e2_client_round(t.h, g.h, h.h, SK, c1, c2, GIANT, relu, bits, rs)
    pool = ctx.e2_client_round_pool(t.h, g.h, h.h, SK, c1, c2, 3, 5, 7, 1, 1, GIANT, relu, bits, rs)
    assert np.array_equal(plain[0], pool[0]) and np.array_equal(plain[1], pool[1])
    for a, b in zip(plain[2] + plain[3], pool[2] + pool[3]):
        assert a.tobytes() == b.tobytes()


def test_the_last_round_may_pool_and_encrypts_nothing(env):
    pooled(env, values(0x61, 2 * 5 * 5), (2, 5, 5, 3, 1), 1, 0, reencrypt=False)


def test_all_negative_windows_with_and_without_relu(env):
    vals = [-(1 + (37 * i) % 1000) for i in range(32)]
    _, act, _, _ = pooled(env, vals, (2, 4, 4, 2, 2), 0, 0)
    assert all(int(a) < 0 for a in act)
    _, act, _, _ = pooled(env, vals, (2, 4, 4, 2, 2), 1, 0)
    assert all(int(a) == 0 for a in act)


def raises(code, match, fn):
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError, match=match) as e:
        fn()
    assert e.value.code == code, e.value


def test_an_unfound_value_inside_a_window_names_the_input_index(env):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    shape = (2, 5, 5, 2, 2)  # windows cover rows and columns 0 .. 3 of every plane
    vals = values(0x71, 50, 1 << 12)
    far = 4 * NB + 5  # max_giant = 3 covers +-(4 nb - 1)
    inside = 25 + 2 * 5 + 3  # plane 1, row 2, column 3: the first of the two planted inside a window
    vals[inside] = far
    vals[25 + 3 * 5 + 1] = -far
    c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(0x72, 50))
    rs = EM.splitmix_scalars(0x73, 8)
    run = lambda giant: ctx.e2_client_round_pool(t.h, g.h, h.h, SK, c1, c2, *shape, giant, True, 0, rs)
    raises(ESHAPE, "vpin_e2_client_round_pool: element %d, inside a window, has no value within the walk's range" % inside, lambda: run(3))
    v, act, _, _ = run(4)
    assert [int(a) for a in v] == vals and [int(a) for a in act] == MM.pooled_round(vals, *shape, 1, 0) and far in [int(a) for a in act]


def test_an_unfound_value_outside_every_window_is_no_error(env):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    far = 4 * NB + 5
    for shape, outside in (((2, 5, 5, 2, 2), [4, 24, 25 + 4 * 5 + 1]),   # the dropped column and row
                           ((1, 6, 6, 2, 3), [2, 2 * 6 + 3, 5 * 6 + 5])):  # the gaps of stride 3 over windows of 2, and the remainder
        planes, H, W, k, stride = shape
        assert not any(MM.in_a_window(H, W, k, stride, i) for i in outside)
        vals = values(0x81, planes * H * W, 1 << 12)
        for i in outside:
            vals[i] = far
        c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(0x82, len(vals)))
        n_out = planes * MM.out_dims(H, W, k, stride)[0] * MM.out_dims(H, W, k, stride)[1]
        v, act, o1, _ = ctx.e2_client_round_pool(t.h, g.h, h.h, SK, c1, c2, *shape, 3, False, 0, EM.splitmix_scalars(0x83, n_out))
        assert [int(a) for a in v] == [0 if i in outside else x for i, x in enumerate(vals)], "reported in v_out as 0"
        assert [int(a) for a in act] == MM.pooled_round(vals, *shape, 0, 0) and o1[2].shape == (n_out,)


def test_a_shifted_maximum_past_int32_names_the_output_index(env):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    # shifting(v, 1) = v * 2^15: int32 holds 2^31 - 2^15 (v = 2^16 - 1) but not 2^31 (v = 2^16)
    vals = [2**16 - 1, 5, -9, 0,
            7, 2**16, 2**16 - 1, -(2**16) - 1]
    assert LM.shifting(2**16, 1) is None and LM.shifting(-(2**16) - 1, 1) is None
    c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(0x91, 8))
    run = lambda a, b, planes: ctx.e2_client_round_pool(t.h, g.h, h.h, SK, a, b, planes, 2, 2, 2, 2, GIANT, False, 1, EM.splitmix_scalars(0x92, planes))
    raises(ESHAPE, "vpin_e2_client_round_pool: the activated value of output element 1 \\(the maximum decrypted, 65536\\) does not fit",
           lambda: run(c1, c2, 2))
    first = ([a[:4] for a in c1], [a[:4] for a in c2])  # the negative value that would not fit is never the maximum
    _, act, _, _ = run(first[0], first[1], 1)
    assert [int(a) for a in act] == [2**31 - 2**15]


def test_rejections(env):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    c1, c2 = E.encrypt(g, h, list(range(1, 17)), EM.splitmix_scalars(0xA1, 16))

    def rnd(shape=(1, 4, 4, 2, 2), sk=SK, giant=3, bits=0, rs=(7, 8, 9, 10), a=c1, b=c2):
        return ctx.e2_client_round_pool(t.h, g.h, h.h, sk, a, b, *shape, giant, True, bits, list(rs))

    who = "vpin_e2_client_round_pool: "
    raises(EINVAL, who + "planes, H or W is zero", lambda: rnd((0, 4, 4, 2, 2)))
    raises(EINVAL, who + "planes, H or W is zero", lambda: rnd((1, 0, 4, 2, 2)))
    raises(EINVAL, who + "planes, H or W is zero", lambda: rnd((1, 4, 0, 2, 2)))
    raises(EINVAL, who + "the window k or the stride is zero", lambda: rnd((1, 4, 4, 0, 2)))
    raises(EINVAL, who + "the window k or the stride is zero", lambda: rnd((1, 4, 4, 2, 0)))
    raises(EINVAL, who + "the window k does not fit the H x W plane", lambda: rnd((2, 2, 4, 3, 1)))
    raises(EINVAL, who + "the window k does not fit the H x W plane", lambda: rnd((2, 4, 2, 3, 1)))
    raises(EINVAL, who + "planes \\* H \\* W must be in 1 .. 2\\^30 - 1", lambda: rnd((1 << 10, 1 << 10, 1 << 10, 2, 2)))
    raises(EINVAL, who + "planes \\* H \\* W must be in 1 .. 2\\^30 - 1", lambda: rnd((1 << 40, 1 << 40, 1 << 40, 2, 2)))
    raises(EINVAL, who + "the key sk is zero", lambda: rnd(sk=0))
    raises(EINVAL, who + "the key sk is not below the group order", lambda: rnd(sk=N))
    raises(EINVAL, who + "a randomness r is zero", lambda: rnd(rs=(7, 8, 9, 0)))
    raises(EINVAL, who + "a randomness r is not below the group order", lambda: rnd(rs=(N, 8, 9, 10)))
    raises(EINVAL, who + "shift_bits must be 0", lambda: rnd(bits=63))
    raises(EINVAL, who + "shift_bits must be 0", lambda: rnd(bits=-1))
    raises(EINVAL, who + "max_giant \\* nb is past 2\\^62", lambda: rnd(giant=2**62 // NB + 1))
    bad = (c1[0].copy(), c1[1].copy(), c1[2])
    bad[1][1, 0] ^= 1
    raises(EINVAL, "vpin_e2_client_round_pool: .*c1 point is not on the curve", lambda: rnd(a=bad))
    v, act, _, _ = rnd()
    assert [int(x) for x in v] == list(range(1, 17)) and [int(x) for x in act] == [6, 8, 14, 16]


def test_the_same_bytes_on_a_context_whose_pool_is_poisoned(env):
    """every device block the round takes from the pool is filled with a poison word first: what the kernels do not write
    themselves (the decryptions of elements outside every window, the padding of a message) would show"""
    import vpin_amd
    from vpin_amd import elgamal as E
    shape = (3, 5, 7, 2, 3)
    vals = values(0xB1, 3 * 5 * 7)
    want = pooled(env, vals, shape, 1, 18, seed=0xB2)
    ctx = vpin_amd.Context(0)
    ctx.set_pool_poison(0xA5A5A5A5)
    g, h, t = tables(ctx)
    try:
        got = pooled((ctx, g, h, t), vals, shape, 1, 18, seed=0xB2)
        assert ctx.pool_poison_stats()[0] > 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for a, b in zip(got[2] + got[3], want[2] + want[3]):
            assert a.tobytes() == b.tobytes()
    finally:
        t.free()
        h.free()
        g.free()
        ctx.close()
