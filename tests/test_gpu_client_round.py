"""GPU tests of one round of the client as a single launch chain (vpin_e2_client_round, e2_act_kernel): decryption, the
activation and the encryption of the result, against tests/lenet_model.py and tests/elgamal_model.py and on the inputs of the
reference's own relu / shifting runs (tests/golden/inference_pins.json).  Every comparison is exact.

The baby-step table has 2^16 entries and the rounds stay within +-2^30 (max_giant = 2^14, a walk 256 shared inversions deep).
Over that table the walk of six values with max_giant = 2^17 / 2^19 / 2^21 measured 0.74 / 2.6 / 9.5 s on an MI355X, so 2^23 would
be ~40 s, not seconds: the values over the 2^16 table are therefore lowered to what it covers quickly, and the pinned values
beyond 2^30, up to 2^39, run over a table of 2^24 baby steps instead (2^15 giant steps, 512 shared inversions deep)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import elgamal_model as EM
import gadgets_model as GM
import lenet_model as LM
from test_gpu_enc_conv import points_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "inference_pins.json")) as f:
    PINS = json.load(f)["client"]
N = EM.ORDER
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % N
NB = 1 << 16
GIANT = 1 << 14   # +-2^30
SMALL = 1 << 30


@pytest.fixture(scope="module")
def env():
    import vpin_amd
    from vpin_amd import elgamal as E
    ctx = vpin_amd.Context(0)
    g = E.BaseTable(ctx)
    h = E.BaseTable(ctx, E.keygen(g, SK))
    t = E.DlogTable(ctx, NB)
    yield ctx, g, h, t
    t.free()
    h.free()
    g.free()
    ctx.close()


def pinned(name, lo=0, hi=SMALL):
    c = PINS[name]
    return [(int(v), int(r)) for v, r in zip(c["values"], c["results"]) if lo <= abs(int(v)) < hi]


def one_round(env, values, relu, bits, reencrypt=True, giant=GIANT, seed=0xC11E):
    """encrypt `values`, run the round, check v and act against the model and the ciphertext against vpin_e2_encrypt of the
    model's act under the same r (and, for a few elements, against the model's own encryption).  Returns act"""
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    n = len(values)
    c1, c2 = E.encrypt(g, h, values, EM.splitmix_scalars(seed, n))
    rs = EM.splitmix_scalars(seed + 1, n) if reencrypt else None
    v, act, o1, o2 = ctx.e2_client_round(t.h, g.h, h.h, SK, c1, c2, giant, relu, bits, rs)
    exp = [LM.activate(a, relu, bits) for a in values]
    assert [int(a) for a in v] == list(values)
    assert [int(a) for a in act] == exp
    if not reencrypt:
        assert o1 is None and o2 is None
        return exp
    e1, e2 = E.encrypt(g, h, exp, rs)
    for got, want in zip(o1 + o2, e1 + e2):
        assert np.array_equal(got, want)
    H = EM.keygen(SK)
    for i in sorted({0, 1, n // 2, n - 1}):
        m1, m2 = EM.encrypt(H, exp[i], rs[i])
        assert points_of(o1[0][i], o1[1][i], o1[2][i:i + 1]) == [m1] and points_of(o2[0][i], o2[1][i], o2[2][i:i + 1]) == [m2]
    return exp


def test_relu_round_on_the_pinned_inputs(env):
    vals = [v for v, _ in pinned("relu")]
    assert min(vals) < 0 < max(vals)
    exp = one_round(env, vals, True, 0)
    assert exp == [r for _, r in pinned("relu")]


def test_shift_26_round_on_the_pinned_inputs(env):
    pins = pinned("shifting_26")
    assert len(pins) > 30 and max(abs(v) for v, _ in pins) > 2**24
    exp = one_round(env, [v for v, _ in pins], False, 26)
    assert exp == [r for _, r in pins]
    assert sum(LM.shift_int(v, 26) != r for v, r in pins) >= 3  # an integer shift would not pass


def test_relu_shift_33_round_on_the_pinned_inputs(env):
    pins = pinned("shifting_33")
    exp = one_round(env, [v for v, _ in pins], True, 33)
    assert exp == [r if v > 0 else 0 for v, r in pins]


def test_last_round_does_not_encrypt(env):
    one_round(env, [5, -5, 0, 2**29, -(2**29)], True, 0, reencrypt=False)


def test_257_elements(env):
    """past a workgroup of the activation and of every stage around it"""
    pins = pinned("shifting_26")
    vals = [v for v, _ in pins] + [(i * 7919 * 65537 + 12345) % (2**31 - 3) - (2**30 - 1) for i in range(257 - len(pins))]
    assert len(vals) == 257 and max(abs(v) for v in vals) < SMALL
    one_round(env, vals, False, 26)


@pytest.fixture(scope="module")
def env_2_24(env):
    from vpin_amd import elgamal as E
    ctx, g, h, _ = env
    t = E.DlogTable(ctx, 1 << 24)
    yield ctx, g, h, t
    t.free()


@pytest.mark.parametrize("bits,name", [(26, "shifting_26"), (33, "shifting_33")])
def test_pinned_large_values(env_2_24, bits, name):
    """every pinned input between 2^30 and 2^39, both signs: the sizes R6 and R7 of the real network decrypt to"""
    pins = pinned(name, 2**30, 2**39)
    assert len(pins) >= 30 and min(v for v, _ in pins) < -2**38 and max(v for v, _ in pins) > 2**38
    exp = one_round(env_2_24, [v for v, _ in pins], False, bits, giant=1 << 15)
    assert exp == [r for _, r in pins]


def eshape(fn, match):
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError, match=match) as e:
        fn()
    assert e.value.code == -5


def test_value_outside_the_walk_names_the_index(env):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    vals = [3, -7, 4 * NB + 5, 9]  # max_giant = 3 covers +-(4 nb - 1)
    c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(0xE5, 4))
    eshape(lambda: ctx.e2_client_round(t.h, g.h, h.h, SK, c1, c2, 3, True, 0, EM.splitmix_scalars(0xE6, 4)), "element 2 has no value")
    v, act, _, _ = ctx.e2_client_round(t.h, g.h, h.h, SK, c1, c2, 4, True, 0, EM.splitmix_scalars(0xE6, 4))
    assert [int(a) for a in v] == vals and [int(a) for a in act] == [3, 0, 4 * NB + 5, 9]


def test_shifted_value_past_int32_names_the_index(env):
    from vpin_amd import elgamal as E
    ctx, g, h, t = env
    vals = [2**16 - 1, 2**16, -(2**16), -(2**16) - 1]  # shifting(v, 1) = v * 2^15: int32 holds -2^31 but not 2^31
    assert [LM.shifting(v, 1) for v in vals] == [2**31 - 2**15, None, -(2**31), None]
    c1, c2 = E.encrypt(g, h, vals, EM.splitmix_scalars(0xE7, 4))
    eshape(lambda: ctx.e2_client_round(t.h, g.h, h.h, SK, c1, c2, 3, False, 1, EM.splitmix_scalars(0xE8, 4)), "element 1 ")
    keep = ([a[[0, 2]] for a in c1], [a[[0, 2]] for a in c2])
    v, act, _, _ = ctx.e2_client_round(t.h, g.h, h.h, SK, keep[0], keep[1], 3, False, 1, EM.splitmix_scalars(0xE8, 2))
    assert [int(a) for a in act] == [2**31 - 2**15, -(2**31)]


def test_rejections(env):
    import vpin_amd
    from vpin_amd import capi
    from vpin_amd import elgamal as E
    ctx, g, h, t = env

    def einval(fn, match):
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            fn()
        assert e.value.code == -1

    c1, c2 = E.encrypt(g, h, [5, 6], [11, 12])
    rnd = lambda sk=SK, a=c1, b=c2, giant=3, bits=0, rs=(7, 8): ctx.e2_client_round(t.h, g.h, h.h, sk, a, b, giant, True, bits, list(rs))
    einval(lambda: rnd(sk=0), "sk is zero")
    einval(lambda: rnd(sk=N), "group order")
    einval(lambda: rnd(rs=(7, 0)), "r is zero")
    einval(lambda: rnd(rs=(N, 7)), "group order")
    einval(lambda: rnd(bits=63), "shift_bits")
    einval(lambda: rnd(bits=-1), "shift_bits")
    einval(lambda: rnd(giant=2**62 // NB + 1), "2\\^62")
    bad = (c1[0].copy(), c1[1].copy(), c1[2])
    bad[1][1, 0] ^= 1
    einval(lambda: rnd(a=bad), "c1 point is not on the curve")
    big = (c2[0].copy(), c2[1], c2[2])
    big[0][0] = np.frombuffer(GM.Q.to_bytes(32, "little"), np.uint8)
    einval(lambda: rnd(b=big), "below q")
    # a missing r in a round that encrypts, through the C ABI itself
    L = capi.lib()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    k = np.frombuffer(SK.to_bytes(32, "little"), np.uint8).copy()
    v, act = np.zeros(2, np.int64), np.zeros(2, np.int64)
    out = [np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)] * 2
    rc = L.vpin_e2_client_round(ctx.h, t.h, g.h, h.h, p(k), p(c1[0]), p(c1[1]), p(c1[2]), p(c2[0]), p(c2[1]), p(c2[2]), 2, 3, 1, 0, 1,
                                None, p(v), p(act), *[p(a) for a in out])
    assert rc == -1 and b"null argument" in L.vpin_last_error()
    v, act, _, _ = rnd()
    assert [int(a) for a in v] == [5, 6]
