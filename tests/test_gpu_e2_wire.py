"""GPU test of the packed points (vpin_e2_pack, vpin_e2_unpack: e2_wire.hip) against tests/wire_model.py: pack is the model's
bytes and unpack(pack(P)) is P, byte for byte, over multiples of G and their negatives (both parities), the identity in every
position, the points over the smallest x and over q - 1, and every count around the workgroup size; and every rejection of an
encoding names its index and its rule, with the bad point first, last and alone.  Every rejection is a flagged return."""
import numpy as np
import pytest

import gadgets_model as GM
import wire_model as WM
from test_gpu_enc_conv import points_of, to_arrays

pytestmark = pytest.mark.gpu

Q = WM.Q


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def multiples():
    """k * G for k = 1 .. 64, computed once"""
    out, P = [], None
    for _ in range(64):
        P = GM.e2_add(P, WM.G)
        out.append(P)
    return out


def neg(P):
    return None if P is None else (P[0], (Q - P[1]) % Q)


def packed(points):
    return np.frombuffer(b"".join(WM.pack(P) for P in points), dtype=np.uint8).reshape(-1, 32)


def check_round_trip(ctx, points):
    got = ctx.e2_pack(*to_arrays(points))
    assert np.array_equal(got, packed(points)), "pack differs from the model"
    x, y, inf = ctx.e2_unpack(got)
    assert points_of(x, y, inf) == points, "unpack(pack(P)) is not P"
    ex, ey, einf = to_arrays(points)
    assert np.array_equal(x, ex) and np.array_equal(y, ey) and np.array_equal(inf, einf)


def test_multiples_of_g_and_their_negatives(ctx, multiples):
    pts = multiples + [neg(P) for P in multiples]
    assert {P[1] & 1 for P in pts} == {0, 1}
    check_round_trip(ctx, pts)
    assert bytes(ctx.e2_pack(*to_arrays([WM.G]))[0]).hex() == "74a7eb7c9dce1e21936a3597795040247267cda53cba65f570abb33b6bfd150a"


def test_identity_in_every_position(ctx, multiples):
    for pts in ([None], [None, multiples[0], multiples[1]], [multiples[0], None, multiples[1]], [multiples[0], multiples[1], None], [None] * 3):
        check_round_trip(ctx, pts)
    assert bytes(ctx.e2_pack(*to_arrays([None]))[0]) == bytes(31) + b"\x40"


def test_the_points_over_small_x_and_q_minus_1(ctx):
    pts = [WM.lift(x, par) for x in (0, 1, 2, 3, 4, Q - 1) for par in (0, 1)]
    assert all(P is not None for P in pts)
    check_round_trip(ctx, pts)
    got = ctx.e2_pack(*to_arrays(pts[:2]))
    assert bytes(got[0]) == bytes(32) and bytes(got[1]) == bytes(31) + b"\x80"  # (0, +-sqrt(b)): 32 zero bytes is a point


@pytest.mark.parametrize("cnt", [1, 255, 256, 257, 513])
def test_counts_around_the_workgroup(ctx, multiples, cnt):
    base = multiples + [neg(P) for P in multiples] + [None]
    check_round_trip(ctx, [base[(7 * i + 3) % len(base)] for i in range(cnt)])


def _word(v):
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


BAD_WORDS = [(5, "x is not on the curve E2"), (6, "x is not on the curve E2"), (7, "x is not on the curve E2"),
             (Q - 2, "x is not on the curve E2"), (Q, "x is not below q"), (Q + 1, "x is not below q"),
             (Q | WM.BIT_PARITY, "x is not below q"), (1 | WM.BIT_RESERVED, "bit 253 is set"),
             (WM.BIT_IDENTITY | 1, "the identity bit is set together with other bits"),
             (WM.BIT_IDENTITY | WM.BIT_PARITY, "the identity bit is set together with other bits"),
             (WM.BIT_IDENTITY | WM.BIT_RESERVED, "the identity bit is set together with other bits")]


@pytest.mark.parametrize("word, rule", BAD_WORDS, ids=[str(i) for i in range(len(BAD_WORDS))])
def test_unpack_rejections_name_index_and_rule(ctx, multiples, word, rule):
    import vpin_amd
    with pytest.raises(WM.WireError):
        WM.unpack(word.to_bytes(32, "little"))
    good = packed([multiples[i % 64] for i in range(299)] + [None])  # 300 points: two workgroups
    n = good.shape[0]
    for at, rows in ((0, n), (n - 1, n), (0, 1)):
        b = good[:rows].copy()
        b[at] = _word(word)
        with pytest.raises(vpin_amd.VpinError) as e:
            ctx.e2_unpack(b)
        assert e.value.code == -1 and "vpin_e2_unpack: point %d: %s" % (at, rule) in str(e.value)
    # two bad points: the first is named
    b = good.copy()
    b[3] = _word(word)
    b[n - 2] = _word(Q)
    with pytest.raises(vpin_amd.VpinError, match="point 3: "):
        ctx.e2_unpack(b)
    # and the context still unpacks
    x, y, inf = ctx.e2_unpack(good)
    assert points_of(x, y, inf)[-1] is None


def test_pack_rejections(ctx, multiples):
    import vpin_amd
    n = len(multiples)
    G2 = multiples[1]
    for at, pts in ((0, list(multiples)), (n - 1, list(multiples)), (0, [None])):
        pts[at] = (G2[0], (G2[1] + 1) % Q)  # off the curve
        with pytest.raises(vpin_amd.VpinError) as e:
            ctx.e2_pack(*to_arrays(pts))
        assert e.value.code == -1 and "vpin_e2_pack: point %d: the point is not on the curve E2" % at in str(e.value)
    x, y, inf = to_arrays(multiples[:3])
    x[1] = _word(Q)  # a coordinate that is not canonical
    with pytest.raises(vpin_amd.VpinError, match="vpin_e2_pack: point 1: a coordinate is not below q"):
        ctx.e2_pack(x, y, inf)
    with pytest.raises(vpin_amd.VpinError, match="cnt must be in"):
        ctx.e2_pack(x[:0], y[:0], inf[:0])
    p = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    assert vpin_amd.lib().vpin_e2_unpack(ctx.h, None, 1, p(x), p(y), p(inf)) == -1
    assert vpin_amd.lib().vpin_e2_pack(ctx.h, p(x), p(y), None, 3, p(x)) == -1
