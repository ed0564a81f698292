"""GPU tests of the client side on E2 (vpin_e2_base_*, vpin_e2_encrypt, vpin_e2_dlog_*, vpin_e2_decrypt): the fixed-base
multiplication and the encryption against the Python model tests/elgamal_model.py, the discrete logarithm at the edges of its
range, and the round trips that need no model point at all -- among them the plaintext check of the three encrypted layers:
encrypt an integer image, run the layer, decrypt, compare with numpy.

A model multiplication costs 10 to 17 ms, so every case keeps to tens of model points."""
import numpy as np
import pytest

import elgamal_model as EM
import gadgets_model as GM
from test_gpu_enc_conv import KEYS, point_at, points_of, to_arrays

pytestmark = pytest.mark.gpu

N = EM.ORDER
W = 10  # the default window width of a base table
SK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % N


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def base_g(ctx):
    from vpin_amd import elgamal as E
    b = E.BaseTable(ctx)
    yield b
    b.free()


@pytest.fixture(scope="module")
def base_h(ctx, base_g):
    from vpin_amd import elgamal as E
    b = E.BaseTable(ctx, E.keygen(base_g, SK))
    yield b
    b.free()


@pytest.fixture(scope="module")
def table_1000(ctx):
    from vpin_amd import elgamal as E
    t = E.DlogTable(ctx, 1000)
    yield t
    t.free()


@pytest.fixture(scope="module")
def table_64k(ctx):
    from vpin_amd import elgamal as E
    t = E.DlogTable(ctx, 1 << 16)
    yield t
    t.free()


def einval(fn, match):
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError, match=match) as e:
        fn()
    assert e.value.code == -1


# ---- fixed base -------------------------------------------------------------------------------------------------------

def special_scalars(w):
    """1, 2, the largest digit, the first of the second window, n - 1, (n - 1) / 2, a digit in the top window only, every digit
    of the full windows below it maximal"""
    top = (N.bit_length() - 1) // w * w
    out = [1, 2, 2**w - 1, 2**w, N - 1, (N - 1) // 2, (N >> top) << top, 2**top - 1]
    assert all(0 < s < N for s in out) and out[6].bit_length() > top and (out[6] & (2**top - 1)) == 0
    return out


SPECIAL = special_scalars(W)


@pytest.mark.parametrize("k", [1, 7])
def test_fixed_base_special_scalars(ctx, base_g, k):
    """the base G, and a second base 7 G: cnt = 1 and cnt = 65 (past a wave)"""
    from vpin_amd import elgamal as E
    base = base_g if k == 1 else E.BaseTable(ctx, EM.mul(7))
    x, y, inf = base.mul([SPECIAL[4]])
    assert points_of(x, y, inf) == [EM.mul(SPECIAL[4] * k % N)]
    scalars = SPECIAL + EM.splitmix_scalars(0xBA5E + k, 65 - len(SPECIAL), 0)
    x, y, inf = base.mul(scalars)
    for i in list(range(len(SPECIAL))) + [30, 64]:
        assert point_at(x, y, inf, i) == EM.mul(scalars[i] * k % N), f"scalar {i}"
    if k != 1:
        base.free()


@pytest.mark.parametrize("w", [5, 8, 12])
def test_fixed_base_other_widths(ctx, w):
    """vpin_e2_base_create_w: a width whose digits straddle the scalar's 32-bit words, the narrowest table with whole bytes, the
    widest; each with the special scalars of its own window layout"""
    from vpin_amd import elgamal as E
    base = E.BaseTable(ctx, None, w)
    scalars = special_scalars(w) + EM.splitmix_scalars(0xBA5E + w, 3, 0)
    x, y, inf = base.mul(scalars)
    assert points_of(x, y, inf) == [EM.mul(s) for s in scalars]
    base.free()
    einval(lambda: E.BaseTable(ctx, None, 3), "window width")
    einval(lambda: E.BaseTable(ctx, None, 13), "window width")


def test_fixed_base_past_a_workgroup_and_zero(ctx, base_g):
    scalars = EM.splitmix_scalars(0x257, 257, 0)
    scalars[100] = 0
    x, y, inf = base_g.mul(scalars)
    assert point_at(x, y, inf, 100) is None and int(inf.sum()) == 1
    for i in (0, 63, 64, 127, 128, 200, 231, 255, 256):  # 8 sampled indices and the last
        assert point_at(x, y, inf, i) == EM.mul(scalars[i]), f"scalar {i}"


def test_variable_base_matches_fixed_base(ctx, base_g):
    """the 256-bit double-and-add over replicated G against the window table: no model point"""
    scalars = SPECIAL + [0] + EM.splitmix_scalars(0x256, 70 - len(SPECIAL) - 1, 0)
    gx, gy, ginf = to_arrays([EM.G] * len(scalars))
    got = ctx.e2_mul256(scalars, gx, gy, ginf)
    exp = base_g.mul(scalars)
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)
    assert point_at(*got, i=4) == EM.mul(N - 1)


def test_fixed_base_rejections(ctx, base_g):
    from vpin_amd import elgamal as E
    einval(lambda: base_g.mul([1, N]), "group order")
    einval(lambda: E.BaseTable(ctx, (EM.G[0], (EM.G[1] + 1) % GM.Q)), "not on the curve")
    einval(lambda: E.BaseTable(ctx, (0, 0)), "identity")
    einval(lambda: E.BaseTable(ctx, (GM.Q, EM.G[1])), "below q")


# ---- encryption -------------------------------------------------------------------------------------------------------

def test_encrypt_literal(ctx, base_g, base_h):
    from vpin_amd import elgamal as E
    H = EM.keygen(SK)
    assert E.keygen(base_g, SK) == H
    msgs = [0, 1, -1, 65535, -(2**40)]
    rs = EM.splitmix_scalars(0xE2, len(msgs), 1, 2**104)  # 13 bytes
    c1, c2 = E.encrypt(base_g, base_h, msgs, rs)
    exp = [EM.encrypt(H, m, r) for m, r in zip(msgs, rs)]
    assert points_of(*c1) == [e[0] for e in exp]
    assert points_of(*c2) == [e[1] for e in exp]


def test_encrypt_complete_last_addition(ctx, base_g):
    """H = G: r = n - 5 with msg = 5 cancels (the flagged identity); r = 9 with msg = 9 coincides (the doubling)"""
    from vpin_amd import elgamal as E
    c1, c2 = E.encrypt(base_g, base_g, [5, 9], [N - 5, 9])
    assert points_of(*c2) == [None, EM.mul(18)]
    assert points_of(*c1) == [EM.mul(N - 5), EM.mul(9)]


def test_encrypt_rejections(ctx, base_g, base_h):
    from vpin_amd import elgamal as E
    einval(lambda: E.encrypt(base_g, base_h, [1, 2], [5, 0]), "zero")
    einval(lambda: E.encrypt(base_g, base_h, [1, 2], [N, 5]), "group order")
    einval(lambda: E.encrypt(base_g, base_h, [2**62], [5]), "message")
    einval(lambda: E.encrypt(base_g, base_h, [-(2**62)], [5]), "message")


# ---- the discrete logarithm ---------------------------------------------------------------------------------------------

def test_dlog_edges_nb_1000(ctx, table_1000):
    """nb = 1000 (slots != entries), max_giant = 3: every value up to 3999 in absolute value, and no further"""
    assert table_1000.nb == 1000 and 49 * 1000 <= table_1000.device_bytes <= 65 * 1000  # the header's bytes per entry
    vs = [0, 1, -1, 999, 1000, -1000, 1001, -1001, 2000, -2000, 2017, -2017, 3999, -3999, 4000, -4000]
    pts = [EM.mul(v) for v in vs]
    pts.append(EM.neg(EM.mul(17)))
    assert pts[0] is None
    v, found = table_1000.solve(to_arrays(pts), 3)
    assert [int(f) for f in found] == [1] * 14 + [0, 0, 1]
    assert [int(a) for a in v] == vs[:14] + [0, 0, -17]


def test_dlog_257_lanes_finish_at_different_steps(ctx, table_1000):
    """v = ((37 i) mod 7999) - 3999: values met at the giant steps 0 to 3 mixed inside every workgroup (four lanes a point at
    max_giant = 3, so 64 points a workgroup), and the 257th point in a workgroup of its own"""
    vs = [(i * 37) % 7999 - 3999 for i in range(257)]
    assert min(abs(v) for v in vs) < 1000 and max(abs(v) for v in vs) > 3000
    step, wrap = EM.mul(37), EM.mul(-7999)
    pts, P = [], EM.mul(vs[0])
    for i in range(257):
        pts.append(P)
        P = GM.e2_add(P, step)
        if i + 1 < 257 and vs[i + 1] < vs[i]:
            P = GM.e2_add(P, wrap)
    assert pts[256] == EM.mul(vs[256])
    v, found = table_1000.solve(to_arrays(pts), 3)
    assert found.all() and [int(a) for a in v] == vs


def test_dlog_without_giant_steps(ctx, table_1000):
    """max_giant = 0: one lane a point, the baby steps alone"""
    vs = [0, 5, -999, 1000, -1000]
    v, found = table_1000.solve(to_arrays([EM.mul(a) for a in vs]), 0)
    assert [int(f) for f in found] == [1, 1, 1, 0, 0] and [int(a) for a in v] == [0, 5, -999, 0, 0]


def test_dlog_table_past_one_tile(ctx):
    """nb = 2^20 + 1000: the build takes a full tile of 2^20 entries and a partial second one.  Baby steps at the end of the first
    tile, at the start and the end of the second, both signs, alone (max_giant = 0) and one giant step away"""
    from vpin_amd import elgamal as E
    nb = 2**20 + 1000
    t = E.DlogTable(ctx, nb)
    assert t.nb == nb and 49 * nb <= t.device_bytes <= 65 * nb
    vs = [2**20 - 1, 2**20, 2**20 + 1, 2**20 + 999, -(2**20 - 1), -(2**20), -(2**20 + 999), 12345]
    pts = to_arrays([EM.mul(v) for v in vs])
    v, found = t.solve(pts, 0)
    assert found.all() and [int(a) for a in v] == vs
    far = [nb + 2**20 + 500, -(nb + 2**20 + 500), 2 * nb - 2, nb + 2**20 - 1, nb, 2 * nb - 1, 2 * nb]
    v, found = t.solve(to_arrays([EM.mul(a) for a in far]), 1)
    assert [int(f) for f in found] == [1] * 6 + [0] and [int(a) for a in v] == far[:6] + [0]
    v, found = t.solve(to_arrays([EM.mul(nb)]), 0)
    assert not found[0]
    t.free()


def test_dlog_tiled_table(ctx, table_64k):
    vs = [65535, 65536, -(3 * 65536 + 1), 2**20 + 3]
    v, found = table_64k.solve(to_arrays([EM.mul(a) for a in vs]), 16)
    assert found.all() and [int(a) for a in v] == vs
    v, found = table_64k.solve(to_arrays([EM.mul(17 * 65536)]), 16)
    assert not found[0] and v[0] == 0


def test_dlog_rejections(ctx, table_1000):
    from vpin_amd import elgamal as E
    einval(lambda: E.DlogTable(ctx, 1), "nb")
    einval(lambda: E.DlogTable(ctx, 2**28 + 1), "nb")
    einval(lambda: table_1000.solve(to_arrays([EM.G]), 2**62 // 1000 + 1), "2\\^62")
    einval(lambda: table_1000.solve(to_arrays([(EM.G[0], EM.G[1] + 1)]), 3), "not on the curve")


# ---- round trips: no model points ---------------------------------------------------------------------------------------

MAX_GIANT = 1 << 14  # with nb = 2^16: +-2^30


def messages(seed, count, bound):
    return [v - bound for v in EM.splitmix_scalars(seed, count, 0, 2 * bound + 1)]


def test_round_trip_300(ctx, base_g, base_h, table_64k):
    from vpin_amd import elgamal as E
    msgs = messages(0x300, 300, 2**30)
    assert min(msgs) < -2**29 and max(msgs) > 2**29
    c1, c2 = E.encrypt(base_g, base_h, msgs, EM.splitmix_scalars(0x301, 300))
    v, found = E.decrypt(table_64k, SK, c1, c2, MAX_GIANT)
    assert found.all() and [int(a) for a in v] == msgs


def test_round_trip_2100(ctx, base_g, base_h, table_64k):
    """past 2048 points the launch gives a point 32 lanes instead of 64"""
    from vpin_amd import elgamal as E
    msgs = messages(0x2100, 2100, 2**30)
    c1, c2 = E.encrypt(base_g, base_h, msgs, EM.splitmix_scalars(0x2101, 2100))
    v, found = E.decrypt(table_64k, SK, c1, c2, MAX_GIANT)
    assert found.all() and [int(a) for a in v] == msgs


def encrypt_image(base_g, base_h, img, seed):
    """an integer array -> the two ciphertext planes, each (x, y, inf) of shape (1,) + img.shape (+ (32,))"""
    from vpin_amd import elgamal as E
    c1, c2 = E.encrypt(base_g, base_h, img, EM.splitmix_scalars(seed, img.size))
    one = lambda t: tuple(a[None] for a in t)
    return one(c1), one(c2)


def decrypt_output(table, tr):
    """the layer's output (c1 planes first, then c2) -> the integers, shape (oh, ow)"""
    from vpin_amd import elgamal as E
    x, y, inf = tr.output()
    assert tr.P == 2
    v, found = E.decrypt(table, SK, (x[0], y[0], inf[0]), (x[1], y[1], inf[1]), 64)
    assert found.all()
    return v


IMAGE = np.array([[(7 * i + 3 * j) % 23 - 5 for j in range(6)] for i in range(6)], dtype=np.int64)
FILTER = np.array([[1, 0, 1], [2, 0, 2], [1, 0, 1]], dtype=np.int64)


def conv_plain(img, filt, pad):
    p = np.pad(img, pad)
    oh, ow = p.shape[0] - filt.shape[0] + 1, p.shape[1] - filt.shape[1] + 1
    return np.array([[int((p[i:i + filt.shape[0], j:j + filt.shape[1]] * filt).sum()) for j in range(ow)] for i in range(oh)], dtype=np.int64)


def pool_plain(img, k, scale):
    return np.array([[scale * int(img[i:i + k, j:j + k].sum()) for j in range(0, img.shape[1] - k + 1, k)]
                     for i in range(0, img.shape[0] - k + 1, k)], dtype=np.int64)


def test_conv_layer_decrypts_to_the_convolution(ctx, base_g, base_h, table_64k):
    from vpin_amd import enc_conv as EC
    c1, c2 = encrypt_image(base_g, base_h, IMAGE, 0xC0)
    tr = EC.conv_layer(ctx, c1, c2, FILTER.tolist(), 1, 1, KEYS[:2], 13)
    assert (tr.oh, tr.ow) == (6, 6) and (IMAGE < 0).any()
    assert np.array_equal(decrypt_output(table_64k, tr), conv_plain(IMAGE, FILTER, 1))
    tr.free()


def test_fc_layer_decrypts_to_the_product(ctx, base_g, base_h, table_64k):
    from vpin_amd import elgamal as E
    from vpin_amd import enc_conv as EC
    K, Nn = 5, 3
    xv = np.array([3, -7, 0, 11, -2], dtype=np.int64)
    Wm = np.array([[1 + (3 * k + 5 * j) % 9 for j in range(Nn)] for k in range(K)], dtype=np.int64)
    b = np.array([-40, 0, 17], dtype=np.int64)
    c1, c2 = E.encrypt(base_g, base_h, xv, EM.splitmix_scalars(0xFC1, K))
    b1, b2 = E.encrypt(base_g, base_h, b, EM.splitmix_scalars(0xFC2, Nn))
    tr = EC.fc_layer(ctx, c1, c2, Wm.tolist(), b1, b2, KEYS[:2], 13)
    got = decrypt_output(table_64k, tr)
    assert np.array_equal(got.reshape(-1), xv @ Wm + b)
    tr.free()


def test_avgpool_layer_decrypts_to_the_scaled_sums(ctx, base_g, base_h, table_64k):
    from vpin_amd import enc_conv as EC
    c1, c2 = encrypt_image(base_g, base_h, IMAGE, 0xA0)
    tr = EC.avgpool_layer(ctx, c1, c2, 2, 2, 3)
    assert (tr.oh, tr.ow) == (3, 3)
    assert np.array_equal(decrypt_output(table_64k, tr), pool_plain(IMAGE, 2, 3))
    tr.free()


def test_chained_layers_with_the_activation_in_between(ctx, base_g, base_h, table_64k):
    """conv -> decrypt -> ReLU (numpy) -> encrypt -> pool -> decrypt, against the plaintext pipeline"""
    from vpin_amd import enc_conv as EC
    c1, c2 = encrypt_image(base_g, base_h, IMAGE, 0xC4)
    tr = EC.conv_layer(ctx, c1, c2, FILTER.tolist(), 1, 1, KEYS[:2], 13)
    mid = decrypt_output(table_64k, tr).copy()
    tr.free()
    plain = conv_plain(IMAGE, FILTER, 1)
    for a in (mid, plain):
        a[1, 2] = -a[1, 2] - 1
        a[4, 0] = -9
    assert (mid < 0).sum() >= 2
    mid, plain = np.maximum(mid, 0), np.maximum(plain, 0)
    c1, c2 = encrypt_image(base_g, base_h, mid, 0xC5)
    tr = EC.avgpool_layer(ctx, c1, c2, 2, 2, 3)
    assert np.array_equal(decrypt_output(table_64k, tr), pool_plain(plain, 2, 3))
    tr.free()


# ---- decryption rejections ----------------------------------------------------------------------------------------------

def test_decrypt_rejections(ctx, base_g, base_h, table_1000):
    from vpin_amd import elgamal as E
    c1, c2 = E.encrypt(base_g, base_h, [5, 6], [11, 12])
    einval(lambda: E.decrypt(table_1000, 0, c1, c2, 3), "zero")
    einval(lambda: E.decrypt(table_1000, N, c1, c2, 3), "group order")
    bad = (c1[0].copy(), c1[1].copy(), c1[2])
    bad[1][1, 0] ^= 1
    einval(lambda: E.decrypt(table_1000, SK, bad, c2, 3), "c1 point is not on the curve")
    v, found = E.decrypt(table_1000, SK, c1, c2, 3)
    assert found.all() and [int(a) for a in v] == [5, 6]
