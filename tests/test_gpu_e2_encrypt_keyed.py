"""GPU tests of the encryption under a key per element (vpin_e2_encrypt_keyed, vpin_amd.elgamal.encrypt_keyed): c2[i] = msg_i * G +
r_i * H[key_of[i]] with r * H by double-and-add over the key's affine coordinates and no table of any H.  The results are canonical
bytes, so the contract is exact: byte for byte vpin_e2_encrypt under a table of the same H, for every element, and the Python
model tests/elgamal_model.py on sampled elements (a model encryption costs three multiplications of 10 to 17 ms).  Public keys
sk * G for sk = 1, a generic value and ORDER - 1; cnt at the edges of the kernels' workgroup of 256; key_of all one key,
alternating, and only the last element under another key; r and msg at the ends of their ranges; one element whose c2 is the
identity.  Then every rejection, each naming its rule, with a good encryption on the same context after it."""
import ctypes as C

import numpy as np
import pytest

import elgamal_model as EM
from test_gpu_enc_conv import point_at

pytestmark = pytest.mark.gpu

N = EM.ORDER
SKS = [1, 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % N, N - 1]
R_EDGES = [1, N - 1, 0x0BADC0FFEE0DDF00D0BADC0FFEE0DDF00D0BADC0FFEE0DDF00D % N]
MSG_EDGES = [0, 1, -1, 2**62 - 1, -(2**62 - 1), 123456789, -987654321012]


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
def pubs(base_g):
    from vpin_amd import elgamal as E
    out = [E.keygen(base_g, sk) for sk in SKS]
    assert out == [EM.keygen(sk) for sk in SKS]
    return out


@pytest.fixture(scope="module")
def tables(ctx, pubs):
    """the reference: a window table of every H, which the keyed form never builds"""
    from vpin_amd import elgamal as E
    out = [E.BaseTable(ctx, H) for H in pubs]
    yield out
    for b in out:
        b.free()


def check(base_g, tables, pubs, key_of, msgs, rs, model_at):
    """the keyed encryption of all elements; byte for byte the table form's under each key where key_of says so; the model at
    the indices model_at"""
    from vpin_amd import elgamal as E
    c1, c2 = E.encrypt_keyed(base_g, pubs, key_of, msgs, rs)
    key_of = np.asarray(key_of)
    seen = np.zeros(len(msgs), dtype=bool)
    for k, table in enumerate(tables):
        at = key_of == k
        if not at.any():
            continue
        t1, t2 = E.encrypt(base_g, table, msgs, rs)
        for got, ref in zip(c1 + c2, t1 + t2):
            assert np.array_equal(got[at], ref[at]), "key %d" % k
        seen |= at
    assert seen.all()
    for i in model_at:
        m1, m2 = EM.encrypt(pubs[key_of[i]], int(msgs[i]), rs[i])
        assert point_at(*c1, i) == m1 and point_at(*c2, i) == m2, "element %d" % i
    return c1, c2


def patterns(cnt):
    return {"one key": [1] * cnt, "alternating": [i % 3 for i in range(cnt)], "the last under another": [2] * (cnt - 1) + [0]}


@pytest.mark.parametrize("pattern", ["one key", "alternating", "the last under another"])
@pytest.mark.parametrize("cnt", [1, 255, 256, 257, 513])
def test_keyed_is_the_table_form_byte_for_byte(base_g, tables, pubs, cnt, pattern):
    key_of = patterns(cnt)[pattern]
    msgs = [int(v) % 2**40 - 2**39 for v in EM.splitmix_scalars(0xE7C + cnt, cnt)]
    rs = EM.splitmix_scalars(0xE7D + cnt, cnt)
    check(base_g, tables, pubs, key_of, msgs, rs, sorted({0, cnt // 2, cnt - 1}))


def test_every_edge_of_r_and_msg_under_every_key(base_g, tables, pubs):
    combos = [(k, r, m) for k in range(3) for r in R_EDGES for m in MSG_EDGES]
    key_of, rs, msgs = ([c[i] for c in combos] for i in range(3))
    model_at = [i for i, (k, r, m) in enumerate(combos) if (r != R_EDGES[2] and abs(m) == 2**62 - 1) or (k, r, m) == (1, R_EDGES[2], 0)]
    assert len(combos) == 63 and len(model_at) == 13
    check(base_g, tables, pubs, key_of, msgs, rs, model_at)


def test_a_c2_that_is_the_identity(base_g, tables, pubs):
    """sk = 1: H = G, so msg * G = -(r * H) for msg = -r; the last addition is complete and flags the identity"""
    key_of, msgs, rs = [1, 0, 0, 2], [-9, -9, 5, -9], [9, 9, 9, 9]
    c1, c2 = check(base_g, tables, pubs, key_of, msgs, rs, [0, 1, 3])
    assert [int(v) for v in c2[2]] == [0, 1, 0, 0] and not c1[2].any()
    assert point_at(*c2, 1) is None and not c2[0][1].any() and not c2[1][1].any()


def test_every_rejection_names_its_rule_and_the_context_goes_on(ctx, base_g, tables, pubs):
    import vpin_amd
    from vpin_amd import capi
    from vpin_amd import elgamal as E

    def good():
        check(base_g, tables, pubs, [0, 1, 2], [7, -8, 9], [3, 4, 5], [1])

    def einval(fn, text):
        with pytest.raises(vpin_amd.VpinError) as e:
            fn()
        assert e.value.code == -1 and text in str(e.value), e.value
        good()

    off_curve = (pubs[1][0], (pubs[1][1] + 1) % EM.Q)
    einval(lambda: E.encrypt_keyed(base_g, pubs, [], [], []), "vpin_e2_encrypt_keyed: cnt must be in 1 .. 2^30 - 1")
    einval(lambda: E.encrypt_keyed(base_g, [], [0], [1], [1]), "vpin_e2_encrypt_keyed: n_pub must be in 1 .. 2^30 - 1")
    einval(lambda: E.encrypt_keyed(base_g, pubs, [0, 2, 3, 4], [1] * 4, [1] * 4), "vpin_e2_encrypt_keyed: key_of[2] = 3 is not below n_pub = 3")
    einval(lambda: E.encrypt_keyed(base_g, [pubs[0], (0, 0), pubs[2]], [0], [1], [1]), "vpin_e2_encrypt_keyed: public key 1 is the identity")
    einval(lambda: E.encrypt_keyed(base_g, [pubs[0], pubs[1], (EM.Q, pubs[2][1])], [0], [1], [1]),
           "vpin_e2_encrypt_keyed: a coordinate is not below q (public key 2)")
    einval(lambda: E.encrypt_keyed(base_g, [pubs[0], off_curve, (EM.Q, 5)], [0], [1], [1]),
           "vpin_e2_encrypt_keyed: a public key is not on the curve E2 (public key 1)")  # the first bad key, with its own rule
    einval(lambda: E.encrypt_keyed(base_g, [pubs[0], off_curve, pubs[2]], [0], [1], [1]),
           "vpin_e2_encrypt_keyed: a public key is not on the curve E2 (public key 1)")
    einval(lambda: E.encrypt_keyed(base_g, pubs, [0, 1], [1, 1], [5, 0]), "vpin_e2_encrypt_keyed: a randomness r is zero")
    einval(lambda: E.encrypt_keyed(base_g, pubs, [0, 1], [1, 1], [N, 5]), "vpin_e2_encrypt_keyed: a randomness r is not below the group order")
    einval(lambda: E.encrypt_keyed(base_g, pubs, [0, 1], [1, 2**62], [5, 5]), "vpin_e2_encrypt_keyed: a message is not in -(2^62) < msg < 2^62")
    einval(lambda: E.encrypt_keyed(base_g, pubs, [0, 1], [-(2**62), 1], [5, 5]), "vpin_e2_encrypt_keyed: a message is not in -(2^62) < msg < 2^62")
    # a null argument, each of the thirteen pointers in turn
    L = capi.lib()
    buf = np.zeros(64, np.uint8)
    one = np.ones(8, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [ctx.h, base_g.h, p(buf), p(buf), 1, p(buf), p(buf), p(one), 1] + [p(buf)] * 6
    for i in [j for j in range(len(args)) if j not in (4, 8)]:
        bad = list(args)
        bad[i] = None
        assert L.vpin_e2_encrypt_keyed(*bad) == -1 and b"vpin_e2_encrypt_keyed: null argument" in L.vpin_last_error(), i
    good()
