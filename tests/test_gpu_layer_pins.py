"""The encrypted layers and the ElGamal client on the GPU pinned to RUNS of the reference's own Python.

Every case of tests/golden/layer_pins.json (what the reference's service and client computed in the build container,
tests/golden/make_layer_pins.py) goes through vpin_enc_conv2d, vpin_enc_fc, vpin_enc_avgpool2d, vpin_e2_base_mul,
vpin_e2_encrypt and vpin_e2_decrypt with the fixture's keys, PRF width, geometry and scale, and the output planes, the two
operation lists (the rz flags where the reference added the identity included) and the left sides are compared with the
recorded values DIRECTLY -- no Python model stands in between.  tests/test_layer_pins.py checks the models against the same file.

The product deliberately rejects a few inputs the reference computes through (an identity accumulator, an identity B'[k] /
X[k] / C[j]: VPIN_ESHAPE); the fixture's inputs avoid them, and the rejections have their own tests in test_gpu_enc_conv.py
and test_gpu_enc_fc.py."""
import numpy as np
import pytest

from test_gpu_enc_conv import assert_lists, points_of, to_arrays
from test_layer_pins import CONV_NAMES, FC_NAMES, M_BABY, PINS, POOL_NAMES, assert_counts, case, keys_of, lists_of, pt, pts

pytestmark = pytest.mark.gpu


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
def base_h(ctx):
    from vpin_amd import elgamal as E
    b = E.BaseTable(ctx, pt(PINS["client"]["h"]))
    yield b
    b.free()


@pytest.fixture(scope="module")
def table(ctx):
    """the reference's table size: 3 200 000 baby steps, built once"""
    from vpin_amd import elgamal as E
    t = E.DlogTable(ctx, M_BABY)
    yield t
    t.free()


def flat(rows):
    return [v for r in rows for v in r]


def assert_trace(tr, c, mults, adds, left):
    ox, oy, oi = tr.output()
    assert points_of(ox, oy, oi) == flat(pts(o) for o in c["output"]), "output ciphertext"
    assert_lists(tr, mults, adds, left)
    assert [int(v) for v in tr.adds()[4]] == [int(a[1] is None) for a in adds], "rz = 1 exactly where the reference added the identity"


# ---- the layers -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_layer(ctx, name):
    c = case("conv", name)
    mults, adds = lists_of(c)
    P = len(c["planes"])
    x, y, inf = to_arrays(flat(pts(p) for p in c["input"]))
    tr = ctx.enc_conv2d(x, y, inf, P, c["H"], c["W"], c["filter"], c["fh"], c["fw"], c["pad"], c["stride"], keys_of(c),
                        c["prf_bytes"])
    taps = c["fh"] * c["fw"]
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (P, c["oh"], c["ow"], P * taps, P * (taps - 1))
    assert_trace(tr, c, mults, adds, pts(c["left"]))
    tr.free()


@pytest.mark.parametrize("name", FC_NAMES)
def test_fc_layer(ctx, name):
    c = case("fc", name)
    mults, adds = lists_of(c)
    K, N = c["K"], c["N"]
    x, y, inf = to_arrays(flat(pts(r) for r in c["input"]))
    bx, by, binf = to_arrays(flat(pts(b) for b in c["bias_points"]))
    tr = ctx.enc_fc(x, y, inf, 2, K, c["weights"], N, bx, by, binf, keys_of(c), c["prf_bytes"])
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (2, 1, N, 2 * K, 2 * (N + K - 1))
    assert_trace(tr, c, mults, adds, pts(c["left"]))
    tr.free()


@pytest.mark.parametrize("name", POOL_NAMES)
def test_pool_layer(ctx, name):
    c = case("pool", name)
    adds = [(pt(p), pt(r)) for p, r in zip(c["add_p"], c["add_r"])]
    x, y, inf = to_arrays(flat(pts(p) for p in c["input"]))
    tr = ctx.enc_avgpool2d(x, y, inf, 2, c["H"], c["W"], c["k"], c["stride"], c["scale"])
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (2, c["oh"], c["ow"], 0, len(adds))
    assert_trace(tr, c, [], adds, [])
    tr.free()


# ---- the client -----------------------------------------------------------------------------------------------------

def test_keygen_and_encrypt(ctx, base_g, base_h):
    from vpin_amd import elgamal as E
    assert_counts()
    cl = PINS["client"]
    sk = int(cl["sk"], 16)
    assert E.keygen(base_g, sk) == pt(cl["h"])
    assert points_of(*ctx.e2_base_mul(base_g.h, [sk])) == [pt(cl["h"])]
    enc = cl["encrypt"]
    c1, c2 = E.encrypt(base_g, base_h, [e["msg"] for e in enc], [int(e["r"], 16) for e in enc])
    assert points_of(*c1) == [pt(e["c1"]) for e in enc] and points_of(*c2) == [pt(e["c2"]) for e in enc]
    # the ciphertexts the reference's client decrypted, and its encryption of a whole image
    d = cl["decrypt"]
    c1, c2 = E.encrypt(base_g, base_h, d["values"], [int(r, 16) for r in d["r"]])
    assert points_of(*c1) == pts(d["c1"]) and points_of(*c2) == pts(d["c2"])
    c = case("conv", CONV_NAMES[1])  # with the repeated ciphertext and the pair P, -P
    c1, c2 = E.encrypt(base_g, base_h, np.array(c["image"], dtype=np.int64), [int(r, 16) for r in c["r"]])
    assert c["planes"] == ["c1", "c2"]
    assert points_of(*c1) == pts(c["input"][0]) and points_of(*c2) == pts(c["input"][1])


def test_decrypt_with_the_reference_table_size(ctx, table):
    from vpin_amd import elgamal as E
    assert_counts()
    d, sk = PINS["client"]["decrypt"], int(PINS["client"]["sk"], 16)
    assert table.nb == M_BABY == PINS["client"]["m"] and len(d["results"]) == 9
    c1, c2 = to_arrays(pts(d["c1"])), to_arrays(pts(d["c2"]))
    v, found = E.decrypt(table, sk, c1, c2, 6)
    assert found.all() and [int(a) for a in v] == d["results"]
    v, found = E.decrypt(table, sk, c1, c2, 4)
    assert [bool(f) for f in found] == [True] * 8 + [False] and [int(a) for a in v[:8]] == d["results"][:8]
    script = PINS["client"]["table_script"]
    v, found = table.solve(to_arrays([pt(e["point"]) for e in script]), 6)
    assert found.all() and [int(a) for a in v] == [e["result"] for e in script]


def test_chained_conv_then_decrypt(ctx, table):
    """the reference's ciphertext image -> the GPU's convolution layer -> the GPU's decryption = the integers the reference's
    client decrypted from the reference's own layer output (equal to numpy's plain convolution, checked by the generator)"""
    from vpin_amd import elgamal as E
    assert_counts()
    ch = PINS["chained"]
    c = case("conv", ch["conv"])
    x, y, inf = to_arrays(flat(pts(p) for p in c["input"]))
    tr = ctx.enc_conv2d(x, y, inf, 2, c["H"], c["W"], c["filter"], c["fh"], c["fw"], c["pad"], c["stride"], keys_of(c),
                        c["prf_bytes"])
    ox, oy, oi = tr.output()
    v, found = E.decrypt(table, int(PINS["client"]["sk"], 16), (ox[0], oy[0], oi[0]), (ox[1], oy[1], oi[1]), 0)
    assert found.all() and v.shape == (c["oh"], c["ow"]) and v.tolist() == ch["values"]
    tr.free()
