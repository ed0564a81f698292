"""GPU parity of the addition layer (vpin_enc_add) with the Python model tests/residual_model.py: outputs, flags, the addition
list, the dims and the NULL views, exactly.  The GPU is fed points k * G from vpin_synthetic_points (negated, copied or flagged
where a case needs it) and the model their discrete logs; expected points come from one batched conversion
(lenet_model.logs_to_points).  Plane sizes 1, 63, 64, 65 and 257 are the lane, wave and workgroup edges of e2_pair_add_kernel (one
wave per workgroup); the degenerate operands sit at elements 0, 63, 64 and the last.  The refusals are ordinary error returns."""
import ctypes as C

import numpy as np
import pytest

import enc_conv_model as EM
import lenet_model as LM
import pool_poison_cases as PP
import residual_model as RM
from test_gpu_enc_conv import points_of
from test_gpu_enc_convmc import negated

pytestmark = pytest.mark.gpu

EINVAL, ESHAPE = -1, -5
SEED_C = bytes(range(64))
SEED_P = bytes((11 * i + 5) % 256 for i in range(64))
SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 257: (257, 1)}  # plane size -> H x W


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


def operands(P, H, W, seed=0xADD0):
    """X and R: P planes of H x W synthetic points each, with their discrete logs -> (x, y, f), (rx, ry, rf), logs_x, logs_r"""
    from vpin_amd import gadgets as G
    n = P * H * W
    out = []
    for s in (seed, seed + 0x1000):
        x, y = G.synthetic_points(s, n)
        out.append([np.array(x, dtype=np.uint8).reshape(n, 32).copy(), np.array(y, dtype=np.uint8).reshape(n, 32).copy(), np.zeros(n, np.uint8)])
    return out[0], out[1], EM.synthetic_logs(seed, n), EM.synthetic_logs(seed + 0x1000, n)


def planes(flat, P):
    n = len(flat) // P
    return [flat[p * n:(p + 1) * n] for p in range(P)]


def null_views(tr):
    """the raw views of the multiplication list and the left sides: all NULL for a trace without them"""
    from vpin_amd import capi
    out = []
    for fn in ("vpin_conv_trace_mults", "vpin_conv_trace_left"):
        ptrs = [C.c_void_p(1) for _ in range(3)]
        assert getattr(capi.lib(), fn)(tr.h, *[C.byref(p) for p in ptrs]) == 0
        out += [p.value for p in ptrs]
    return out


def check(ctx, X, R, lx, lr, P, H, W):
    """the layer on the GPU against the model on logarithms: dims, NULL views, output with flags, the addition list -> the trace"""
    tr = ctx.enc_add(*X, *R, P, H, W)
    exp = RM.add_layer(RM.LOGS, planes(lx, P), planes(lr, P))
    assert (tr.P, tr.oh, tr.ow, tr.n_mult, tr.n_add) == (P, H, W, 0, P * H * W)
    assert null_views(tr) == [None] * 6
    flat = [v for plane in exp["out"] for v in plane] + [a[0] for a in exp["adds"]] + [a[1] for a in exp["adds"]]
    pts = LM.logs_to_points(flat)
    n = P * H * W
    assert points_of(*tr.output()) == pts[:n], "output ciphertext (an identity flagged and written as zeros)"
    px, py, rx, ry, rz = tr.adds()
    assert points_of(px, py) == pts[n:2 * n], "first operands"
    assert points_of(rx, ry, rz) == pts[2 * n:], "second operands (rz = 1 and zeros for the identity)"
    assert [int(v) for v in rz] == [int(l == 0) for l in lr]
    assert ctx.enc_last_refusals() == []
    return tr


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("size", sorted(SHAPES))
def test_parity_at_the_lane_wave_and_workgroup_edges(ctx, size, P):
    H, W = SHAPES[size]
    X, R, lx, lr = operands(P, H, W, 0xADD0 + 16 * size + P)
    check(ctx, X, R, lx, lr, P, H, W).free()
    t = ctx.enc_conv_timings()
    assert t["validate"] > 0 and t["conv"] > 0 and t["host_tail"] > 0 and t["prf"] == 0 and t["rlc"] == 0
    assert t["total"] >= t["validate"] + t["conv"] + t["host_tail"]


EDGES = (0, 63, 64, 256)  # of a plane of 257 elements: lane 0, the last lane of a wave, the first of the next workgroup, the last


@pytest.mark.parametrize("case", ["identity", "double", "cancel"])
def test_degenerate_second_operands_are_cases_of_the_addition(ctx, case):
    """in plane 1 of 2 x 257: R the identity (rz = 1, zero coordinates), R == X (a doubling), R == -X (the flagged identity)"""
    P, H, W = 2, 257, 1
    X, R, lx, lr = operands(P, H, W, 0xADE0)
    for e in EDGES:
        i = 257 + e
        if case == "identity":
            R[0][i], R[1][i], R[2][i], lr[i] = 0, 0, 1, 0
            R[0][i][0], R[1][i][0] = 7, 9  # flagged: its coordinates (7, 9) are no point's, are not read, and are written as zeros
        elif case == "double":
            R[0][i], R[1][i], lr[i] = X[0][i], X[1][i], lx[i]
        else:
            R[0][i], R[1][i], lr[i] = X[0][i], negated(X[1][i]), -lx[i] % EM.ORDER
    tr = check(ctx, X, R, lx, lr, P, H, W)
    ox, oy, oi = tr.output()
    assert [int(oi.reshape(-1)[257 + e]) for e in EDGES] == [int(case == "cancel")] * 4 and int(oi.sum()) == (4 if case == "cancel" else 0)
    if case == "identity":
        for e in EDGES:
            assert np.array_equal(ox.reshape(-1, 32)[257 + e], X[0][257 + e]) and np.array_equal(oy.reshape(-1, 32)[257 + e], X[1][257 + e])
    tr.free()


def test_an_identity_first_operand_is_refused_and_its_planes_are_named(ctx):
    import vpin_amd
    P, H, W = 3, 5, 13
    X, R, lx, lr = operands(P, H, W, 0xADF0)
    for i in (0 * 65 + 64, 2 * 65 + 7, 2 * 65 + 9):  # planes 0 and 2 of three
        X[0][i], X[1][i], X[2][i], lx[i] = 0, 0, 1, 0
    with pytest.raises(RM.ShapeError) as m:
        RM.add_layer(RM.LOGS, planes(lx, P), planes(lr, P))
    assert m.value.planes == [0, 2]
    with pytest.raises(vpin_amd.VpinError) as e:
        ctx.enc_add(*X, *R, P, H, W)
    assert e.value.code == ESHAPE and "vpin_enc_add: the first operand X[0][64] is the identity" in str(e.value), e.value
    assert ctx.enc_last_refusals() == [0, 2]
    check(ctx, [a[65:130] for a in X], [a[65:130] for a in R], lx[65:130], lr[65:130], 1, H, W).free()  # plane 1 alone is fine


@pytest.mark.parametrize("operand, name", [(0, "first operand"), (1, "second operand")])
def test_a_bad_point_is_einval_with_the_operand_named(ctx, operand, name):
    import vpin_amd
    P, H, W = 1, 8, 8
    for what, text in (("range", "vpin_enc_add: a coordinate is not below q"), ("curve", "vpin_enc_add: a %s is not on the curve E2" % name)):
        X, R, _, _ = operands(P, H, W, 0xAE00)
        bad = (EM.GM.Q + 1 if what == "range" else 5).to_bytes(32, "little")
        (X, R)[operand][0][63] = np.frombuffer(bad, dtype=np.uint8)
        with pytest.raises(vpin_amd.VpinError) as e:
            ctx.enc_add(*X, *R, P, H, W)
        assert e.value.code == EINVAL and text in str(e.value), e.value
        assert ctx.enc_last_refusals() == []


def test_bad_arguments(ctx):
    import vpin_amd
    from vpin_amd import capi
    X, R, _, _ = operands(1, 2, 2, 0xAE10)
    for dims, text in (((0, 2, 2), "a dimension is zero"), ((1, 0, 4), "a dimension is zero"), ((1, 4, 0), "a dimension is zero"),
                       ((65536, 1, 1), "planes are more than 65535"), ((1, (1 << 24) + 1, 1), "a dimension is out of range"),
                       ((1, 1, (1 << 24) + 1), "a dimension is out of range")):
        h = C.c_void_p()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = capi.lib().vpin_enc_add(ctx.h, p(X[0]), p(X[1]), p(X[2]), p(R[0]), p(R[1]), p(R[2]), *dims, C.byref(h))
        assert rc == EINVAL and not h.value and text in capi.lib().vpin_last_error().decode(), (dims, capi.lib().vpin_last_error())
    h = C.c_void_p()
    assert capi.lib().vpin_enc_add(ctx.h, None, p(X[1]), p(X[2]), p(R[0]), p(R[1]), p(R[2]), 1, 2, 2, C.byref(h)) == EINVAL
    assert "vpin_enc_add: null argument" in capi.lib().vpin_last_error().decode()


def test_the_add_instance_of_an_honest_trace_is_proven_and_one_doubling_breaks_it(ctx):
    P, H, W = 2, 5, 13
    X, R, lx, lr = operands(P, H, W, 0xAE20)
    tr = check(ctx, X, R, lx, lr, P, H, W)
    gm, ga = tr.instances()
    assert gm is None and ga is not None and ga.is_sat()
    proof = ga.snark_prove(SEED_C, SEED_P)
    assert ctx.snark_verify(dict(inputs=ga.inputs, num_inputs=ga.num_inputs), proof)
    ga.free()
    tr.free()
    i = 65 + 12
    R[0][i], R[1][i], lr[i] = X[0][i], X[1][i], lx[i]  # one R == X row: the layer adds it, the gadget's chord rule does not hold
    tr = check(ctx, X, R, lx, lr, P, H, W)
    gm, ga = tr.instances()
    assert gm is None and not ga.is_sat()
    ga.free()
    tr.free()


def test_add_layer_of_enc_conv_is_the_same_call(ctx):
    from vpin_amd import enc_conv as EC
    P, H, W = 2, 3, 5
    X, R, lx, lr = operands(P, H, W, 0xAE28)
    shaped = lambda t: (t[0].reshape(P, H, W, 32), t[1].reshape(P, H, W, 32), t[2].reshape(P, H, W))
    a, b = EC.add_layer(ctx, shaped(X), (shaped(R)[0], shaped(R)[1], None)), check(ctx, X, R, lx, lr, P, H, W)
    for u, v in zip(list(a.output()) + list(a.adds()), list(b.output()) + list(b.adds())):
        assert np.array_equal(u, v)
    a.free()
    b.free()


def test_the_same_bytes_on_poisoned_pool_blocks(ctx):
    P, H, W = 3, 5, 13
    X, R, lx, lr = operands(P, H, W, 0xAE30)
    R[2][7], lr[7] = 1, 0
    ref = ctx.enc_add(*X, *R, P, H, W)
    for word in PP.WORDS:
        c = PP.poisoned_context(word)
        with PP.filled(c):
            tr = check(c, X, R, lx, lr, P, H, W)
        for u, v in zip(list(tr.output()) + list(tr.adds()), list(ref.output()) + list(ref.adds())):
            assert np.array_equal(u, v)
        tr.free()
        c.close()
    ref.free()
