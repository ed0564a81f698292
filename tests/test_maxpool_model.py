"""The model of the client's round with max pooling (tests/maxpool_model.py) against a written-out loop; the identity the feature
rests on, act(max v) == max act(v), at the float32 rounding edges; and the counts formula against the model's own lists.  No GPU."""
import itertools

import pytest

import lenet_model as LM
import maxpool_model as MM
import net_model as NM

SHAPES = [(1, 4, 4, 2, 2), (3, 5, 7, 2, 2), (2, 5, 5, 3, 1), (2, 6, 6, 2, 3), (3, 3, 3, 3, 1), (1, 2, 514, 2, 2), (2, 4, 3, 1, 1)]


def values(seed, n, bound=1 << 29):
    return [(seed * 2654435761 + i * 40503 * 65537 + i * i * 977) % (2 * bound - 1) - (bound - 1) for i in range(n)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("relu,bits", [(0, 0), (1, 0), (0, 26), (1, 20)])
def test_the_model_is_the_written_out_loop(shape, relu, bits):
    planes, H, W, k, stride = shape
    v = values(sum(shape), planes * H * W)
    Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
    exp = []
    for p in range(planes):
        for oy in range(Ho):
            for ox in range(Wo):
                a = None
                for i in range(k):
                    for j in range(k):
                        c = v[p * H * W + (oy * stride + i) * W + (ox * stride + j)]
                        a = c if a is None or c > a else a
                if relu and a < 0:
                    a = 0
                exp.append(LM.shifting(a, bits) if bits else a)
    assert MM.out_dims(H, W, k, stride) == (Ho, Wo) and len(exp) == planes * Ho * Wo
    assert MM.pooled_round(v, planes, H, W, k, stride, relu, bits) == exp
    # an element is in a window exactly when some output's window holds it
    held = {i for o in range(planes * Ho * Wo) for i in MM.window(planes, H, W, k, stride, o)}
    assert held == {i for i in range(planes * H * W) if MM.in_a_window(H, W, k, stride, i)}
    assert all(i // (H * W) == o // (Ho * Wo) for o in range(planes * Ho * Wo) for i in MM.window(planes, H, W, k, stride, o)), "a window never crosses a plane"


def edges():
    """float32 rounding edges with either sign: 2^24 +- 1, 2, 3, ties-to-even neighbours at several exponents, and values whose
    rounding carries into the next power of two"""
    out = []
    for e in (24, 25, 26, 30, 40):
        ulp = 1 << (e - 23)  # the spacing of float32 in [2^e, 2^(e + 1))
        base = 1 << e
        out += [base + d for d in (-3, -2, -1, 0, 1, 2, 3)]
        for q in (0, 1, 2, 3, 7):
            out += [base + q * ulp + ulp // 2 + d for d in (-1, 0, 1)]  # around a tie; q even and odd
        out += [2 * base - ulp // 2 + d for d in (-1, 0, 1)] + [2 * base - 1]  # rounds up into 2^(e + 1)
    return sorted(set(out + [-x for x in out] + [0, 1, -1]))


def test_activation_commutes_with_the_maximum_at_the_float32_edges():
    E = edges()
    assert (1 << 24) + 1 in E and -((1 << 24) + 3) in E
    assert LM.f32_rn((1 << 24) + 1) == 1 << 24 and LM.f32_rn((1 << 24) + 3) == (1 << 24) + 4  # ties to even, both ways
    assert LM.f32_rn((1 << 25) - 1) == 1 << 25  # the carry into the next power of two
    for relu, bits in itertools.product((0, 1), (0, 17, 26, 33, 41)):
        fits = [x for x in E if LM.activate(x, relu, bits) is not None]  # shifting(., 17) takes |x| < 2^32: the tails do not fit int32
        assert len(fits) >= len(E) // 2 and fits == [x for x in E if fits[0] <= x <= fits[-1]]
        act = {x: LM.activate(x, relu, bits) for x in fits}
        # non-decreasing over the sorted edges: the whole claim, pair by pair
        assert all(act[a] <= act[b] for a, b in zip(fits, fits[1:])), (relu, bits)
        for w in itertools.combinations(fits[::3] + fits[1::7], 2):
            assert LM.activate(max(w), relu, bits) == max(act[x] for x in w)
    # windows of four neighbours, as the kernel sees them, through the model of the round
    v = E[:len(E) // 4 * 4]
    for relu, bits in ((0, 27), (1, 27), (1, 0), (0, 33)):  # |v| <= 2^41: from 27 bits on every shifted value fits int32
        got = MM.pooled_round(v, 1, 2, len(v) // 2, 2, 2, relu, bits)
        exp = [max(LM.activate(v[i], relu, bits) for i in MM.window(1, 2, len(v) // 2, 2, 2, o)) for o in range(len(v) // 4)]
        assert got == exp


@pytest.mark.parametrize("relu", [0, 1])
def test_all_negative_windows_and_ties(relu):
    v = [-5, -3, -9, -4,
         -(1 << 25) - 1, -(1 << 25) - 2, -(1 << 25) - 3, -(1 << 25) - 5]  # 2 planes of 2 x 2
    for bits in (0, 20):
        got = MM.pooled_round(v, 2, 2, 2, 2, 2, relu, bits)
        assert got == [max(LM.activate(x, relu, bits) for x in v[:4]), max(LM.activate(x, relu, bits) for x in v[4:])]
        assert not relu or got == [0, 0]
    assert MM.pooled_round(v, 2, 2, 2, 2, 2, 0, 0) == [-3, -(1 << 25) - 1]
    ties = [7, 7, 7, 7, -2, -2, -8, -2]
    assert MM.pooled_round(ties, 2, 2, 2, 2, 2, relu, 0) == [7, 0 if relu else -2]
    assert MM.pooled_round(ties, 2, 2, 2, 1, 1, relu, 0) == [LM.activate(x, relu, 0) for x in ties], "k = 1, stride = 1: elementwise"


def test_counts_are_the_models_own_lists():
    """the formula of net_counts against what the model on logarithms does: the lists' lengths, per round what the client sees"""
    model = MM.small_config()
    d = MM.inputs(model, 1)
    counts = d["counts"]
    shapes = MM.net_shapes(model)
    assert [s[1:] for s in shapes] == [((2, 8, 8), (2, 4, 4)), ((2, 4, 4), (2, 4, 4)), ((2, 4, 4), (2, 4, 4)), ((1, 1, 3), (1, 1, 3))]
    assert counts["per_round"] == [128, 32, 32, 3] and counts["encryptions"] == 64 + 32 + 32 + 32
    assert MM.pool_schedule(model) == [(8, 8, 2, 2), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    sk = 0x1234567 % NM.EM.ORDER
    c1, c2 = NM.log_encrypt(sk, d["images"][0], d["image_r"][0])
    biases, pos = [], 0
    for l in model["layers"]:
        if l.get("bias") is not None:
            biases.append(NM.log_encrypt(sk, l["bias"], d["bias_r"][0][pos:pos + len(l["bias"])]))
            pos += len(l["bias"])
    seen = []
    client = MM.log_client(sk, d["client_r"][0], seen, MM.pool_schedule(model))
    layers, label = MM.infer_model(MM.LOGS, model, [c1], [c2], [d["keys"][0]], [biases], client)
    assert client.left == [], "the client's queue is what the counts say"
    assert [(len(res.get("mults", [])), len(res["adds"])) for res in layers] == counts["layers"]
    assert (len(label["mults"]), len(label["adds"])) == (counts["n_mult"], counts["n_add"])
    assert [len(v) for v, _ in seen] == counts["per_round"] and [len(a) for _, a in seen] == [32, 32, 32, 3]
    vs, acts = MM.net_plaintext(model, d["images"][0])
    assert [list(v) for v, _ in seen] == vs and [list(a) for _, a in seen] == acts, "activate-then-max (plaintext) is max-then-activate (the client)"
    assert max(abs(x) for v in vs for x in v) < 1 << 30, "inside the range of the GPU test's table"
    assert any(x < 0 for x in vs[0]) and len(set(acts[0])) > 8


def test_shape_errors_of_the_model():
    bad = MM.small_config()
    bad["layers"][0]["round"]["maxpool"] = (9, 1)
    with pytest.raises(ValueError, match="does not fit"):
        MM.net_shapes(bad)
    unpooled = MM.small_config()
    unpooled["layers"][0]["round"]["maxpool"] = None
    with pytest.raises(ValueError, match="K does not match"):  # FCS 32 -> 3 over 2 x 8 x 8: K is only right over the pooled shape
        MM.net_counts(unpooled)
