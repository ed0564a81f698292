"""The model of the addition layer and of a network with tensor references (tests/residual_model.py), checked against itself
without a GPU: the add list against a plain affine addition written out on Python ints, the counts formula against the lists the
driver's model emits, the walk's rejections, and that the small networks of tests/test_gpu_net_residual.py keep every round inside
what a table of 2^16 baby steps with 2^14 giant steps decrypts while every round still carries signal."""
import pytest

import enc_conv_model as EM
import net_model as NM
import residual_model as RM

SK = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EM.ORDER


def test_add_layer_against_a_plain_affine_addition():
    logs_x, logs_r = EM.synthetic_logs(0xADD1, 10), EM.synthetic_logs(0xADD2, 10)
    X = [[EM.log_point(k) for k in logs_x[:5]], [EM.log_point(k) for k in logs_x[5:]]]
    R = [[EM.log_point(k) for k in logs_r[:5]], [EM.log_point(k) for k in logs_r[5:]]]
    R[0][1] = None                              # an identity second operand
    R[0][2] = X[0][2]                           # a doubling
    R[1][4] = (X[1][4][0], EM.GM.Q - X[1][4][1])  # a cancelling pair
    res = RM.add_layer(RM.POINTS, X, R)
    assert res["mults"] == [] and res["left"] == [] and len(res["adds"]) == 10
    assert res["adds"] == [(X[p][t], R[p][t]) for p in range(2) for t in range(5)]
    assert res["out"] == [[RM.affine_add(X[p][t], R[p][t]) for t in range(5)] for p in range(2)]
    assert res["out"][0][1] == X[0][1] and res["out"][1][4] is None and res["out"][0][2] == EM.log_point(2 * logs_x[2])
    # and the same layer on logarithms
    lx, lr = [logs_x[:5], logs_x[5:]], [logs_r[:5], logs_r[5:]]
    assert RM.add_layer(RM.LOGS, lx, lr)["out"] == [[(a + b) % EM.ORDER for a, b in zip(x, r)] for x, r in zip(lx, lr)]


def test_add_layer_refuses_an_identity_first_operand_and_names_every_plane():
    X = [[5, 7], [0, 3], [9, 0]]
    with pytest.raises(RM.ShapeError, match=r"X\[1\]\[0\] is the identity") as e:
        RM.add_layer(RM.LOGS, X, [[1, 1]] * 3)
    assert e.value.planes == [1, 2]


@pytest.mark.parametrize("name", sorted(RM.CONFIGS))
def test_counts_formula_is_what_the_driver_model_emits(name):
    model = RM.CONFIGS[name]()
    d = RM.inputs(model, 1)
    counts = d["counts"]
    c1, c2 = NM.log_encrypt(SK, d["images"][0], d["image_r"][0])
    biases, pos = [], 0
    for l in model["layers"]:
        if l.get("bias") is not None:
            biases.append(NM.log_encrypt(SK, l["bias"], d["bias_r"][0][pos:pos + len(l["bias"])]))
            pos += len(l["bias"])
    seen = []
    client = NM.log_client(SK, d["client_r"][0], seen)
    layers, label = RM.infer_model(RM.LOGS, model, [c1], [c2], d["keys"], [biases], client)
    assert [(len(r.get("mults", [])), len(r["adds"])) for r in layers] == counts["layers"]
    assert (len(label["mults"]), len(label["adds"])) == (counts["n_mult"], counts["n_add"])
    assert [len(v) for v, _ in seen] == counts["per_round"] and not client.left
    for l, (m, a), ((C, H, W), _) in zip(model["layers"], counts["layers"], RM.net_shapes(model)):
        if l["kind"] == "add":
            assert (m, a) == (0, 2 * C * H * W)
    # the rounds are the plaintext network's, inside the client's range, and not all zero
    vs, acts = RM.net_plaintext(model, d["images"][0])
    assert [list(v) for v, _ in seen] == vs and [list(a) for _, a in seen] == acts
    assert all(abs(v) < 1 << 30 for r in vs for v in r) and all(any(a for a in r) for r in acts)


def test_every_image_of_the_batch_tests_stays_in_range():
    for name in ("base",):
        model = RM.CONFIGS[name]()
        for image in RM.images(4):
            vs, acts = RM.net_plaintext(model, image)
            assert all(abs(v) < 1 << 30 for r in vs for v in r) and all(any(a for a in r) for r in acts)


def test_shapes_follow_input_from():
    shapes = RM.net_shapes(RM.projection_config())
    assert [s[0] for s in shapes] == [(1, 6, 6), (2, 3, 3), (1, 6, 6), (2, 3, 3), (2, 3, 3)]
    assert [s[1] for s in shapes] == [(2, 3, 3), (2, 3, 3), (2, 3, 3), (2, 3, 3), (1, 1, 3)]
    blind = RM.projection_config()
    del blind["layers"][2]["input_from"]
    with pytest.raises(ValueError, match="differ in shape"):  # behind layer 1 the projection would see 3 x 3 and leave 2 x 2
        RM.net_shapes(blind)


@pytest.mark.parametrize("edit, text", [
    (lambda L: L[2].update(skip_from=3), "the layer itself or a later one"),
    (lambda L: L[1].update(input_from=2), "the layer itself or a later one"),
    (lambda L: L[1].update(skip_from=1), "only an addition layer"),
    (lambda L: L[2].update(skip_from=0), "has no skip_from"),
    (lambda L: L[2].update(skip_from=2), "the same tensor twice"),
    (lambda L: L[2].update(skip_from=RM.FROM_INPUT), "differ in shape"),
])
def test_the_walk_rejects(edit, text):
    model = RM.base_config()
    edit(model["layers"])
    with pytest.raises(ValueError, match=text):
        RM.net_shapes(model)
