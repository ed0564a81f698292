"""Python-integer model of the addition layer (vpin_enc_add) and of a network whose layers name the tensors they read
(vpin_net_layer's input_from and skip_from, VPIN_NET_ADD): a skip connection.  Built on convmc_model, fcs_model, elgamal_model and
net_batch_model by import: the groups (POINTS, LOGS), the other layers' models, the one-call-over-all-images rule and the client
are theirs; here are the addition, the references and the walk that follows them.

A layer of this module's lists is a layer of fcs_model's with two optional keys, input_from and skip_from, spelt as the C ABI
spells them: 0 the default, k the output of layer k - 1 (after its round), FROM_INPUT the encrypted input; and the kind "add":
dict(kind="add", skip_from=.., round=..).

Also here: the small residual networks of tests/test_gpu_net_residual.py over a 6 x 6 crop, and the residual network of
tools/time_net.py resnet over 1 x 32 x 32 under seeded weights."""
import numpy as np

import convmc_model as CM
import elgamal_model as EL
import enc_conv_model as EM
import fcs_model as TM
import lenet_model as LM
import net_batch_model as BM
import net_model as NM

ShapeError = EM.ShapeError
POINTS, LOGS = EM.POINTS, EM.LOGS
FROM_INPUT = -1  # VPIN_NET_FROM_INPUT, (size_t)-1


# ---- the layer ---------------------------------------------------------------------------------------------------------------------

def add_layer(grp, X, R):
    """vpin_enc_add, literally.  X, R: P planes of H * W group elements each.  Returns dict(out = P planes, adds = [(X[p][t],
    R[p][t])] plane-major then t (an identity R is what the witness writes as rz = 1), mults = [], left = []).  ShapeError, with
    every offending plane in .planes, when an X[p][t] is the identity"""
    assert len(X) == len(R) and all(len(x) == len(r) for x, r in zip(X, R))
    bad = [p for p, x in enumerate(X) if any(v == grp.identity for v in x)]
    if bad:
        t = next(t for t, v in enumerate(X[bad[0]]) if v == grp.identity)
        e = ShapeError(f"the first operand X[{bad[0]}][{t}] is the identity")
        e.planes = bad
        raise e
    return dict(out=[[grp.add(x, r) for x, r in zip(xp, rp)] for xp, rp in zip(X, R)], mults=[],
                adds=[(x, r) for xp, rp in zip(X, R) for x, r in zip(xp, rp)], left=[])


def affine_add(p, q):
    """a plain affine addition on E2 over Python ints, written out here: the chord and the tangent, None the identity"""
    import gadgets_model as GM
    Q, A = GM.Q, GM.E2_A
    if p is None or q is None:
        return q if p is None else p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        lam = (3 * p[0] * p[0] + A) * pow(2 * p[1], Q - 2, Q) % Q
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], Q - 2, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return x, (lam * (p[0] - x) - p[1]) % Q


# ---- the walk that follows the references -----------------------------------------------------------------------------------------

def tensor_of(ref, i):
    """a reference on layer i as a tensor: 0 the encrypted input, t the output of layer t - 1"""
    return 0 if ref == FROM_INPUT else ref if ref else i


def net_shapes(cfg):
    """per layer ((C, H, W) in, (C, H, W) out), input_from followed; ValueError where vpin_net_cfg_counts answers VPIN_EINVAL for a
    reference"""
    shape = [(cfg["C"], cfg["H"], cfg["W"])]
    out = []
    for i, l in enumerate(cfg["layers"]):
        refs = [l.get("input_from", 0)] + ([l["skip_from"]] if l.get("skip_from") else [])
        if any(r != FROM_INPUT and not 0 <= r <= i for r in refs):
            raise ValueError("a reference names the layer itself or a later one")
        if l.get("skip_from") and l["kind"] != "add":
            raise ValueError("only an addition layer takes a skip_from")
        C, H, W = shape[tensor_of(l.get("input_from", 0), i)]
        if l["kind"] == "add":
            if not l.get("skip_from"):
                raise ValueError("an addition layer has no skip_from")
            if tensor_of(l["skip_from"], i) == tensor_of(l.get("input_from", 0), i):
                raise ValueError("the same tensor twice")
            if shape[tensor_of(l["skip_from"], i)] != (C, H, W):
                raise ValueError("the operands differ in shape")
            o = (C, H, W)
        else:
            o = CM.net_shapes(dict(C=C, H=H, W=W, layers=[l]))[0][1]
        out.append(((C, H, W), o))
        shape.append(o)
    return out


def net_counts(cfg):
    """fcs_model.net_counts layer by layer over the shapes that reach them; an addition layer: no multiplication, 2 C H W additions,
    no keys, no bias r"""
    layers, dec, keys, bias_r, enc = [], [], 0, 0, cfg["C"] * cfg["H"] * cfg["W"]
    for l, ((C, H, W), (oC, oH, oW)) in zip(cfg["layers"], net_shapes(cfg)):
        if l["kind"] == "add":
            layers.append((0, 2 * C * H * W))
        else:
            one = TM.net_counts(dict(cfg, C=C, H=H, W=W, layers=[dict(l, round=None)]))
            layers += one["layers"]
            keys += one["prf_keys"]
            bias_r += one["bias_r"]
        if l.get("round"):
            dec.append(oC * oH * oW)
            if l["round"]["reencrypt"]:
                enc += oC * oH * oW
    return dict(layers=layers, n_mult=sum(m for m, _ in layers), n_add=sum(a for _, a in layers), per_round=dec, decryptions=sum(dec),
                encryptions=enc, prf_keys=keys, bias_r=bias_r)


def net_plaintext(cfg, image):
    """per round what the client decrypts and what it encrypts again: the plaintext network with its skip connections"""
    x = np.array([[[int(v) for v in row] for row in plane] for plane in np.asarray(image).reshape(cfg["C"], cfg["H"], cfg["W"])], dtype=object)
    tensors, vs, acts = [x], [], []
    for i, l in enumerate(cfg["layers"]):
        x = tensors[tensor_of(l.get("input_from", 0), i)]
        if l["kind"] == "add":
            x = x + tensors[tensor_of(l["skip_from"], i)]
        elif l["kind"] == "convmc":
            x = CM.plain_conv2d_mc(x, l["w"], l["connect"], l["fh"], l["fw"], l["pad"], l["stride"])
            if l.get("bias") is not None:
                x = np.array([p + int(b) for p, b in zip(x, l["bias"])], dtype=object)
        elif l["kind"] == "pool":
            x = np.array([LM._pool(p, l["k"], l["stride"], l["scale"]) for p in x], dtype=object)
        else:
            assert l["kind"] == "fcs"
            flat = [int(v) for v in x.reshape(-1)]
            assert len(flat) == len(l["w"])
            x = np.array([[[sum(flat[k] * l["w"][k][j] for k in range(len(flat))) + l["bias"][j] for j in range(l["N"])]]], dtype=object)
        if l.get("round"):
            a = LM._act(x, l["round"]["relu"], l["round"]["shift_bits"])
            vs.append([int(v) for v in x.reshape(-1)])
            acts.append([int(v) for v in a.reshape(-1)])
            x = a
        tensors.append(x)
    return vs, acts


def infer_model(grp, cfg, c1, c2, keys, biases, client):
    """net_batch_model.infer_batch_model with references: B images in ONE call per layer and ONE round per round.  c1, c2: per image
    its C * H * W elements; keys: per image its keys in the order a single run consumes them; biases: per image, per layer that has
    one, (c1 elements, c2 elements); client: over the values of all images at once.  Every layer other than the addition is
    infer_batch_model's own, over the tensor its input_from names.  Returns (layers, label) as there"""
    B = len(c1)
    keys, biases = [list(k) for k in keys], [list(b) for b in biases]
    tensors, layers, rnd = [(c1, c2)], [], 0
    for i, (l, ((C, H, W), _)) in enumerate(zip(cfg["layers"], net_shapes(cfg))):
        c1, c2 = tensors[tensor_of(l.get("input_from", 0), i)]
        if l["kind"] == "add":
            per = H * W
            planes = lambda pair: [c[b][p * per:(p + 1) * per] for b in range(B) for c in pair for p in range(C)]  # [b][half][plane]
            res = add_layer(grp, planes((c1, c2)), planes(tensors[tensor_of(l["skip_from"], i)]))
        else:
            one = dict(cfg, C=C, H=H, W=W, layers=[{k: v for k, v in l.items() if k != "round"}])
            n_keys = TM.net_counts(one)["prf_keys"]
            has_bias = l["kind"] in ("fc", "fcs") or l.get("bias") is not None
            res = BM.infer_batch_model(grp, one, c1, c2, [[k.pop(0) for _ in range(n_keys)] for k in keys],
                                       [[b.pop(0)] if has_bias else [] for b in biases], None)[0][0]
        layers.append(res)
        planes_out = len(res["out"]) // B
        c1, c2 = [[[v for plane in res["out"][b * planes_out + h * planes_out // 2:b * planes_out + (h + 1) * planes_out // 2] for v in plane]
                   for b in range(B)] for h in range(2)]
        if l.get("round"):
            r = l["round"]
            ans = client(rnd, r["relu"], r["shift_bits"], r["reencrypt"], BM.flat(c1), BM.flat(c2))
            rnd += 1
            if r["reencrypt"]:
                c1, c2 = ([BM.part(a, b, B) for b in range(B)] for a in ans)
        tensors.append((c1, c2))
    assert not any(keys) and not any(biases)
    image_label = lambda b, key: [v for res in layers for v in BM.part(res.get(key, []), b, B)]
    return layers, dict(mults=[m for b in range(B) for m in image_label(b, "mults")], adds=[a for b in range(B) for a in image_label(b, "adds")])


def client_queue(cfg, per_image_rs):
    """net_batch_model.client_queue over the shapes the references give: stage after stage the r of all images"""
    out, pos = [], 0
    for l, (_, (oC, oH, oW)) in zip(cfg["layers"], net_shapes(cfg)):
        if l.get("round") and l["round"]["reencrypt"]:
            for rs in per_image_rs:
                out += rs[pos:pos + oC * oH * oW]
            pos += oC * oH * oW
    assert all(len(rs) == pos for rs in per_image_rs)
    return out


def device_config(cfg, giants):
    """a configuration of this module as a vpin_amd.net.Config; giants: max_giant per round"""
    from vpin_amd import net as VN
    out = VN.Config(cfg["C"], cfg["H"], cfg["W"], cfg["prf_bytes"])
    giants = list(giants)
    ref = lambda r: VN.FROM_INPUT if r == FROM_INPUT else r
    for l in cfg["layers"]:
        src = ref(l.get("input_from", 0))
        if l["kind"] == "add":
            out.add(ref(l["skip_from"]), input_from=src)
        elif l["kind"] == "convmc":
            out.convmc(np.array(l["w"], dtype=np.int64).reshape(l["n_out"], -1, l["fh"], l["fw"]), l["connect"], l["pad"], l["stride"],
                       bias=l.get("bias"), input_from=src)
        elif l["kind"] == "pool":
            out.pool(l["k"], l["stride"], l["scale"], input_from=src)
        else:
            assert l["kind"] == "fcs"
            out.fcs(l["w"], l["bias"], input_from=src)
        if l.get("round"):
            r = l["round"]
            out.round(r["relu"], r["shift_bits"], giants.pop(0), r["reencrypt"])
    return out


# ---- the small residual networks of tests/test_gpu_net_residual.py ---------------------------------------------------------------

def _rnd(relu, bits, re=True):
    return dict(relu=relu, shift_bits=bits, reencrypt=re)


def _conv(seed, n_out, C, f, pad, stride, rnd, bias=None, **more):
    w = [[CM._signed(seed + C * o + c, f * f) for c in range(C)] for o in range(n_out)]
    return dict(kind="convmc", n_out=n_out, fh=f, fw=f, pad=pad, stride=stride, w=w, connect=None, bias=bias, round=rnd, **more)


def _fcs(seed, K, N, bias):
    return dict(kind="fcs", N=N, w=[CM._signed(seed + k, N) for k in range(K)], bias=bias, round=_rnd(0, 0, False))


def base_config():
    """1 x 6 x 6: CONVMC 1 -> 2 (3 x 3 pad 1), CONVMC 2 -> 2 (3 x 3 pad 1), ADD of it and layer 0's output, pool 2 / 2 (no round: its
    output goes straight on), FCS 18 -> 3.  Both operands of the ADD are at 16 fractional bits"""
    return dict(C=1, H=6, W=6, prf_bytes=13, layers=[
        _conv(0x2A00, 2, 1, 3, 1, 1, _rnd(1, 20), bias=[1 << 20, -(1 << 19)]),
        _conv(0x2A10, 2, 2, 3, 1, 1, _rnd(0, 20)),
        dict(kind="add", skip_from=1, round=_rnd(1, 0)),
        dict(kind="pool", k=2, stride=2, scale=1),
        _fcs(0x2A20, 18, 3, [700, -1200, 35])])


def projection_config():
    """the stride-2 block with the 1 x 1 projection: CONVMC 1 -> 2 (stride 2, pad 1) to 2 x 3 x 3, CONVMC 2 -> 2 (pad 1), CONVMC
    1 -> 2 (1 x 1, stride 2) that reads the INPUT through input_from, ADD of the projection and layer 1's output, FCS 18 -> 3.  The
    shapes are only right if input_from is followed: behind layer 1 a 1 x 1 convolution over one channel does not fit"""
    return dict(C=1, H=6, W=6, prf_bytes=13, layers=[
        _conv(0x2B00, 2, 1, 3, 1, 2, _rnd(1, 20)),
        _conv(0x2B10, 2, 2, 3, 1, 1, _rnd(0, 20)),
        _conv(0x2B20, 2, 1, 1, 0, 2, _rnd(0, 19), input_from=FROM_INPUT),
        dict(kind="add", skip_from=2, round=_rnd(1, 0)),
        _fcs(0x2B30, 18, 3, [5, -9, 100])])


def from_input_config():
    """ADD with VPIN_NET_FROM_INPUT: CONVMC 1 -> 1 (3 x 3 pad 1) plus the encrypted input itself, FCS 36 -> 2"""
    return dict(C=1, H=6, W=6, prf_bytes=13, layers=[
        _conv(0x2C00, 1, 1, 3, 1, 1, _rnd(0, 20)),
        dict(kind="add", skip_from=FROM_INPUT, round=_rnd(1, 0)),
        _fcs(0x2C10, 36, 2, [1, -1])])


def twice_config():
    """a tensor referenced twice, and kept across a layer that does not read it: layer 0's output is the skip of the first ADD and,
    two layers later, of the second, whose first operand is named by input_from"""
    return dict(C=1, H=6, W=6, prf_bytes=13, layers=[
        _conv(0x2D00, 2, 1, 3, 1, 1, _rnd(1, 20)),
        _conv(0x2D10, 2, 2, 3, 1, 1, _rnd(0, 20)),
        dict(kind="add", skip_from=1, round=_rnd(1, 0)),
        _conv(0x2D20, 2, 2, 3, 1, 1, _rnd(0, 20)),
        dict(kind="add", input_from=4, skip_from=1, round=_rnd(1, 0)),
        dict(kind="pool", k=2, stride=2, scale=1),
        _fcs(0x2D30, 18, 3, [0, 4, -4])])


CONFIGS = dict(base=base_config, projection=projection_config, from_input=from_input_config, twice=twice_config)
CROPS = ((13, 13), (9, 15), (15, 8), (7, 17))  # (row, column) of image b's 6 x 6 crop of the reference's 32 x 32 image


def images(B):
    full = NM.reference_image()
    return [[int(v) for v in full[i:i + 6, j:j + 6].reshape(-1)] for i, j in CROPS[:B]]


def inputs(model, B):
    """per image b < B of `model`: image, image_r, keys, bias_r, client_r, all seeded by b"""
    counts = net_counts(model)
    n = model["C"] * model["H"] * model["W"]
    seed = lambda base, b: base + 0x100 * b
    return dict(model=model, counts=counts, images=images(B),
                image_r=[EL.splitmix_scalars(seed(0x2E1, b), n) for b in range(B)],
                bias_r=[EL.splitmix_scalars(seed(0x2E2, b), counts["bias_r"]) for b in range(B)],
                client_r=[EL.splitmix_scalars(seed(0x2E3, b), counts["encryptions"] - n) for b in range(B)],
                keys=[[NM.net_key(500 + 1000 * b + i) for i in range(counts["prf_keys"])] for b in range(B)])


# ---- the residual network of tools/time_net.py resnet -----------------------------------------------------------------------------

RESNET_SHIFTS = dict(stem=21, conv=22, proj=21, pool=24)  # back to about 16 fractional bits after every weighted layer
RESNET_ROUNDS = 10


def resnet_model_config():
    """1 x 32 x 32 under seeded signed weights |w| < 2^4: CONVMC 1 -> 8 (3 x 3 pad 1); a block 8 -> 8; a block 8 -> 16 at stride 2
    with the 1 x 1 projection; pooling over the whole 16 x 16 plane; FCS 16 -> 10.  A block is what Config.residual_block appends:
    CONVMC 3 x 3 and its round with ReLU, CONVMC 3 x 3 and its round without, the projection (reading the block's input) where there
    is one, the ADD and its round with ReLU"""
    s = RESNET_SHIFTS
    bias = lambda seed, n: CM._signed(seed, n, 1 << 16)
    return dict(C=1, H=32, W=32, prf_bytes=13, layers=[
        _conv(0x3A00, 8, 1, 3, 1, 1, _rnd(1, s["stem"]), bias=bias(0x3A99, 8)),
        _conv(0x3B00, 8, 8, 3, 1, 1, _rnd(1, s["conv"]), bias=bias(0x3B99, 8)),
        _conv(0x3C00, 8, 8, 3, 1, 1, _rnd(0, s["conv"]), bias=bias(0x3C99, 8)),
        dict(kind="add", skip_from=1, round=_rnd(1, 0)),
        _conv(0x3D00, 16, 8, 3, 1, 2, _rnd(1, s["conv"]), bias=bias(0x3D99, 16)),
        _conv(0x3E00, 16, 16, 3, 1, 1, _rnd(0, s["conv"]), bias=bias(0x3E99, 16)),
        _conv(0x3F00, 16, 8, 1, 0, 2, _rnd(0, s["proj"]), input_from=4),
        dict(kind="add", skip_from=6, round=_rnd(1, 0)),
        dict(kind="pool", k=16, stride=16, scale=1, round=_rnd(0, s["pool"])),
        dict(kind="fcs", N=10, w=[CM._signed(0x3F80 + k, 10) for k in range(16)], bias=CM._signed(0x3F99, 10, 1 << 14), round=_rnd(0, 0, False))])


def resnet_device_config(giants, model=None):
    """the same network through vpin_amd.net.Config.residual_block; giants: max_giant for its ten rounds"""
    from vpin_amd import net as VN
    L = (model or resnet_model_config())["layers"]
    w = lambda l: np.array(l["w"], dtype=np.int64).reshape(l["n_out"], -1, l["fh"], l["fw"])
    g = list(giants)
    rnd = lambda l: dict(shift_bits=l["round"]["shift_bits"], max_giant=g.pop(0))
    cfg = VN.Config(1, 32, 32, 13)
    cfg.convmc(w(L[0]), pad=1, bias=L[0]["bias"]).round(relu=True, **rnd(L[0]))
    cfg.residual_block(w(L[1]), L[1]["bias"], w(L[2]), L[2]["bias"], [rnd(L[1]), rnd(L[2]), rnd(L[3])])
    cfg.residual_block(w(L[4]), L[4]["bias"], w(L[5]), L[5]["bias"], [rnd(L[4]), rnd(L[5]), rnd(L[6]), rnd(L[7])], stride=2, proj=w(L[6]))
    cfg.pool(16, 16, 1).round(**rnd(L[8]))
    cfg.fcs(L[9]["w"], L[9]["bias"]).round(reencrypt=False, max_giant=g.pop(0))
    assert not g
    return cfg
