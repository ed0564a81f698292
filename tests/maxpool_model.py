"""Python-integer model of the client's round with max pooling (vpin_e2_client_round_pool) and of a network with such a round
(vpin_net_layer's round_pool_k and round_pool_stride).  Built on lenet_model (the activation), elgamal_model, net_model (the client
on logarithms) and residual_model (every layer, the references, the one-call-over-all-images rule) by import; here are the maximum
in front of the activation and the walk that follows the pooled shape.

A layer of this module's lists is a layer of residual_model's whose round may carry maxpool=(k, stride): the client decrypts the
layer's C x H x W output, takes the maximum of every k x k window of every plane, activates and encrypts the C x Ho x Wo maxima.

Also here: the small network of tests/test_gpu_net_maxpool.py over an 8 x 8 crop, and the LeNet-5 shape with max pooling of
tools/time_net.py lenet5max under seeded weights."""
import numpy as np

import convmc_model as CM
import elgamal_model as EL
import fcs_model as TM
import lenet_model as LM
import net_batch_model as BM
import net_model as NM
import residual_model as RM

LOGS = RM.LOGS
FROM_INPUT = RM.FROM_INPUT


# ---- the round ---------------------------------------------------------------------------------------------------------------------

def out_dims(H, W, k, stride):
    """Ho, Wo of k x k windows at `stride` over H x W: a remainder of rows or columns is dropped"""
    assert 0 < k <= min(H, W) and stride > 0
    return (H - k) // stride + 1, (W - k) // stride + 1


def window(planes, H, W, k, stride, o):
    """the input indices of output element o of planes x Ho x Wo, row-major inside the window"""
    Ho, Wo = out_dims(H, W, k, stride)
    p, t = divmod(o, Ho * Wo)
    oy, ox = divmod(t, Wo)
    return [p * H * W + (oy * stride + i) * W + ox * stride + j for i in range(k) for j in range(k)]


def pooled_round(v, planes, H, W, k, stride, relu, bits):
    """act of vpin_e2_client_round_pool on the raw decryptions v (planes * H * W ints): per output the maximum of its window, then
    lenet_model.activate (None where the shifted value does not fit int32)"""
    assert len(v) == planes * H * W
    Ho, Wo = out_dims(H, W, k, stride)
    return [LM.activate(max(v[i] for i in window(planes, H, W, k, stride, o)), relu, bits) for o in range(planes * Ho * Wo)]


def in_a_window(H, W, k, stride, i):
    """is input element i (of any plane) inside some window?  Not in a dropped remainder, nor in a gap of stride > k"""
    Ho, Wo = out_dims(H, W, k, stride)
    y, x = divmod(i % (H * W), W)
    return any(oy * stride <= y < oy * stride + k for oy in range(Ho)) and any(ox * stride <= x < ox * stride + k for ox in range(Wo))


def log_client(sk, rs, rounds_out, pools):
    """net_model.log_client with the client's own pooling schedule: pools[rnd] = (H, W, k, stride), or (0, 0, 0, 0) for a round as
    there.  rounds_out collects per round (v, act), act the pooled values"""
    rs = list(rs)
    order = EL.ORDER

    def client(rnd, relu, bits, reencrypt, c1, c2):
        v = [(b - sk * a) % order for a, b in zip(c1, c2)]
        v = [x - order if x > order // 2 else x for x in v]
        H, W, k, stride = pools[rnd]
        act = pooled_round(v, len(v) // (H * W), H, W, k, stride, relu, bits) if k else [LM.activate(x, relu, bits) for x in v]
        rounds_out.append((v, act))
        if not reencrypt:
            return None
        r = [rs.pop(0) for _ in act]
        return r, [(m + x * sk) % order for m, x in zip(act, r)]

    client.left = rs
    return client


# ---- the walk that follows the pooled shape ------------------------------------------------------------------------------------------

def _pool_of(l):
    return (l.get("round") or {}).get("maxpool")


def net_shapes(cfg):
    """per layer ((C, H, W) in, (C, H, W) the layer call leaves and the round decrypts, (C, H, W) that goes on), input_from and a
    round's pooling followed; ValueError where vpin_net_cfg_counts answers VPIN_EINVAL for the pooling"""
    shape, out = [(cfg["C"], cfg["H"], cfg["W"])], []
    for i, l in enumerate(cfg["layers"]):
        C, H, W = shape[RM.tensor_of(l.get("input_from", 0), i)]
        if l["kind"] == "add":
            if shape[RM.tensor_of(l["skip_from"], i)] != (C, H, W):
                raise ValueError("the operands differ in shape")
            d = (C, H, W)
        else:
            d = CM.net_shapes(dict(C=C, H=H, W=W, layers=[l]))[0][1]
        o = d
        if _pool_of(l):
            k, stride = _pool_of(l)
            if not k or not stride:
                raise ValueError("one of k and stride is zero")
            if k > d[1] or k > d[2]:
                raise ValueError("the window does not fit")
            o = (d[0],) + out_dims(d[1], d[2], k, stride)
        out.append(((C, H, W), d, o))
        shape.append(o)
    return out


def pool_schedule(cfg):
    """per round (H, W, k, stride) of the planes it decrypts; all zero for a round that does not pool"""
    return [((d[1], d[2]) + tuple(_pool_of(l))) if _pool_of(l) else (0, 0, 0, 0)
            for l, (_, d, _) in zip(cfg["layers"], net_shapes(cfg)) if l.get("round")]


def net_counts(cfg):
    """residual_model.net_counts over the shapes that reach the layers: a round decrypts C H W values and encrypts C Ho Wo"""
    layers, dec, keys, bias_r, enc = [], [], 0, 0, cfg["C"] * cfg["H"] * cfg["W"]
    for l, ((C, H, W), d, o) in zip(cfg["layers"], net_shapes(cfg)):
        if l["kind"] == "add":
            layers.append((0, 2 * C * H * W))
        else:
            one = TM.net_counts(dict(cfg, C=C, H=H, W=W, layers=[dict(l, round=None)]))
            layers += one["layers"]
            keys += one["prf_keys"]
            bias_r += one["bias_r"]
        if l.get("round"):
            dec.append(d[0] * d[1] * d[2])
            if l["round"]["reencrypt"]:
                enc += o[0] * o[1] * o[2]
    return dict(layers=layers, n_mult=sum(m for m, _ in layers), n_add=sum(a for _, a in layers), per_round=dec, decryptions=sum(dec),
                encryptions=enc, prf_keys=keys, bias_r=bias_r)


def net_plaintext(cfg, image):
    """per round what the client decrypts and what it encrypts again: the plaintext network, whose pooling is the ELEMENTWISE
    activation followed by the maximum (the order a plaintext model computes in)"""
    x = np.array([[[int(v) for v in row] for row in plane] for plane in np.asarray(image).reshape(cfg["C"], cfg["H"], cfg["W"])], dtype=object)
    tensors, vs, acts = [x], [], []
    for i, l in enumerate(cfg["layers"]):
        x = tensors[RM.tensor_of(l.get("input_from", 0), i)]
        if l["kind"] == "add":
            x = x + tensors[RM.tensor_of(l["skip_from"], i)]
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
            if _pool_of(l):
                k, stride = _pool_of(l)
                Ho, Wo = out_dims(a.shape[1], a.shape[2], k, stride)
                a = np.array([[[max(int(p[oy * stride + ii][ox * stride + jj]) for ii in range(k) for jj in range(k)) for ox in range(Wo)]
                               for oy in range(Ho)] for p in a], dtype=object)
            acts.append([int(v) for v in a.reshape(-1)])
            x = a
        tensors.append(x)
    return vs, acts


def infer_model(grp, cfg, c1, c2, keys, biases, client):
    """residual_model.infer_model where a round may pool: the layer calls are its own, over the shapes net_shapes gives; the client
    (log_client above) answers a pooled round with C Ho Wo elements per image.  Returns (layers, label) as there"""
    B = len(c1)
    keys, biases = [list(k) for k in keys], [list(b) for b in biases]
    tensors, layers, rnd = [(c1, c2)], [], 0
    for i, (l, ((C, H, W), _, _)) in enumerate(zip(cfg["layers"], net_shapes(cfg))):
        c1, c2 = tensors[RM.tensor_of(l.get("input_from", 0), i)]
        if l["kind"] == "add":
            per = H * W
            planes = lambda pair: [c[b][p * per:(p + 1) * per] for b in range(B) for c in pair for p in range(C)]  # [b][half][plane]
            res = RM.add_layer(grp, planes((c1, c2)), planes(tensors[RM.tensor_of(l["skip_from"], i)]))
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
    """stage after stage the r of all images: a round that pools consumes C Ho Wo per image"""
    out, pos = [], 0
    for l, (_, _, (oC, oH, oW)) in zip(cfg["layers"], net_shapes(cfg)):
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
            out.round(r["relu"], r["shift_bits"], giants.pop(0), r["reencrypt"], maxpool=r.get("maxpool"))
    return out


# ---- the small network of tests/test_gpu_net_maxpool.py ----------------------------------------------------------------------------

def _rnd(relu, bits, re=True, maxpool=None):
    return dict(relu=relu, shift_bits=bits, reencrypt=re, maxpool=maxpool)


def small_config():
    """1 x 8 x 8: CONVMC 1 -> 2 (3 x 3 pad 1) with a round of ReLU, shifting(., 20) and max pooling (2, 2), which leaves 2 x 4 x 4;
    CONVMC 2 -> 2 (3 x 3 pad 1); an ADD whose skip_from names the POOLED tensor (2 x 4 x 4: with the unpooled shape the ADD's
    comparison fails); FCS 32 -> 3, whose K is only right over the pooled shape"""
    return dict(C=1, H=8, W=8, prf_bytes=13, layers=[
        RM._conv(0x4A00, 2, 1, 3, 1, 1, _rnd(1, 20, maxpool=(2, 2)), bias=[1 << 20, -(1 << 19)]),
        RM._conv(0x4A10, 2, 2, 3, 1, 1, _rnd(0, 20)),
        dict(kind="add", skip_from=1, round=_rnd(1, 0)),
        dict(kind="fcs", N=3, w=[CM._signed(0x4A20 + k, 3) for k in range(32)], bias=[700, -1200, 35], round=_rnd(0, 0, False))])


CROPS = ((12, 12), (8, 15), (15, 7), (6, 17))  # (row, column) of image b's 8 x 8 crop of the reference's 32 x 32 image


def images(B):
    full = NM.reference_image()
    return [[int(v) for v in full[i:i + 8, j:j + 8].reshape(-1)] for i, j in CROPS[:B]]


def inputs(model, B):
    """per image b < B of `model`: image, image_r, keys, bias_r, client_r, all seeded by b"""
    counts = net_counts(model)
    n = model["C"] * model["H"] * model["W"]
    seed = lambda base, b: base + 0x100 * b
    return dict(model=model, counts=counts, images=images(B),
                image_r=[EL.splitmix_scalars(seed(0x4E1, b), n) for b in range(B)],
                bias_r=[EL.splitmix_scalars(seed(0x4E2, b), counts["bias_r"]) for b in range(B)],
                client_r=[EL.splitmix_scalars(seed(0x4E3, b), counts["encryptions"] - n) for b in range(B)],
                keys=[[NM.net_key(700 + 1000 * b + i) for i in range(counts["prf_keys"])] for b in range(B)])


# ---- the LeNet-5 shape with max pooling of tools/time_net.py lenet5max ------------------------------------------------------------

LENET5MAX_SHIFTS = (26, 22, 24, 22, 0)  # fcs_model's, with each pooling's own shift folded into the convolution's: 27 + 17 - 16 - 2, 22 + 18 - 16 - 2


def lenet5max_model_config(w=None):
    """fcs_model.lenet5_model_config under the same seeded weights with both average poolings and their rounds removed and maxpool
    (2, 2) on the rounds behind the two convolutions: CONVMC 1 -> 6 (f 5) + round (ReLU, pool) -> 6 x 14 x 14, CONVMC 6 -> 16 (f 5) +
    round (ReLU, pool) -> 16 x 5 x 5, FCS 400 -> 120, FCS 120 -> 84, FCS 84 -> 10.  An average pooling there is a sum of four and a
    shift by two more bits; the maximum of four needs neither, so the values keep the scale they have in that network"""
    w = w or TM.lenet5_weights()
    s = LENET5MAX_SHIFTS
    conv = lambda key, b, n_out, i: dict(kind="convmc", n_out=n_out, fh=5, fw=5, pad=0, stride=1, w=w[key], connect=None, bias=w[b],
                                         round=_rnd(1, s[i], maxpool=(2, 2)))
    fcs = lambda key, b, i, relu: dict(kind="fcs", N=len(w[b]), w=w[key], bias=w[b], round=_rnd(relu, s[i], i < 4))
    return dict(C=1, H=32, W=32, prf_bytes=13, layers=[conv("conv1", "b1", 6, 0), conv("conv2", "b2", 16, 1), fcs("fc", "bfc", 2, 1),
                                                       fcs("fc1", "bfc1", 3, 1), fcs("fc2", "bfc2", 4, 0)])
