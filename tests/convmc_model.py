"""Python model of the trained convolution layer (vpin_enc_conv2d_mc): one signed filter per (output channel, input channel), an
optional connection table, and the random-linear-combination check per (group, output channel) with ONE chain over all
(channel, tap) terms -- the reference's myConv2d type 1 with rLCL / rLCR type 0 (src/LeNet/Server.py), generalised from its one
non-negative filter.  Built over enc_conv_model's groups (POINTS: affine points of E2; LOGS: discrete logarithms to the base G,
where every expected point is one multiplication of G by a sum mod the order) and its PRF.  With C = n_out = 1 and non-negative
weights it is enc_conv_model.layer, which tests/test_convmc_model.py pins to the reference's recorded run.

Also here: the plaintext integer convolution, and a layer-list network with "convmc" layers on top of net_model (its plaintext
rounds, its loop over the layers' models, its counts)."""
import numpy as np

import enc_conv_model as EM
import enc_fc_model as FM
import gadgets_model as GM
import lenet_model as LM
import net_model as NM

ShapeError, VerifyError = EM.ShapeError, EM.VerifyError
POINTS, LOGS = EM.POINTS, EM.LOGS


def neg(grp, v):
    """-v: (x, q - y) for a point, the negative mod the order for a logarithm; the identity stays"""
    if v == grp.identity:
        return v
    return (v[0], (GM.Q - v[1]) % GM.Q) if grp is POINTS else (-v) % EM.ORDER


def connected(connect, n_out, C):
    """per output channel its connected input channels, ascending (None: all)"""
    rows = [[c for c in range(C) if connect is None or connect[o][c]] for o in range(n_out)]
    if not n_out or not C or any(not r for r in rows):
        raise ValueError("n_out or C is zero, or a row of connect selects no channel")
    return rows


def conv2d_mc(grp, planes, C, n_out, H, W, weights, connect, fh, fw, pad, stride):
    """planes: groups * C lists of H * W elements, group-major; weights[o][c] = fh * fw signed ints row-major.  Returns the
    groups * n_out output planes, group-major.  Weights of unconnected pairs are not read"""
    oh, ow = EM.out_dims(H, W, fh, fw, pad, stride)
    rows = connected(connect, n_out, C)
    out = []
    for g in range(len(planes) // C):
        for o in range(n_out):
            plane = []
            for t in range(oh * ow):
                acc = grp.identity
                for c in rows[o]:
                    win = EM.window(grp, planes[g * C + c], H, W, fh, fw, pad, stride, t // ow, t % ow)
                    for w, x in zip(weights[o][c], win):
                        acc = grp.add(acc, grp.mul(abs(w), neg(grp, x) if w < 0 else x))
                plane.append(acc)
            out.append(plane)
    return out


def layer(grp, planes, C, n_out, H, W, weights, connect, fh, fw, pad, stride, keys, prf_bytes):
    """The layer, literally.  keys: one per (g, o), group-major.  Returns dict(out = groups * n_out planes, mults = [(|w|, S)],
    adds = [(acc, T)] (an identity T is what the witness writes as rz = 1), left = groups * n_out elements)"""
    oh, ow = EM.out_dims(H, W, fh, fw, pad, stride)
    taps = fh * fw
    rows = connected(connect, n_out, C)
    groups = len(planes) // C
    assert groups * C == len(planes) and len(keys) == groups * n_out
    res = dict(out=conv2d_mc(grp, planes, C, n_out, H, W, weights, connect, fh, fw, pad, stride), mults=[], adds=[], left=[])
    for g in range(groups):
        for o in range(n_out):
            out = res["out"][g * n_out + o]
            r = [EM.prf(keys[g * n_out + o], t, prf_bytes) for t in range(oh * ow)]
            left = grp.identity
            for t in range(oh * ow):
                left = grp.add(left, grp.mul(r[t], out[t]))
            acc, first = grp.identity, True
            for c in rows[o]:
                Bp = [grp.identity] * taps
                for t in range(oh * ow):
                    win = EM.window(grp, planes[g * C + c], H, W, fh, fw, pad, stride, t // ow, t % ow)
                    for k in range(taps):
                        Bp[k] = grp.add(Bp[k], grp.mul(r[t], win[k]))
                for k in range(taps):
                    w = weights[o][c][k]
                    if Bp[k] == grp.identity:
                        raise ShapeError(f"B'[{c}][{k}] is the identity")
                    S = neg(grp, Bp[k]) if w < 0 else Bp[k]  # the gadget's weights are u128: the sign goes into the point
                    res["mults"].append((abs(w), S))
                    T = grp.mul(abs(w), S)
                    if first:
                        acc, first = T, False
                        continue
                    if acc == grp.identity:
                        raise ShapeError(f"the accumulator before term ({c}, {k}) is the identity")
                    res["adds"].append((acc, T))
                    acc = grp.add(acc, T)
            if acc != left:
                raise VerifyError("sum_m |w_m| * S_m != sum_t r_t * out[t]")
            res["left"].append(left)
    return res


def trace_counts(groups, C, n_out, connect, fh, fw):
    """(multiplications, additions) of the layer's trace"""
    pairs = sum(len(r) for r in connected(connect, n_out, C))
    return groups * fh * fw * pairs, groups * fh * fw * pairs - groups * n_out


def plain_conv2d_mc(x, weights, connect, fh, fw, pad, stride):
    """the plaintext integer convolution: x of shape C x H x W (Python ints) -> n_out x oh x ow"""
    x = np.asarray(x, dtype=object)
    C, H, W = x.shape
    rows = connected(connect, len(weights), C)
    xp = np.zeros((C, H + 2 * pad, W + 2 * pad), dtype=object)
    xp[:, pad:pad + H, pad:pad + W] = x
    oh, ow = EM.out_dims(H, W, fh, fw, pad, stride)
    return np.array([[[sum(int(weights[o][c][a * fw + b]) * int(xp[c, i * stride + a, j * stride + b]) for c in rows[o] for a in range(fh)
                           for b in range(fw)) for j in range(ow)] for i in range(oh)] for o in range(len(weights))], dtype=object)


# ---- a layer list with trained convolutions, over net_model ---------------------------------------------------------------
# a "convmc" layer: dict(kind="convmc", n_out, fh, fw, pad, stride, w = [o][c][fh * fw], connect = rows or None, round = ..)

def net_shapes(cfg):
    C, H, W = cfg["C"], cfg["H"], cfg["W"]
    out = []
    for l in cfg["layers"]:
        if l["kind"] == "convmc":
            connected(l["connect"], l["n_out"], C)
            o = (l["n_out"],) + EM.out_dims(H, W, l["fh"], l["fw"], l["pad"], l["stride"])
        else:
            o = NM.shapes(dict(C=C, H=H, W=W, layers=[l]))[0][1]
        out.append(((C, H, W), o))
        C, H, W = o
    return out


def net_counts(cfg):
    """net_model.counts with the trained convolution: 2 * f^2 * pairs multiplications, as many additions less 2 * n_out, 2 * n_out keys"""
    layers, dec, keys, bias_r, enc = [], [], 0, 0, cfg["C"] * cfg["H"] * cfg["W"]
    for l, ((C, H, W), (oC, oH, oW)) in zip(cfg["layers"], net_shapes(cfg)):
        if l["kind"] == "convmc":
            layers.append(trace_counts(2, C, l["n_out"], l["connect"], l["fh"], l["fw"]))
            keys += 2 * l["n_out"]
        else:
            one = NM.counts(dict(C=C, H=H, W=W, layers=[dict(l, round=None)]))
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
    """net_model.plaintext with the trained convolution: per round what the client decrypts and what it encrypts again"""
    x = np.array([[[int(v) for v in row] for row in plane] for plane in np.asarray(image).reshape(cfg["C"], cfg["H"], cfg["W"])], dtype=object)
    vs, acts = [], []
    for l in cfg["layers"]:
        if l["kind"] == "convmc":
            x = plain_conv2d_mc(x, l["w"], l["connect"], l["fh"], l["fw"], l["pad"], l["stride"])
        elif l["kind"] == "pool":
            x = np.array([LM._pool(p, l["k"], l["stride"], l["scale"]) for p in x], dtype=object)
        else:
            assert l["kind"] == "fc"
            flat = [int(v) for v in x.reshape(-1)]
            assert len(flat) == len(l["w"])
            x = np.array([[[sum(flat[i] * l["w"][i][j] for i in range(len(flat))) + l["bias"][j] for j in range(l["N"])]]], dtype=object)
        if l.get("round"):
            a = LM._act(x, l["round"]["relu"], l["round"]["shift_bits"])
            vs.append([int(v) for v in x.reshape(-1)])
            acts.append([int(v) for v in a.reshape(-1)])
            x = a
    return vs, acts


def net_infer_model(grp, cfg, c1, c2, keys, biases, client):
    """net_model.infer_model with the trained convolution: groups = 2, the C c1 planes and then the C c2 planes, 2 * n_out keys"""
    keys, biases = list(keys), list(biases)
    take = lambda n: [keys.pop(0) for _ in range(n)]
    layers, rnd = [], 0
    for l, ((C, H, W), _) in zip(cfg["layers"], net_shapes(cfg)):
        per = H * W
        planes = [c[p * per:(p + 1) * per] for c in (c1, c2) for p in range(C)]
        if l["kind"] == "convmc":
            res = layer(grp, planes, C, l["n_out"], H, W, l["w"], l["connect"], l["fh"], l["fw"], l["pad"], l["stride"], take(2 * l["n_out"]),
                        cfg["prf_bytes"])
        elif l["kind"] == "pool":
            res = FM.avgpool(grp, planes, H, W, l["k"], l["stride"], l["scale"])
        else:
            b1, b2 = biases.pop(0)
            res = FM.fc(grp, [list(c1), list(c2)], C * H * W, l["w"], l["N"], [list(b1), list(b2)], take(2), cfg["prf_bytes"])
        layers.append(res)
        half = len(res["out"]) // 2
        c1 = [v for plane in res["out"][:half] for v in plane]
        c2 = [v for plane in res["out"][half:] for v in plane]
        if l.get("round"):
            r = l["round"]
            ans = client(rnd, r["relu"], r["shift_bits"], r["reencrypt"], c1, c2)
            rnd += 1
            if r["reencrypt"]:
                c1, c2 = ans
    assert not keys and not biases
    label = dict(mults=[m for res in layers for m in res.get("mults", [])], adds=[a for res in layers for a in res["adds"]], result=(c1, c2))
    return layers, label


# ---- the LeNet-5-shaped network of tests/test_gpu_net_convmc.py -------------------------------------------------------------

def _signed(seed, n, bound=16):
    """n signed pseudo-random ints with |w| < bound (splitmix64), the first one non-zero: a zero first weight of a chain is VPIN_ESHAPE"""
    out, st = [], seed
    for _ in range(n):
        st, v = GM.splitmix64(st)
        out.append(v % (2 * bound - 1) - (bound - 1))
    if out[0] == 0:
        out[0] = 3
    return out


def lenet_shaped_config():
    """CONVMC 1 -> 2 (f 3), pool 2 / 2, CONVMC 2 -> 3 under a connection table (f 2), FC 27 -> 4, FC 4 -> 3 over a 10 x 10 input,
    signed convolution weights |w| < 2^4 (the FC weights are non-negative: vpin_enc_fc's rule), a round after every layer"""
    w1 = [[_signed(0xC1 + o, 9)] for o in range(2)]
    table = [[1, 0], [1, 1], [0, 1]]
    w2 = [[_signed(0xC2 + 2 * o + c, 4) for c in range(2)] for o in range(3)]
    fc1 = [[abs(v) for v in _signed(0xF1 + k, 4)] for k in range(27)]
    fc2 = [[abs(v) for v in _signed(0xF2 + k, 3)] for k in range(4)]
    rnd = lambda relu, bits, re=True: dict(relu=relu, shift_bits=bits, reencrypt=re)
    return dict(C=1, H=10, W=10, prf_bytes=13, layers=[
        dict(kind="convmc", n_out=2, fh=3, fw=3, pad=0, stride=1, w=w1, connect=None, round=rnd(1, 0)),
        dict(kind="pool", k=2, stride=2, scale=1, round=rnd(0, 26)),
        dict(kind="convmc", n_out=3, fh=2, fw=2, pad=0, stride=1, w=w2, connect=table, round=rnd(1, 20)),
        dict(kind="fc", N=4, w=fc1, bias=[-700, 1200, 0, 35], round=rnd(1, 26)),
        dict(kind="fc", N=3, w=fc2, bias=[5, -9, 100], round=rnd(0, 0, False))])


def device_config(cfg, giants):
    """a configuration of this module as a vpin_amd.net.Config; giants: max_giant per round"""
    from vpin_amd import net as VN
    out = VN.Config(cfg["C"], cfg["H"], cfg["W"], cfg["prf_bytes"])
    giants = list(giants)
    for l in cfg["layers"]:
        if l["kind"] == "convmc":
            out.convmc(np.array(l["w"], dtype=np.int64).reshape(l["n_out"], -1, l["fh"], l["fw"]), l["connect"], l["pad"], l["stride"])
        elif l["kind"] == "pool":
            out.pool(l["k"], l["stride"], l["scale"])
        else:
            out.fc(l["w"], l["bias"])
        if l.get("round"):
            r = l["round"]
            out.round(r["relu"], r["shift_bits"], giants.pop(0), r["reencrypt"])
    return out


def lenet_shaped_image():
    """the 10 x 10 crop (rows and columns 11 .. 20) of the reference's preprocessed 32 x 32 image"""
    return NM.reference_image()[11:21, 11:21]
