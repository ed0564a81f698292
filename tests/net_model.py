"""Python model of the layer-list inference of the reference's CNN A .. E service (src/cnn_networks/Server.py inferenceCNN,
src/cnn_networks/Client.py main): a pure-integer plaintext network that says what every round decrypts to, the loop over the
layers' models (enc_conv_model.layer, enc_fc_model.avgpool / fc) with the network's one label -- the lists of all layers
concatenated in layer order, what the reference leaves in its four global lists --, and the counts.  The group arithmetic is
enc_conv_model's (POINTS or LOGS); the client's activation is lenet_model's.

The networks' constants are not restated here: the filter, pad, stride, the PRF bytes, the pooling windows and the weight files
of the five versions and the schedule of the rounds are read from tests/golden/net_pins.json, where runs of the reference left
them (tests/golden/make_net_pins.py)."""
import hashlib
import json
import os

import numpy as np

import enc_conv_model as EM
import enc_fc_model as FM
import lenet_model as LM

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
VERSIONS = ("A", "B", "C", "D", "E")


def pins():
    with open(os.path.join(GOLDEN, "net_pins.json")) as f:
        return json.load(f)


def make_config(H, W, conv, pool, pool_scale, prf_bytes, rounds, w1, b1, w2, b2, C=1):
    """the four layers of inferenceCNN with the client's round after each"""
    rnd = lambda i: dict(relu=rounds[i]["relu"], shift_bits=rounds[i]["shift_bits"], reencrypt=i + 1 < len(rounds))
    as_ints = lambda a: [[int(v) for v in row] for row in a]
    return dict(C=C, H=H, W=W, prf_bytes=prf_bytes, layers=[
        dict(kind="conv", fh=conv["fh"], fw=conv["fw"], pad=conv["pad"], stride=conv["stride"], filter=[int(v) for v in conv["filter"]], round=rnd(0)),
        dict(kind="pool", k=pool[0], stride=pool[1], scale=int(pool_scale), round=rnd(1)),
        dict(kind="fc", N=len(b1), w=as_ints(w1), bias=[int(v) for v in b1], round=rnd(2)),
        dict(kind="fc", N=len(b2), w=as_ints(w2), bias=[int(v) for v in b2], round=rnd(3))])


def cnn_config(version):
    """the reference's network `version` (A .. E) on its 32 x 32 image, the weights as 16-bit fixed point"""
    p = pins()
    net, v = p["network"], p["networks"][version]
    load = lambda key: LM.fixed_point(np.load(os.path.join(GOLDEN, v[key])), net["weight_bits"])
    k = v["pool"][0]
    return make_config(net["H"], net["W"], net["conv"], v["pool"], int(2**net["pool_scale_bits"] / k**2), net["prf_bytes"], p["rounds"],
                       load("weight_fc1"), load("bias_fc1"), load("weight_fc2"), load("bias_fc2"))


def pinned_config(case, p=None):
    """the 8 x 8 network of one case of net_pins.json"""
    p = p or pins()
    return make_config(case["H"], case["W"], case["conv"], case["pool"], case["pool_scale"], case["prf_bytes"], p["rounds"], case["w1"],
                       case["b1"], case["w2"], case["b2"])


def reference_image():
    return LM.preprocess(np.load(os.path.join(GOLDEN, "image_mnist_32_32.npy"))).reshape(32, 32)


def shapes(cfg):
    """per layer ((C, H, W) in, (C, H, W) out); raises ValueError where vpin_net_cfg_counts answers VPIN_EINVAL"""
    C, H, W = cfg["C"], cfg["H"], cfg["W"]
    if not (C and H and W):
        raise ValueError("a dimension is zero")
    out = []
    for l in cfg["layers"]:
        if l["kind"] == "conv":
            if not (l["fh"] and l["fw"] and l["stride"]):
                raise ValueError("a dimension is zero")
            if H + 2 * l["pad"] < l["fh"] or W + 2 * l["pad"] < l["fw"]:
                raise ValueError("a window does not fit")
            o = (C,) + EM.out_dims(H, W, l["fh"], l["fw"], l["pad"], l["stride"])
        elif l["kind"] == "pool":
            if not (l["k"] and l["stride"]):
                raise ValueError("a dimension is zero")
            if l["k"] > H or l["k"] > W:
                raise ValueError("a window does not fit")
            o = (C,) + FM.pool_dims(H, W, l["k"], l["stride"])
        else:
            if not l["N"]:
                raise ValueError("a dimension is zero")
            if len(l["w"]) != C * H * W:
                raise ValueError("K does not match")
            o = (1, 1, l["N"])
        out.append(((C, H, W), o))
        C, H, W = o
    return out


def counts(cfg):
    """per layer (multiplications, additions), their totals (the label), per round the decryptions, and what a run consumes"""
    layers, dec, keys, bias_r, enc = [], [], 0, 0, cfg["C"] * cfg["H"] * cfg["W"]
    for l, ((C, H, W), (oC, oH, oW)) in zip(cfg["layers"], shapes(cfg)):
        if l["kind"] == "conv":
            taps = l["fh"] * l["fw"]
            layers.append((2 * C * taps, 2 * C * (taps - 1)))
            keys += 2 * C
        elif l["kind"] == "pool":
            layers.append((0, 2 * C * oH * oW * (l["k"] ** 2 - 1)))
        else:
            K = C * H * W
            layers.append((2 * K, 2 * (l["N"] + K - 1)))
            keys += 2
            bias_r += l["N"]
        if l.get("round"):
            dec.append(oC * oH * oW)
            if l["round"]["reencrypt"]:
                enc += oC * oH * oW
    return dict(layers=layers, n_mult=sum(m for m, _ in layers), n_add=sum(a for _, a in layers), per_round=dec, decryptions=sum(dec),
                encryptions=enc, prf_keys=keys, bias_r=bias_r)


# ---- the plaintext network --------------------------------------------------------------------------------------------

def _conv(plane, l):
    p = np.pad(plane, l["pad"], mode="constant", constant_values=0)
    H, W = p.shape
    fh, fw, st = l["fh"], l["fw"], l["stride"]
    return np.array([[sum(l["filter"][a * fw + b] * int(p[i + a, j + b]) for a in range(fh) for b in range(fw))
                      for j in range(0, W - fw + 1, st)] for i in range(0, H - fh + 1, st)], dtype=object)


def plaintext(cfg, image):
    """image: C x H x W (or H x W) ints.  Returns (v, act): per round what the client decrypts and what it encrypts again (the last
    act is the result), as flat lists of Python ints in the order the server sends them (plane-major, row-major)"""
    x = np.array([[[int(v) for v in row] for row in plane] for plane in np.asarray(image).reshape(cfg["C"], cfg["H"], cfg["W"])], dtype=object)
    vs, acts = [], []
    for l in cfg["layers"]:
        if l["kind"] == "conv":
            x = np.array([_conv(p, l) for p in x], dtype=object)
        elif l["kind"] == "pool":
            x = np.array([LM._pool(p, l["k"], l["stride"], l["scale"]) for p in x], dtype=object)
        else:
            flat = [int(v) for v in x.reshape(-1)]
            assert len(flat) == len(l["w"])
            x = np.array([[[sum(flat[i] * l["w"][i][j] for i in range(len(flat))) + l["bias"][j] for j in range(l["N"])]]], dtype=object)
        if l.get("round"):
            a = LM._act(x, l["round"]["relu"], l["round"]["shift_bits"])
            vs.append([int(v) for v in x.reshape(-1)])
            acts.append([int(v) for v in a.reshape(-1)])
            x = a
    return vs, acts


# ---- the folded weights of a fully connected layer ------------------------------------------------------------------

def folded_fit(w, N, key, prf_bytes):
    """whether every s_k = sum_j r_j * W[k][j] under this row's key fits 128 bits (else vpin_enc_fc answers VPIN_ESHAPE)"""
    r = [EM.prf(key, j, prf_bytes) for j in range(N)]
    return all(sum(r[j] * row[j] for j in range(N)) < 1 << 128 for row in w)


def net_key(i):
    return hashlib.sha256(b"net/key/%d" % i).digest()


def keys_fit(cfg, keys):
    """per fully connected layer whether the folded weights of both rows fit, for keys in call order"""
    out, pos = [], 0
    for l, ((C, H, W), _) in zip(cfg["layers"], shapes(cfg)):
        if l["kind"] == "conv":
            pos += 2 * C
        elif l["kind"] == "fc":
            out.append(all(folded_fit(l["w"], l["N"], keys[pos + i], cfg["prf_bytes"]) for i in range(2)))
            pos += 2
    return out


# ---- the whole loop over the layers' models -----------------------------------------------------------------------------

def infer_model(grp, cfg, c1, c2, keys, biases, client):
    """inferenceCNN over the layers' models.  c1, c2: the input's C * H * W group elements (plane-major); keys: one per
    convolution plane and fully connected row in call order; biases: per fully connected layer the encrypted bias as (c1 elements,
    c2 elements); client(round, relu, shift_bits, reencrypt, c1, c2) -> (c1, c2) is the interaction over flat lists.  Returns
    (layers, label): per layer the dict of its model (out, mults, adds, ..) and the label dict(mults, adds, result = (c1, c2))"""
    keys, biases = list(keys), list(biases)
    take = lambda n: [keys.pop(0) for _ in range(n)]
    layers, rnd = [], 0
    for l, ((C, H, W), (oC, oH, oW)) in zip(cfg["layers"], shapes(cfg)):
        per = H * W
        planes = [c[p * per:(p + 1) * per] for c in (c1, c2) for p in range(C)]
        if l["kind"] == "conv":
            res = EM.layer(grp, planes, H, W, l["filter"], l["fh"], l["fw"], l["pad"], l["stride"], take(2 * C), cfg["prf_bytes"])
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


def log_client(sk, rs, rounds_out):
    """the client on discrete logarithms: a ciphertext (c1, c2) = (r, m + r * sk) mod the order.  rs: the queue of encryption
    randomness (consumed in order); rounds_out collects per round (v, act)"""
    rs = list(rs)
    order = EM.ORDER

    def client(rnd, relu, bits, reencrypt, c1, c2):
        v = [(b - sk * a) % order for a, b in zip(c1, c2)]
        v = [x - order if x > order // 2 else x for x in v]
        act = [LM.activate(x, relu, bits) for x in v]
        rounds_out.append((v, act))
        if not reencrypt:
            return None
        r = [rs.pop(0) for _ in act]
        return r, [(m + x * sk) % order for m, x in zip(act, r)]

    client.left = rs
    return client


def log_encrypt(sk, msgs, rs):
    return [r % EM.ORDER for r in rs], [(int(m) + r * sk) % EM.ORDER for m, r in zip(msgs, rs)]
