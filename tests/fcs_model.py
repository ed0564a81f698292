"""Python model of the two layers a trained model needs beside convmc_model: the fully connected layer over signed weights
(vpin_enc_fc_signed) and the trained convolution with a bias per output channel (vpin_enc_conv2d_mc_bias), and of the driver's two
additions (VPIN_NET_FCS, a CONVMC layer with a bias).  Built on enc_fc_model, convmc_model and net_model by import: the groups
(POINTS, LOGS), the PRF, the unbiased layer and the client are theirs.

Also here: the small trained network of tests/test_gpu_net_trained.py, and the LeNet-5 of the reference's
src/accuracy/train_test_lenet5.py at full size under seeded weights (tools/time_net.py lenet5)."""
import numpy as np

import convmc_model as CM
import enc_conv_model as EM
import enc_fc_model as FM
import lenet_model as LM
import net_model as NM

ShapeError, VerifyError = EM.ShapeError, EM.VerifyError
POINTS, LOGS = EM.POINTS, EM.LOGS
neg = CM.neg


def fc_signed(grp, rows, K, W, N, biases, keys, prf_bytes):
    """enc_fc_model.fc over signed W[k][j] (int32 range): the same dict.  A negative weight adds |w| * (-X[k]); the folded weight
    s_k = pos_k - neg_k is recorded as (|s_k|, S_k) with S_k = -X[k] for s_k < 0"""
    res = dict(out=[], mults=[], adds=[], left=[])
    for X, bias, key in zip(rows, biases, keys):
        assert len(X) == K and len(bias) == N and len(W) == K and all(len(w) == N for w in W)
        assert all(-(1 << 31) <= w < 1 << 31 for row in W for w in row)
        C = []
        for j in range(N):
            acc = grp.identity
            for k in range(K):
                acc = grp.add(acc, grp.mul(abs(W[k][j]), neg(grp, X[k]) if W[k][j] < 0 else X[k]))
            C.append(acc)
        out = []
        for j in range(N):
            if C[j] == grp.identity:
                raise ShapeError(f"C[{j}] is the identity")
            res["adds"].append((C[j], bias[j]))
            out.append(grp.add(C[j], bias[j]))
        r = [FM.prf(key, j, prf_bytes) for j in range(N)]
        left = grp.identity
        for j in range(N):
            left = grp.add(left, grp.mul(r[j], C[j]))
        pos = [sum(r[j] * W[k][j] for j in range(N) if W[k][j] > 0) for k in range(K)]
        neg_ = [sum(r[j] * -W[k][j] for j in range(N) if W[k][j] < 0) for k in range(K)]
        if max(pos + neg_) >= 1 << 128:
            raise ShapeError("a folded weight does not fit 128 bits")
        T = []
        for k in range(K):
            if X[k] == grp.identity:
                raise ShapeError(f"X[{k}] is the identity")
            s = pos[k] - neg_[k]
            S = neg(grp, X[k]) if s < 0 else X[k]
            res["mults"].append((abs(s), S))
            T.append(grp.mul(abs(s), S))
        acc = T[0]
        for k in range(1, K):
            if acc == grp.identity:
                raise ShapeError(f"the accumulator before T_{k} is the identity")
            res["adds"].append((acc, T[k]))
            acc = grp.add(acc, T[k])
        if acc != left:
            raise VerifyError("sum_k |s_k| * S_k != sum_j r_j * C[j]")
        res["out"].append(out)
        res["left"].append(left)
    return res


def layer_bias(grp, planes, C, n_out, H, W, weights, connect, fh, fw, pad, stride, biases, keys, prf_bytes):
    """convmc_model.layer with biases[g * n_out + o] (the identity allowed): out = C + bias, the check over C.  mults and left are
    the unbiased layer's; adds per (g, o): the oh * ow pairs (C[t], bias), then that pair's chain additions"""
    oh, ow = EM.out_dims(H, W, fh, fw, pad, stride)
    rows = CM.connected(connect, n_out, C)
    groups = len(planes) // C
    assert len(biases) == groups * n_out
    conv = CM.conv2d_mc(grp, planes, C, n_out, H, W, weights, connect, fh, fw, pad, stride)
    for q, plane in enumerate(conv):
        for t, v in enumerate(plane):
            if v == grp.identity:
                raise ShapeError(f"C[{t}] of plane {q} is the identity")
    base = CM.layer(grp, planes, C, n_out, H, W, weights, connect, fh, fw, pad, stride, keys, prf_bytes)
    assert base["out"] == conv
    res = dict(out=[[grp.add(v, biases[q]) for v in plane] for q, plane in enumerate(conv)], mults=base["mults"], adds=[], left=base["left"])
    pos = 0
    for q in range(groups * n_out):
        chain = len(rows[q % n_out]) * fh * fw - 1
        res["adds"] += [(v, biases[q]) for v in conv[q]] + base["adds"][pos:pos + chain]
        pos += chain
    assert pos == len(base["adds"])
    return res


def bias_trace_counts(groups, C, n_out, connect, fh, fw, oh, ow):
    m, a = CM.trace_counts(groups, C, n_out, connect, fh, fw)
    return m, a + groups * n_out * oh * ow


# ---- a layer list with "fcs" layers and biased "convmc" layers, over convmc_model's ---------------------------------------
# "fcs": dict(kind="fcs", N, w = K x N signed, bias); a "convmc" layer may carry bias = n_out ints (absent or None: no bias)

def net_counts(cfg):
    """convmc_model.net_counts (which counts "fcs" as "fc"); a biased convolution adds n_out bias r and 2 * n_out * oh * ow additions"""
    res = CM.net_counts(cfg)
    for i, (l, (_, (oC, oH, oW))) in enumerate(zip(cfg["layers"], CM.net_shapes(cfg))):
        if l["kind"] == "convmc" and l.get("bias") is not None:
            m, a = res["layers"][i]
            res["layers"][i] = (m, a + 2 * oC * oH * oW)
            res["bias_r"] += oC
    res["n_add"] = sum(a for _, a in res["layers"])
    return res


def net_plaintext(cfg, image):
    """per round what the client decrypts and what it encrypts again"""
    x = np.array([[[int(v) for v in row] for row in plane] for plane in np.asarray(image).reshape(cfg["C"], cfg["H"], cfg["W"])], dtype=object)
    vs, acts = [], []
    for l in cfg["layers"]:
        if l["kind"] == "convmc":
            x = CM.plain_conv2d_mc(x, l["w"], l["connect"], l["fh"], l["fw"], l["pad"], l["stride"])
            if l.get("bias") is not None:
                x = np.array([p + int(b) for p, b in zip(x, l["bias"])], dtype=object)
        elif l["kind"] == "pool":
            x = np.array([LM._pool(p, l["k"], l["stride"], l["scale"]) for p in x], dtype=object)
        else:
            assert l["kind"] in ("fc", "fcs")
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
    """convmc_model.net_infer_model with the two additions.  biases: per layer that has one, in layer order, (c1 elements, c2
    elements): N each for a fully connected layer, n_out each for a convolution (c1 halves: group 0, c2 halves: group 1)"""
    keys, biases = list(keys), list(biases)
    take = lambda n: [keys.pop(0) for _ in range(n)]
    layers, rnd = [], 0
    for l, ((C, H, W), _) in zip(cfg["layers"], CM.net_shapes(cfg)):
        per = H * W
        planes = [c[p * per:(p + 1) * per] for c in (c1, c2) for p in range(C)]
        if l["kind"] == "convmc":
            args = (grp, planes, C, l["n_out"], H, W, l["w"], l["connect"], l["fh"], l["fw"], l["pad"], l["stride"])
            if l.get("bias") is not None:
                b1, b2 = biases.pop(0)
                res = layer_bias(*args, list(b1) + list(b2), take(2 * l["n_out"]), cfg["prf_bytes"])
            else:
                res = CM.layer(*args, take(2 * l["n_out"]), cfg["prf_bytes"])
        elif l["kind"] == "pool":
            res = FM.avgpool(grp, planes, H, W, l["k"], l["stride"], l["scale"])
        else:
            b1, b2 = biases.pop(0)
            one = fc_signed if l["kind"] == "fcs" else FM.fc
            res = one(grp, [list(c1), list(c2)], C * H * W, l["w"], l["N"], [list(b1), list(b2)], take(2), cfg["prf_bytes"])
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


def folded_fit_signed(w, N, key, prf_bytes):
    """net_model.folded_fit for signed weights: both unsigned sums of every s_k stay below 2^128"""
    r = [EM.prf(key, j, prf_bytes) for j in range(N)]
    return all(max(sum(r[j] * row[j] for j in range(N) if row[j] > 0), sum(r[j] * -row[j] for j in range(N) if row[j] < 0)) < 1 << 128
               for row in w)


def device_config(cfg, giants):
    """a configuration of this module as a vpin_amd.net.Config; giants: max_giant per round"""
    from vpin_amd import net as VN
    out = VN.Config(cfg["C"], cfg["H"], cfg["W"], cfg["prf_bytes"])
    giants = list(giants)
    for l in cfg["layers"]:
        if l["kind"] == "convmc":
            out.convmc(np.array(l["w"], dtype=np.int64).reshape(l["n_out"], -1, l["fh"], l["fw"]), l["connect"], l["pad"], l["stride"],
                       bias=l.get("bias"))
        elif l["kind"] == "pool":
            out.pool(l["k"], l["stride"], l["scale"])
        elif l["kind"] == "fcs":
            out.fcs(l["w"], l["bias"])
        else:
            out.fc(l["w"], l["bias"])
        if l.get("round"):
            r = l["round"]
            out.round(r["relu"], r["shift_bits"], giants.pop(0), r["reencrypt"])
    return out


# ---- the small trained network of tests/test_gpu_net_trained.py ------------------------------------------------------------

def trained_config():
    """convmc_model.lenet_shaped_config with the weights left signed and a bias on both convolutions: CONVMC 1 -> 2 (f 3) with
    bias, pool 2 / 2, CONVMC 2 -> 3 under the table (f 2) with bias, FCS 27 -> 4, FCS 4 -> 3 over the 10 x 10 crop.  The shifts keep
    every round below 2^30 on that image (tests/test_fcs_model.py)"""
    base = CM.lenet_shaped_config()
    fc1 = [CM._signed(0xF1 + k, 4) for k in range(27)]
    fc2 = [CM._signed(0xF2 + k, 3) for k in range(4)]
    rnd = lambda relu, bits, re=True: dict(relu=relu, shift_bits=bits, reencrypt=re)
    L = base["layers"]
    return dict(base, layers=[
        dict(L[0], bias=[1 << 24, -(1 << 25)], round=rnd(1, 28)),
        dict(L[1], round=rnd(0, 17)),
        dict(L[2], bias=[-30000, 0, 55555], round=rnd(1, 20)),
        dict(kind="fcs", N=4, w=fc1, bias=[-700, 1200, 0, 35], round=rnd(1, 21)),
        dict(kind="fcs", N=3, w=fc2, bias=[5, -9, 100], round=rnd(0, 0, False))])


trained_image = CM.lenet_shaped_image


# ---- LeNet-5 at full size under seeded weights ---------------------------------------------------------------------------------

LENET5_SHIFTS = (27, 17, 22, 18, 24, 22, 0)  # after conv1, pool1, conv2, pool2, fc, fc1, fc2: shifting(v, b) is v * 2^(16 - b)
LENET5_RELU = (1, 0, 1, 0, 1, 1, 0)


def lenet5_weights():
    """seeded signed weights |w| < 2^4 and biases in the shapes net.lenet5_config takes (a chain's first weight is non-zero)"""
    conv1 = [[CM._signed(0x5A00 + o, 25)] for o in range(6)]
    conv2 = [[CM._signed(0x5B00 + 6 * o + c, 25) for c in range(6)] for o in range(16)]
    fc = [CM._signed(0x5C00 + k, 120) for k in range(400)]
    fc1 = [CM._signed(0x5D00 + k, 84) for k in range(120)]
    fc2 = [CM._signed(0x5E00 + k, 10) for k in range(84)]
    bias = lambda seed, n, bound: CM._signed(seed, n, bound)
    return dict(conv1=conv1, b1=bias(0x5A99, 6, 1 << 24), conv2=conv2, b2=bias(0x5B99, 16, 1 << 16), fc=fc, bfc=bias(0x5C99, 120, 1 << 16),
                fc1=fc1, bfc1=bias(0x5D99, 84, 1 << 14), fc2=fc2, bfc2=bias(0x5E99, 10, 1 << 14))


def lenet5_model_config(w=None):
    """the model's layer list of train_test_lenet5.py's architecture over the 32 x 32 image: what net.lenet5_config builds"""
    w = w or lenet5_weights()
    rnd = lambda i: dict(relu=LENET5_RELU[i], shift_bits=LENET5_SHIFTS[i], reencrypt=i < 6)
    conv = lambda key, b, n_out, i: dict(kind="convmc", n_out=n_out, fh=5, fw=5, pad=0, stride=1, w=w[key], connect=None, bias=w[b], round=rnd(i))
    pool = lambda i: dict(kind="pool", k=2, stride=2, scale=1, round=rnd(i))
    fcs = lambda key, b, i: dict(kind="fcs", N=len(w[b]), w=w[key], bias=w[b], round=rnd(i))
    return dict(C=1, H=32, W=32, prf_bytes=13, layers=[conv("conv1", "b1", 6, 0), pool(1), conv("conv2", "b2", 16, 2), pool(3),
                                                       fcs("fc", "bfc", 4), fcs("fc1", "bfc1", 5), fcs("fc2", "bfc2", 6)])


def lenet5_device_config(giants, w=None):
    """the same network through vpin_amd.net.lenet5_config"""
    from vpin_amd import net as VN
    w = w or lenet5_weights()
    rounds = [dict(relu=LENET5_RELU[i], shift_bits=LENET5_SHIFTS[i], max_giant=giants[i], reencrypt=i < 6) for i in range(7)]
    a = lambda key, shape: np.array(w[key], dtype=np.int64).reshape(shape)
    return VN.lenet5_config(a("conv1", (6, 1, 5, 5)), w["b1"], a("conv2", (16, 6, 5, 5)), w["b2"], w["fc"], w["bfc"], w["fc1"], w["bfc1"],
                            w["fc2"], w["bfc2"], rounds)
