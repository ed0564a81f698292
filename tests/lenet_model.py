"""Python model of what joins the encrypted layers into the LeNet inference of the reference (src/LeNet/Server.py inferenceCNN,
src/LeNet/Client.py main): the channel sums in front of the second and third convolution, the client's activation between two
layers, and a pure-integer plaintext LeNet that says what every round decrypts to.  Python ints and numpy only; the group
arithmetic is enc_conv_model's (POINTS or LOGS).

The client's `shifting(v, bits)` is (float32(v) / 2^bits * 2^16).astype(int32).  Here it is integer arithmetic: v rounded to
nearest-even into 24 bits of mantissa (f32_rn), then the exact scale by 2^(16 - bits) truncated toward zero.  The division and
the product of the reference are exact in float32 (powers of two, no subnormal in reach), so that is the same number;
tests/test_inference_pins.py checks it against numpy and against recorded runs of the reference's function.  It is NOT the
integer shift sign(v) * (|v| >> (bits - 16)) (shift_int): the rounding into float32 comes first and can carry.

The network's constants are not restated here: the filter and the pooling scale are read from tests/golden/layer_pins.json and
the connection table from tests/golden/inference_pins.json, where runs of the reference left them."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


# ---- the client's activation ------------------------------------------------------------------------------------------

def f32_rn(v):
    """the integer v rounded to the nearest float32 (ties to even), as an integer; |v| < 2^127"""
    m = abs(int(v))
    e = m.bit_length() - 24
    if e > 0:
        q, r, half = m >> e, m & ((1 << e) - 1), 1 << (e - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
        m = q << e
    return -m if v < 0 else m


def shifting(v, bits):
    """the reference's shifting of one integer; None where the result does not fit int32 (numpy's is undefined there)"""
    x = f32_rn(v)
    s = 16 - bits
    m = abs(x) << s if s >= 0 else abs(x) >> -s  # truncation toward zero of an exact quotient
    out = -m if x < 0 else m
    return out if -2**31 <= out < 2**31 else None


def shift_int(v, bits):
    """what shifting is not: the integer shift of the magnitude"""
    m = abs(int(v)) >> (bits - 16)
    return -m if v < 0 else m


def activate(v, relu, shift_bits):
    """one element of a client round: ReLU first, then the shifting (shift_bits = 0: none)"""
    a = int(v)
    if relu and a < 0:
        a = 0
    return shifting(a, shift_bits) if shift_bits else a


# ---- the channel sums -------------------------------------------------------------------------------------------------

def plane_sums(grp, planes, connect):
    """planes: n_in lists of H * W group elements; connect[o][j] != 0 selects plane j for output o.  Returns the n_out lists of
    pixel-wise sums (np.sum(.., axis=0) of the selected planes)"""
    out = []
    for row in connect:
        assert len(row) == len(planes) and any(row)
        acc = [grp.identity] * len(planes[0])
        for j, on in enumerate(row):
            if on:
                acc = [grp.add(a, b) for a, b in zip(acc, planes[j])]
        out.append(acc)
    return out


# ---- the client's preprocessing ---------------------------------------------------------------------------------------

def min_max_scaling(images):
    lo, hi = np.min(images), np.max(images)
    return np.clip((images - lo) / (hi - lo), a_min=0.001, a_max=0.9999999)


def fixed_point(values, bits=16):
    """real numbers -> the int32 fixed point the reference encrypts (truncation toward zero)"""
    return (np.asarray(values) * 2**bits).astype(np.int32)


def preprocess(image):
    """the client's image: min-max scaling into (0.001, 0.9999999), then 16 fractional bits"""
    return fixed_point(min_max_scaling(np.asarray(image)))


# ---- the default configuration, read from the fixtures ---------------------------------------------------------------

def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def default_config():
    """the reference's LeNet: what its runs left in the fixtures, and the schedule of its client's main"""
    layer = _json("layer_pins.json")
    conv = next(c for c in layer["conv"] if c["name"] == "conv_lenet_7x6")
    pool = next(c for c in layer["pool"] if c["service"] == "LeNet")
    inf = _json("inference_pins.json")
    table = inf["second_conv"][-1]["connect"]
    assert len(table) == 16 and all(len(r) == 6 for r in table)
    return dict(H=32, W=32, n1=6, n2=16, n3=120, connect=table, f=conv["fh"], filter=[int(w) for w in conv["filter"]],
                pool_k=pool["k"], pool_stride=pool["stride"], pool_scale=int(pool["scale"]),
                # (relu, shift bits) of the rounds R1 .. R7
                rounds=[(1, 0), (0, 26), (1, 0), (0, 26), (1, 26), (1, 33), (1, 0)], N1=84, N2=10)


def counts(cfg):
    """per label the (multiplications, additions) of the witness lists, and what the run consumes"""
    f2 = cfg["f"] ** 2
    o1 = cfg["H"] - cfg["f"] + 1
    p1 = (o1 - cfg["pool_k"]) // cfg["pool_stride"] + 1
    o2 = p1 - cfg["f"] + 1
    p2 = (o2 - cfg["pool_k"]) // cfg["pool_stride"] + 1
    assert p2 == cfg["f"], "the third convolution's output must be 1 x 1"
    n1, n2, n3, N1, N2, kk = cfg["n1"], cfg["n2"], cfg["n3"], cfg["N1"], cfg["N2"], cfg["pool_k"] ** 2 - 1
    labels = [(2 * n1 * f2, 2 * n1 * (f2 - 1)), (0, 2 * n1 * p1 * p1 * kk), (2 * n2 * f2, 2 * n2 * (f2 - 1)), (0, 2 * n2 * p2 * p2 * kk),
              (2 * n3 * f2, 2 * n3 * (f2 - 1)), (2 * n3, 2 * (N1 + n3 - 1)), (2 * N1, 2 * (N2 + N1 - 1))]
    dec = [n1 * o1 * o1, n1 * p1 * p1, n2 * o2 * o2, n2 * p2 * p2, n3, N1, N2]
    return dict(labels=labels, decryptions=sum(dec), per_round=dec, encryptions=cfg["H"] * cfg["W"] + sum(dec[:-1]),
                prf_keys=2 * (n1 + n2 + n3) + 4, bias_r=N1 + N2)


# ---- the plaintext network --------------------------------------------------------------------------------------------

def _conv(plane, filt, f):
    H, W = plane.shape
    return np.array([[sum(int(filt[a * f + b]) * int(plane[i + a, j + b]) for a in range(f) for b in range(f))
                      for j in range(W - f + 1)] for i in range(H - f + 1)], dtype=object)


def _pool(plane, k, stride, scale):
    H, W = plane.shape
    return np.array([[scale * sum(int(plane[i + a, j + b]) for a in range(k) for b in range(k))
                      for j in range(0, W - k + 1, stride)] for i in range(0, H - k + 1, stride)], dtype=object)


def _act(planes, relu, bits):
    out = np.array([activate(v, relu, bits) for v in np.asarray(planes, dtype=object).reshape(-1)], dtype=object)
    assert all(v is not None for v in out), "a shifted value does not fit int32"
    return out.reshape(np.asarray(planes, dtype=object).shape)


def plaintext(cfg, image, w1, b1, w2, b2):
    """image: H x W ints; w1 (n3 x N1), w2 (N1 x N2): non-negative ints; b1, b2: ints.  Returns (v, act): per round R1 .. R7 what
    the client decrypts and what it encrypts again (the last act is the result), as flat lists of Python ints in the order the
    server sends them (plane-major, row-major)"""
    f, filt, rounds = cfg["f"], cfg["filter"], cfg["rounds"]
    k, st, sc = cfg["pool_k"], cfg["pool_stride"], cfg["pool_scale"]
    img = np.array([[int(x) for x in row] for row in np.asarray(image).reshape(cfg["H"], cfg["W"])], dtype=object)
    vs, acts = [], []

    def rnd(v):
        a = _act(v, *rounds[len(vs)])
        vs.append([int(x) for x in np.asarray(v, dtype=object).reshape(-1)])
        acts.append([int(x) for x in a.reshape(-1)])
        return a

    x = rnd(np.array([_conv(img, filt, f) for _ in range(cfg["n1"])], dtype=object))
    x = rnd(np.array([_pool(p, k, st, sc) for p in x], dtype=object))
    sums = [sum(x[j] for j in range(cfg["n1"]) if row[j]) for row in cfg["connect"]]
    x = rnd(np.array([_conv(s, filt, f) for s in sums], dtype=object))
    x = rnd(np.array([_pool(p, k, st, sc) for p in x], dtype=object))
    total = sum(x[j] for j in range(cfg["n2"]))
    c3 = _conv(total, filt, f)
    assert c3.shape == (1, 1)
    x = rnd(np.array([c3[0, 0]] * cfg["n3"], dtype=object))
    for w, b in ((w1, b1), (w2, b2)):
        K, N = len(w), len(w[0])
        assert len(x) == K and len(b) == N
        x = rnd(np.array([sum(int(x[i]) * int(w[i][j]) for i in range(K)) + int(b[j]) for j in range(N)], dtype=object))
    return vs, acts


def reference_model():
    """the reference's image and weights as the integers its two sides work on"""
    load = lambda n: np.load(os.path.join(GOLDEN, n))
    image = preprocess(load("image_mnist_32_32.npy")).reshape(32, 32)
    return (image, fixed_point(load("weight_fc1_120_84.npy")), fixed_point(load("bias_fc1_84.npy")),
            fixed_point(load("weight_fc2_84_10.npy")), fixed_point(load("bias_fc2_10.npy")))


# ---- the server's steps over the layers' models (generic over the group, like enc_conv_model) -------------------------

def first_conv(grp, c1, c2, H, W, kernels, filt, f, keys, prf_bytes):
    """firstConv: every kernel runs the one filter over the c1 image and then over the c2 image, a key per call.  Returns the
    layer dict of enc_conv_model.layer over the planes (k0, c1), (k0, c2), (k1, c1), .."""
    import enc_conv_model as EM
    return EM.layer(grp, [c1, c2] * kernels, H, W, filt, f, f, 0, 1, keys, prf_bytes)


def avg_pool(grp, c1_planes, c2_planes, H, W, k, stride, scale):
    """firstAvgPool / secondAvgPool: per kernel the c1 plane, then the c2 plane"""
    import enc_fc_model as FM
    planes = [p for pair in zip(c1_planes, c2_planes) for p in pair]
    return FM.avgpool(grp, planes, H, W, k, stride, scale)


def summed_conv(grp, c1_planes, c2_planes, H, W, connect, filt, f, keys, prf_bytes):
    """secondConv (connect = the table) and thirdConv (connect = rows of ones): per output the c1 sum through the filter, then
    the c2 sum.  The plane additions themselves enter no list.  Returns (sums, layer dict), both in the order
    (o0, c1), (o0, c2), (o1, c1), .."""
    import enc_conv_model as EM
    s1, s2 = plane_sums(grp, c1_planes, connect), plane_sums(grp, c2_planes, connect)
    sums = [p for pair in zip(s1, s2) for p in pair]
    return sums, EM.layer(grp, sums, H, W, filt, f, f, 0, 1, keys, prf_bytes)


def logs_to_points(logs):
    """log_point for thousands of logs at once: Jacobian sums over enc_fc_model's table of 4-bit windows and ONE inversion
    for all of them (tests/test_inference_pins.py checks a sample against enc_fc_model.base_point)"""
    import enc_fc_model as FM
    import gadgets_model as GM
    q = GM.Q
    FM.base_point(1)
    table = FM._base_table
    jac = []
    for k in logs:
        k %= FM.ORDER
        X = Y = Z = None
        for i in range(64):
            d = (k >> (4 * i)) & 15
            if not d:
                continue
            x2, y2 = table[i][d]
            if Z is None:
                X, Y, Z = x2, y2, 1
                continue
            zz = Z * Z % q
            h, r = (x2 * zz - X) % q, (y2 * zz * Z - Y) % q
            assert h, "the partial sum of the lower windows is below the next entry"
            hh = h * h % q
            hhh, v = h * hh % q, X * hh % q
            X3 = (r * r - hhh - 2 * v) % q
            X, Y, Z = X3, (r * (v - X3) - Y * hhh) % q, Z * h % q
        jac.append((X, Y, Z))
    pre, acc = [], 1
    for p in jac:
        pre.append(acc)
        if p[2] is not None:
            acc = acc * p[2] % q
    inv = pow(acc, -1, q)
    out = [None] * len(jac)
    for i in range(len(jac) - 1, -1, -1):
        X, Y, Z = jac[i]
        if Z is None:
            continue
        zi = inv * pre[i] % q
        inv = inv * Z % q
        zi2 = zi * zi % q
        out[i] = (X * zi2 % q, Y * zi2 * zi % q)
    return out


# ---- the whole loop -------------------------------------------------------------------------------------------------

def infer_model(grp, cfg, prf_bytes, c1, c2, keys, w1, bias1, w2, bias2, client):
    """inferenceCNN over the layers' models.  c1, c2: the image's H * W group elements; keys: one per myConv2d / FCLayer call in
    call order; bias1, bias2: the encrypted bias as (c1 elements, c2 elements); client(round, relu, shift_bits, reencrypt, c1
    planes, c2 planes) -> (c1 planes, c2 planes) is the interaction (planes: lists of lists).  Returns per label L1 .. L7 the
    dict of its layer model (out, mults, adds, left)"""
    import enc_fc_model as FM
    f, filt, rounds = cfg["f"], cfg["filter"], cfg["rounds"]
    k, st, sc = cfg["pool_k"], cfg["pool_stride"], cfg["pool_scale"]
    keys = list(keys)
    take = lambda n: [keys.pop(0) for _ in range(n)]
    labels = []

    def interact(res):
        r = len(labels)
        labels.append(res)
        relu, bits = rounds[r]
        return client(r, relu, bits, r < 6, res["out"][0::2], res["out"][1::2])

    H = cfg["H"]
    o1 = H - f + 1
    p1 = (o1 - k) // st + 1
    o2 = p1 - f + 1
    p2 = (o2 - k) // st + 1
    a1, a2 = interact(first_conv(grp, c1, c2, H, H, cfg["n1"], filt, f, take(2 * cfg["n1"]), prf_bytes))
    a1, a2 = interact(avg_pool(grp, a1, a2, o1, o1, k, st, sc))
    a1, a2 = interact(summed_conv(grp, a1, a2, p1, p1, cfg["connect"], filt, f, take(2 * cfg["n2"]), prf_bytes)[1])
    a1, a2 = interact(avg_pool(grp, a1, a2, o2, o2, k, st, sc))
    a1, a2 = interact(summed_conv(grp, a1, a2, p2, p2, [[1] * cfg["n2"]] * cfg["n3"], filt, f, take(2 * cfg["n3"]), prf_bytes)[1])
    row = lambda planes: [p[0] for p in planes]
    res = FM.fc(grp, [row(a1), row(a2)], cfg["n3"], w1, cfg["N1"], list(bias1), take(2), prf_bytes)
    a1, a2 = interact(dict(res, out=_rows_as_planes(res["out"]), rows=res["out"]))
    res = FM.fc(grp, [row(a1), row(a2)], cfg["N1"], w2, cfg["N2"], list(bias2), take(2), prf_bytes)
    interact(dict(res, out=_rows_as_planes(res["out"]), rows=res["out"]))
    assert not keys
    return labels


def _rows_as_planes(rows):
    """the two output rows of a fully connected layer as the planes (0, c1), (0, c2), (1, c1), .. of one element each"""
    return [[v] for pair in zip(rows[0], rows[1]) for v in pair]
