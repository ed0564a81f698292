#!/usr/bin/env python3
"""Pin the encrypted layers and the ElGamal client to RUNS of the reference's own Python, mechanically.

Run in the build container (the reference does not travel):

    python tests/golden/make_layer_pins.py            # writes tests/golden/layer_pins.json
    python tests/golden/make_layer_pins.py --out F    # writes F instead (tests/test_layer_pins.py compares the bytes)

What it does.  The reference's service and client are plain Python (src/LeNet/Server.py, src/cnn_networks/Server.py,
src/convolution/Server.py, src/LeNet/Client.py, src/Pre_computed_table/baby-step-giant-step.py).  This script loads those
files from the reference tree at run time and calls THEIR functions on small inputs: keyGen, encrypt, encryptFixedPointValue,
encryptBias, callConv2_ciphertext / conv2_ciphertext / myConv2d (type 1, with rLCL / rLCR type 0), FCLayer (flag 1, with
rLCL / rLCR type 1), myAvgPool2d (flag 1, type1 1), pf, decrypt_c1_c2 / giant_step.  It records the inputs, what the functions
returned, what they left in the four global lists (points_mult, weights_array, point_one_Add, point_two_Add), and the values of
two locals caught at the function that produces them (rLCL's return = result_left; realNumbersToFixedPointRepresentation's
return = the pooling scale).  Nothing of the reference is restated here: the filter of LeNet's convolution, the number of PRF
bytes of each service and the pooling scale are all READ OFF the run (weights_array, pf's output against HMAC-SHA256 prefixes,
the caught return value).  The output file holds inputs and recorded outputs only -- no reference text.

What the reference modules need to load and to be deterministic, supplied here:
  * `ecdsa.ellipticcurve` (CurveFp, Point, INFINITY) is not installed: the stand-in below is the affine short-Weierstrass
    group law, written independently of tests/gadgets_model.py (left-to-right double-and-add, Python's modular inverse), and
    self-checked before use (self_check);
  * sys.argv gets port arguments, sys.modules["socket"] a stub, so that loading a module touches no resolver or network;
  * os.urandom hands out the fixture's 32-byte keys in call order (one per myConv2d call on a ciphertext plane, one per
    FCLayer call), random.randrange the fixture's r values and sk; both queues must be empty after a case;
  * the reference's own MultiCoreFeature switch is set to 0 (the eight-process branch computes the same sum); the fixture
    records the setting.

Inputs are chosen to stay clear of what the product rejects on purpose (VPIN_ESHAPE) although the reference computes through
it: an identity accumulator (a zero first tap, a pooling window that starts with the identity or cancels early, an identity
C[j]) and an identity B'[k] / X[k].  Every filter of the reference has a non-zero first tap, every ciphertext here is a
non-identity point, and padding 1 leaves real pixels under every tap.  Those rejections have their own tests
(tests/test_gpu_enc_conv.py, tests/test_gpu_enc_fc.py).

Every point of the fixture is stored once in "points" as [x, y] (64 hex digits each); the lists hold indices into it, null for
the identity.  Field-size integers are hex strings, PRF outputs and folded weights decimal strings.
"""
import contextlib
import hashlib
import hmac
import importlib.util
import io
import json
import operator
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_gadget_pins  # noqa: E402  (the sibling generator knows where the build container keeps the reference tree)

REF = os.environ.get("VPIN_REFERENCE") or make_gadget_pins.REF.split("/src/")[0]
FILES = dict(lenet_server="src/LeNet/Server.py", lenet_client="src/LeNet/Client.py",
             cnn_server="src/cnn_networks/Server.py", conv_server="src/convolution/Server.py",
             bsgs="src/Pre_computed_table/baby-step-giant-step.py")
M_BABY = 3_200_000  # the table size the issue names; a wrong value here fails the decryption asserts below


# ---------------------------------------------------------------------------------------------------------
# the stand-in for ecdsa.ellipticcurve

class CurveFp:
    def __init__(self, p, a, b, h=None):
        self._p, self._a, self._b = int(p), int(a), int(b)

    def p(self):
        return self._p

    def a(self):
        return self._a

    def b(self):
        return self._b

    def contains_point(self, x, y):
        return (y * y - (x * x * x + self._a * x + self._b)) % self._p == 0

    def __eq__(self, other):
        return isinstance(other, CurveFp) and (self._p, self._a, self._b) == (other._p, other._a, other._b)

    def __hash__(self):
        return hash((self._p, self._a, self._b))


class Point:
    """affine point of y^2 = x^3 + a x + b over F_p; x = y = None is the identity"""

    def __init__(self, curve, x, y, order=None):
        self._curve, self._x, self._y = curve, x, y
        if curve is not None and x is not None:
            assert curve.contains_point(x, y), "point is not on the curve"

    def x(self):
        return self._x

    def y(self):
        return self._y

    def curve(self):
        return self._curve

    def __eq__(self, other):
        if not isinstance(other, Point):
            return NotImplemented  # Python then answers False: a point is unequal to 0
        return self._x == other._x and self._y == other._y

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash((self._x, self._y))

    def __neg__(self):
        return self if self._x is None else Point(self._curve, self._x, -self._y % self._curve.p())

    def __add__(self, other):
        if not isinstance(other, Point):
            return NotImplemented  # numpy object arrays then broadcast over their elements
        if self._x is None:
            return other
        if other._x is None:
            return self
        p = self._curve.p()
        if self._x == other._x:
            if (self._y + other._y) % p == 0:
                return INFINITY
            lam = (3 * self._x * self._x + self._curve.a()) * pow(2 * self._y, -1, p) % p
        else:
            lam = (other._y - self._y) * pow(other._x - self._x, -1, p) % p
        x3 = (lam * lam - self._x - other._x) % p
        return Point(self._curve, x3, (lam * (self._x - x3) - self._y) % p)

    def __mul__(self, k):
        try:
            k = operator.index(k)  # Python and numpy integers
        except TypeError:
            return NotImplemented
        if k < 0:
            return (-self) * (-k)
        acc = INFINITY
        for bit in bin(k)[2:] if k else "":
            acc = acc + acc
            if bit == "1":
                acc = acc + self
        return acc

    __rmul__ = __mul__

    def __repr__(self):
        return "Point(identity)" if self._x is None else "Point(%x, %x)" % (self._x, self._y)


INFINITY = Point(None, None, None)


def self_check(curve, G, order):
    assert curve.contains_point(G.x(), G.y()), "G is not on the curve"
    assert order * G == INFINITY and (order * G).x() is None and 0 * G == INFINITY and G * (3 * order) == INFINITY
    assert G + G == 2 * G and G + (-G) == INFINITY and INFINITY + G == G and G + INFINITY == G
    vals = [1, 2, 3, 255, 65537, 2**104 - 3, order - 1, order // 2, 0x1F3D5B79A2C4E6081F3D5B79A2C4E608]
    for a, b in zip(vals, vals[1:] + vals[:1]):
        assert (a + b) * G == a * G + b * G
        assert (-a) * G == -(a * G) and (a * G) * -1 == -(a * G)
        assert a * (b * G) == (a * b % order) * G == (a * b) * G
        assert np.int64(a % 2**31) * G == G * (a % 2**31) == int(a % 2**31) * G
    P = 77 * G
    assert P + P == 2 * P and (P == 0) is False and (P != 0) is True and P != -P
    # numpy object arrays: padding with the identity, int * array, a point plus an array, matmul
    arr = np.empty((2, 2), dtype=object)
    arr[0, 0], arr[0, 1], arr[1, 0], arr[1, 1] = G, 2 * G, 3 * G, 4 * G
    pad = np.pad(arr, 1, mode="constant", constant_values=INFINITY)
    assert pad.shape == (4, 4) and pad[0, 0] == INFINITY and pad[1, 1] == G and pad[2, 2] == 4 * G
    row = INFINITY + 5 * arr[1]
    assert row[0] == 15 * G and row[1] == 20 * G
    mm = np.matmul(arr, np.array([[1, 0], [2, 3]], dtype=np.int32))
    assert mm[0, 0] == 5 * G and mm[0, 1] == 6 * G and mm[1, 0] == 11 * G and mm[1, 1] == 12 * G


# ---------------------------------------------------------------------------------------------------------
# loading the reference's modules, and the deterministic environment of a case

def load_reference():
    ec = types.ModuleType("ecdsa.ellipticcurve")
    ec.CurveFp, ec.Point, ec.INFINITY = CurveFp, Point, INFINITY
    pkg = types.ModuleType("ecdsa")
    pkg.ellipticcurve = ec
    import multiprocessing  # noqa: F401  (the servers import it; it wants the real socket module, so it loads first)
    import socket as real_socket

    def no_network(*a, **kw):
        raise AssertionError("the reference reached for the network")

    sock = types.ModuleType("socket")
    sock.__dict__.update({k: v for k, v in vars(real_socket).items() if not k.startswith("__")})
    sock.gethostbyname = lambda name: "127.0.0.1"
    sock.socket = sock.getaddrinfo = sock.create_connection = sock.gethostbyname_ex = no_network
    saved = {k: sys.modules.get(k) for k in ("socket", "ecdsa", "ecdsa.ellipticcurve")}
    saved_argv, saved_dwb = sys.argv, sys.dont_write_bytecode
    sys.modules.update({"socket": sock, "ecdsa": pkg, "ecdsa.ellipticcurve": ec})
    sys.argv = ["reference", "50007", "50007", "32"]
    sys.dont_write_bytecode = True
    mods, digests = {}, {}
    try:
        for name, rel in FILES.items():
            path = os.path.join(REF, rel)
            with open(path, "rb") as f:
                digests[rel] = hashlib.sha256(f.read()).hexdigest()
            spec = importlib.util.spec_from_file_location("vpin_reference_" + name, path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods[name] = mod
    finally:
        sys.argv, sys.dont_write_bytecode = saved_argv, saved_dwb
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods, digests


@contextlib.contextmanager
def deterministic(keys=(), rs=(), order=None):
    """os.urandom hands out `keys`, random.randrange hands out `rs`, in call order; both must be used up; stdout is dropped"""
    keys, rs = list(keys), list(rs)
    real_urandom, real_randrange = os.urandom, random.randrange

    def urandom(n):
        assert n == 32 and keys, "an os.urandom call the case did not plan"
        return keys.pop(0)

    def randrange(lo, hi):
        assert rs, "a random.randrange call the case did not plan"
        assert order is None or (lo, hi) == (1, order - 1)
        r = rs.pop(0)
        assert lo <= r < hi
        return r

    os.urandom, random.randrange = urandom, randrange
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        os.urandom, random.randrange = real_urandom, real_randrange
    assert not keys and not rs, "the case planned more randomness than the reference drew"


LISTS = ("points_mult", "weights_array", "point_one_Add", "point_two_Add")


def clear_lists(mod):
    for name in LISTS:
        del getattr(mod, name)[:]


@contextlib.contextmanager
def caught(mod, fname):
    """record what mod.fname returns while the reference's other functions call it"""
    orig, seen = getattr(mod, fname), []

    def wrapper(*a, **kw):
        out = orig(*a, **kw)
        seen.append(out)
        return out

    setattr(mod, fname, wrapper)
    try:
        yield seen
    finally:
        setattr(mod, fname, orig)


# ---------------------------------------------------------------------------------------------------------
# the fixture's own inputs: drawn with SHA-256 over labels, so that the file depends on nothing else

def draw_key(label):
    return hashlib.sha256(("layer_pins/key/" + label).encode()).digest()


def draw_r(label, order):
    return int.from_bytes(hashlib.sha256(("layer_pins/r/" + label).encode()).digest(), "big") % (order - 2) + 1


def draw_small(label, count, lo, hi):
    """count integers in lo .. hi"""
    out, ctr = [], 0
    while len(out) < count:
        d = hashlib.sha256(("layer_pins/int/%s/%d" % (label, ctr)).encode()).digest()
        out += [lo + int.from_bytes(d[i:i + 4], "big") % (hi - lo + 1) for i in range(0, 32, 4)]
        ctr += 1
    return out[:count]


class Pins:
    def __init__(self):
        self.points, self.index = [], {}

    def pid(self, P):
        assert isinstance(P, Point)
        if P.x() is None:
            return None
        key = (int(P.x()), int(P.y()))
        if key not in self.index:
            self.index[key] = len(self.points)
            self.points.append(["%064x" % key[0], "%064x" % key[1]])
        return self.index[key]

    def pids(self, seq):
        return [self.pid(P) for P in seq]


def prf_bytes_of(mod, key):
    """how many leading digest bytes the module's pf reads, found by comparing its output with HMAC-SHA256 prefixes"""
    digest = hmac.new(key, b"0", hashlib.sha256).digest()
    got = mod.pf(key, 0)
    hits = [n for n in range(1, 33) if int.from_bytes(digest[:n], "big") == got]
    assert len(hits) == 1, hits
    return hits[0]


def read_lists(pins, mod, weight=int):
    return dict(mult_weights=[str(weight(w)) for w in mod.weights_array], mult_points=pins.pids(mod.points_mult),
                add_p=pins.pids(mod.point_one_Add), add_r=pins.pids(mod.point_two_Add))


def encrypt_image(client, curve_info, h, image4d, rs):
    curve, q, order, G, _ = curve_info
    with deterministic(rs=rs, order=order):
        return client.encryptFixedPointValue(image4d, curve, q, order, G, h, 0)


def plain_conv(img, filt, pad, stride):
    p = np.pad(np.asarray(img, dtype=np.int64), pad)
    fh, fw = filt.shape
    oh, ow = (p.shape[0] - fh) // stride + 1, (p.shape[1] - fw) // stride + 1
    return np.array([[int((p[i * stride:i * stride + fh, j * stride:j * stride + fw] * filt).sum()) for j in range(ow)]
                     for i in range(oh)], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------
# the cases

def conv_case(pins, name, service, mod, client, curve_info, h, image, filt, pad, stride, planes, twins=(), negs=()):
    """image: H x W ints.  filt None: the module's callConv2_ciphertext chooses it (LeNet).  planes: which ciphertext planes go
    through the layer.  twins: pairs of pixels that share message and r (a repeated ciphertext); negs: pairs (a, b) where
    pixel b is encrypted with -message and order - r of pixel a (the ciphertext pair P, -P); image must agree."""
    _, q, order, G, identity = curve_info
    image = np.array(image, dtype=np.int64)
    H, W = image.shape
    rs = [draw_r("%s/%d" % (name, i), order) for i in range(H * W)]
    for a, b in twins:
        assert image[a] == image[b]
        rs[b[0] * W + b[1]] = rs[a[0] * W + a[1]]
    for a, b in negs:
        assert image[a] == -image[b]
        rs[b[0] * W + b[1]] = order - rs[a[0] * W + a[1]]
    c1, c2 = encrypt_image(client, curve_info, h, image.reshape(1, 1, H, W), rs)
    for a, b in twins:
        assert c1[0][0][a] == c1[0][0][b] and c2[0][0][a] == c2[0][0][b]
    for a, b in negs:
        assert c1[0][0][a] == -c1[0][0][b] and c2[0][0][a] == -c2[0][0][b]
    keys = [draw_key("%s/%s" % (name, p)) for p in planes]
    clear_lists(mod)
    with deterministic(keys=keys), caught(mod, "rLCL") as lefts:
        if filt is None:            # LeNet: the filter is the function's own
            assert planes == ["c1", "c2"]
            out = [mod.callConv2_ciphertext(c, identity, q, pad, stride) for c in (c1, c2)]
        elif planes == ["c1", "c2"]:  # the convolution service, the way its inferenceCNN calls it (pad 1, stride 1 are its own)
            assert (pad, stride) == (1, 1)
            out = list(mod.conv2_ciphertext(c1, c2, identity, q, np.array(filt)))
        else:                        # one plane through myConv2d itself
            src = dict(c1=c1, c2=c2)
            out = [mod.myConv2d(src[p][0][0], np.array(filt), identity, q, 1, padding_size=pad, stride=stride)[None, None]
                   for p in planes]
    lists = read_lists(pins, mod)
    taps = len(mod.weights_array) // len(planes)
    filt_run = [int(w) for w in mod.weights_array[:taps]]
    fh = len(filt) if filt is not None else int(round(taps ** 0.5))
    fw = taps // fh
    assert fh * fw == taps and all([int(w) for w in mod.weights_array[p * taps:(p + 1) * taps]] == filt_run
                                   for p in range(len(planes)))
    if filt is not None:
        assert filt_run == [int(v) for row in filt for v in row]
    oh, ow = out[0].shape[2:]
    assert (oh, ow) == ((H + 2 * pad - fh) // stride + 1, (W + 2 * pad - fw) // stride + 1) and len(lefts) == len(planes)
    src = dict(c1=c1, c2=c2)
    case = dict(name=name, service=service, prf_bytes=prf_bytes_of(mod, keys[0]), H=H, W=W, fh=fh, fw=fw, filter=filt_run,
                pad=pad, stride=stride, oh=int(oh), ow=int(ow), image=image.tolist(), r=["%064x" % r for r in rs],
                planes=planes, keys=[k.hex() for k in keys],
                input=[pins.pids(src[p][0][0].flatten()) for p in planes],
                output=[pins.pids(o[0][0].flatten()) for o in out], left=pins.pids(lefts), **lists)
    return case, (c1, c2), out, np.array(filt_run, dtype=np.int64).reshape(fh, fw)


def fc_case(pins, name, service, mod, client, curve_info, h, xs, weights, bias):
    curve, q, order, G, identity = curve_info
    K, N = len(xs), len(bias)
    W = np.array(weights, dtype=np.int32)
    assert W.shape == (K, N) and W.min() >= 0 and W.max() <= 11016
    # the randomness depends on the shape alone, so that two services run on the same ciphertexts
    rs = [draw_r("fc%dx%d/x/%d" % (K, N, i), order) for i in range(K)]
    rb = [draw_r("fc%dx%d/b/%d" % (K, N, i), order) for i in range(N)]
    with deterministic(rs=rs, order=order):
        c1, c2 = client.encryptFixedPointValue(np.array(xs, dtype=np.int64).reshape(1, K), curve, q, order, G, h, 1)
    with deterministic(rs=rb, order=order):
        b1, b2 = mod.encryptBias(np.array(bias, dtype=np.int32), order, G, h)
    keys = [draw_key("%s/c1" % name), draw_key("%s/c2" % name)]
    clear_lists(mod)
    with deterministic(keys=keys), caught(mod, "rLCL") as lefts:
        out = [mod.FCLayer(c, W, b, 1, identity, q) for c, b in ((c1, b1), (c2, b2))]
    assert len(lefts) == 2 and all(o.shape == (1, N) for o in out)
    lists = read_lists(pins, mod)
    return dict(name=name, service=service, prf_bytes=prf_bytes_of(mod, keys[0]), K=K, N=N, x=[int(v) for v in xs],
                weights=W.tolist(), bias=[int(v) for v in bias], r=["%064x" % r for r in rs], r_bias=["%064x" % r for r in rb],
                rows=["c1", "c2"], keys=[k.hex() for k in keys], input=[pins.pids(c[0]) for c in (c1, c2)],
                bias_points=[pins.pids(b) for b in (b1, b2)], output=[pins.pids(o[0]) for o in out], left=pins.pids(lefts),
                **lists)


def pool_case(pins, name, mod, client, curve_info, h, image, k, stride):
    _, q, order, G, identity = curve_info
    image = np.array(image, dtype=np.int64)
    H, W = image.shape
    rs = [draw_r("%s/%d" % (name, i), order) for i in range(H * W)]
    c1, c2 = encrypt_image(client, curve_info, h, image.reshape(1, 1, H, W), rs)
    clear_lists(mod)
    with deterministic(), caught(mod, "realNumbersToFixedPointRepresentation") as scales:
        out = [mod.myAvgPool2d(1, c[0][0], identity, 1, 0, k, stride) for c in (c1, c2)]
    assert not mod.points_mult and not mod.weights_array
    scale = {int(s) for s in scales}
    assert len(scale) == 1 and len(scales) == 2 * out[0].size
    lists = read_lists(pins, mod)
    return dict(name=name, service="LeNet", H=H, W=W, k=k, stride=stride, oh=out[0].shape[0], ow=out[0].shape[1],
                scale=scale.pop(), image=image.tolist(), r=["%064x" % r for r in rs], planes=["c1", "c2"],
                input=[pins.pids(c[0][0].flatten()) for c in (c1, c2)], output=[pins.pids(o.flatten()) for o in out],
                add_p=lists["add_p"], add_r=lists["add_r"])


def baby_table(G, values, decoys):
    """the reference's table format {(x, y): j}, the identity keyed (None, None) -> 0, holding the baby steps these values
    need and a few more"""
    js = sorted({0} | {abs(v) % M_BABY for v in values} | set(decoys))
    table = {}
    for j in js:
        P = j * G
        table[(P.x(), P.y())] = j
    assert table[(None, None)] == 0
    return table, js


def client_case(pins, mods, curve_info, sk, h):
    client, bsgs = mods["lenet_client"], mods["bsgs"]
    curve, q, order, G, identity = curve_info
    m = M_BABY
    out = dict(sk="%064x" % sk, h=pins.pid(h), encrypt=[], m=m)
    for i, msg in enumerate([0, 1, -1, 65535, -65536, 2**20 + 3]):
        r = draw_r("client/enc/%d" % i, order)
        with deterministic(rs=[r], order=order):
            c1, c2 = client.encrypt(msg, curve, q, order, G, h)
        out["encrypt"].append(dict(msg=msg, r="%064x" % r, c1=pins.pid(c1), c2=pins.pid(c2)))
    values = [0, 1, -1, m - 1, m, -m, 3 * m + 17, -(2 * m + 5), 5 * m + m - 1]
    rs = [draw_r("client/dec/%d" % i, order) for i in range(len(values))]
    with deterministic(rs=rs, order=order):
        c1, c2 = client.encryptFixedPointValue(np.array(values, dtype=np.int64).reshape(1, -1), curve, q, order, G, h, 1)
    table, js = baby_table(G, values, decoys=[2, 16, 18, 4, 6, 1000, m - 2, m // 2])
    with deterministic():
        got = client.decrypt_c1_c2(sk, c1, c2, G, table, 1)
    results = [int(v) for v in got[0]]
    assert results == values, (results, values)
    out["decrypt"] = dict(values=values, r=["%064x" % r for r in rs], c1=pins.pids(c1[0]), c2=pins.pids(c2[0]),
                          results=results, table_js=js)
    # the table script's own giant step (non-negative values only: it has no second walk), its table read from memory
    assert bsgs.curveE2Info()[1:3] == (q, order) and bsgs.curveE2Info()[3] == G
    script = []
    real_load = bsgs.load_table
    bsgs.load_table = lambda filename: table
    try:
        for v in [v for v in values if v >= 0]:
            with deterministic():
                res, _ = bsgs.giant_step(G, v * G, order)
            assert res == v
            script.append(dict(point=pins.pid(v * G), result=int(res)))
    finally:
        bsgs.load_table = real_load
    out["table_script"] = script
    return out


def chained_case(pins, client, curve_info, sk, conv, out_planes, image, filt):
    """the LeNet convolution's output ciphertext through the reference's decrypt, against numpy's plain convolution"""
    _, q, order, G, identity = curve_info
    plain = plain_conv(image, filt, conv["pad"], conv["stride"])
    table, js = baby_table(G, plain.flatten().tolist(), decoys=[1, 2, 3])
    with deterministic():
        got = client.decrypt_c1_c2(sk, out_planes[0], out_planes[1], G, table, 0)
    values = [[int(v) for v in row] for row in got[0][0]]
    assert values == plain.tolist(), (values, plain.tolist())
    assert (plain < 0).any() and (plain > 0).any()
    return dict(conv=conv["name"], values=values, table_js=js)


def prf_pins(mods):
    out = []
    for service, name in (("LeNet", "lenet_server"), ("cnn_networks", "cnn_server"), ("convolution", "conv_server")):
        key = draw_key("prf/" + service)
        ts = [0, 1, 9, 10, 11, 99, 100, 3834]
        out.append(dict(service=service, prf_bytes=prf_bytes_of(mods[name], key), key=key.hex(), t=ts,
                        values=[str(mods[name].pf(key, t)) for t in ts]))
    return out


LENET_IMAGE = [[3, -1, 0, 7, 2, -4],
               [0, 5, -6, 1, 9, 2],
               [-2, 8, 4, 0, -3, 6],
               [1, 0, -7, 5, 2, 11],
               [6, -5, 3, 12, 0, -1],
               [0, 2, 9, -8, 4, 1],
               [-3, 7, 1, 0, 5, -2]]
CONV_IMAGE_A = [[4, -1, -4, 0],    # (0, 0) and (0, 2): the ciphertext pair P, -P, two columns apart so that a window cancels them
                [2, 7, -3, 5],     # (1, 1) and (3, 2): a repeated ciphertext
                [0, -6, 1, 9],
                [-2, 3, 7, 0],
                [8, 0, -5, 6]]
CONV_FILTER_A = [[1, 0, 1], [2, 0, 2], [1, 0, 1]]
CONV_IMAGE_B = [[1, -2, 0, 4, 3],
                [5, 0, -1, 2, -6],
                [0, 3, 8, -4, 1],
                [-7, 2, 0, 6, 5],
                [4, -3, 9, 0, -2],
                [2, 1, -5, 7, 0]]
CONV_FILTER_B = [[3, 1], [0, 2]]
POOL_IMAGE = [[5, 0, -3, 8, 1, -1],
              [2, -4, 7, 0, 6, 3],
              [0, 9, 1, -2, -5, 4],
              [-6, 3, 0, 5, 2, 7],
              [1, -1, 4, 6, 0, -8],
              [3, 2, -7, 0, 9, 5]]


def main():
    out_path = os.path.join(HERE, "layer_pins.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    mods, digests = load_reference()
    lenet, cnn, convsrv, client = mods["lenet_server"], mods["cnn_server"], mods["conv_server"], mods["lenet_client"]
    for mod in (lenet, cnn, convsrv):
        mod.MultiCoreFeature = 0
    curve, q, order, G, identity = client.curveE2Info()
    self_check(curve, G, order)
    assert identity == INFINITY and identity.x() is None
    sk = draw_r("sk", order)
    with deterministic(rs=[sk], order=order):
        curve_info = client.keyGen()
    h, got_sk = curve_info[4], curve_info[5]
    assert got_sk == sk and curve_info[2] == order
    curve_info = (curve, q, order, G, identity)

    pins = Pins()
    out = dict(about="recorded runs of the reference's own Python (tests/golden/make_layer_pins.py); inputs and outputs only",
               multi_core_feature=0, reference_sha256=digests,
               curve=dict(q="%064x" % q, a="%064x" % curve.a(), b="%064x" % curve.b(), gx="%064x" % G.x(), gy="%064x" % G.y(),
                          order="%064x" % order),
               prf=prf_pins(mods))
    out["client"] = client_case(pins, mods, curve_info, sk, h)
    print("client", file=sys.stderr)

    conv_l, _, out_l, filt_l = conv_case(pins, "conv_lenet_7x6", "LeNet", lenet, client, curve_info, h, LENET_IMAGE, None, 1, 1,
                                         ["c1", "c2"])
    conv_a, _, _, _ = conv_case(pins, "conv_service_5x4", "convolution", convsrv, client, curve_info, h, CONV_IMAGE_A,
                                CONV_FILTER_A, 1, 1, ["c1", "c2"], twins=[((1, 1), (3, 2))], negs=[((0, 0), (0, 2))])
    conv_b, _, _, _ = conv_case(pins, "conv_service_6x5_stride2", "convolution", convsrv, client, curve_info, h, CONV_IMAGE_B,
                                CONV_FILTER_B, 0, 2, ["c2"])
    out["conv"] = [conv_l, conv_a, conv_b]
    print("conv", file=sys.stderr)

    x5, b5 = [3, -7, 0, 11, -2], [-40, 0, 17]
    w5 = [[11016, 0, 7], [1, 5000, 0], [0, 3, 9999], [256, 65, 1], [4097, 0, 2]]
    x70 = draw_small("fc70/x", 70, -9, 9)
    x70[0], x70[1], x70[69] = 0, -9, 9
    w70 = np.array(draw_small("fc70/w", 70 * 4, 0, 11016)).reshape(70, 4)
    w70[::7, 1] = 0
    w70[3, :] = [0, 11016, 1, 0]
    w70[69, 3] = 11016
    b70 = [-12345, 0, 1, 30000]
    out["fc"] = [fc_case(pins, "fc_lenet_5x3", "LeNet", lenet, client, curve_info, h, x5, w5, b5),
                 fc_case(pins, "fc_lenet_70x4", "LeNet", lenet, client, curve_info, h, x70, w70.tolist(), b70),
                 fc_case(pins, "fc_cnn_networks_5x3", "cnn_networks", cnn, client, curve_info, h, x5, w5, b5)]
    assert out["fc"][0]["input"] == out["fc"][2]["input"] and out["fc"][0]["output"] == out["fc"][2]["output"]
    print("fc", file=sys.stderr)

    out["pool"] = [pool_case(pins, "pool_lenet_6x6", lenet, client, curve_info, h, POOL_IMAGE, 2, 2)]
    out["chained"] = chained_case(pins, client, curve_info, sk, conv_l, out_l, LENET_IMAGE, filt_l)
    out["points"] = pins.points
    for mod in (lenet, cnn, convsrv):
        clear_lists(mod)

    txt = json.dumps(out, sort_keys=True, separators=(",", ":"))
    for key in ('"points":[', '"add_p":', '"add_r":', '"mult_points":', '"mult_weights":', '"input":', '"output":', '"r":',
                '"conv":[', '"fc":[', '"pool":[', '"client":', '"chained":', '"prf":[', '{"H":', '{"K":', '"weights":'):
        txt = txt.replace(key, "\n" + key)
    txt = txt.replace('"],["', '"],\n["')
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(txt + "\n")
    print("wrote %s: %d bytes, %d points" % (out_path, len(txt) + 1, len(pins.points)), file=sys.stderr)


if __name__ == "__main__":
    main()
