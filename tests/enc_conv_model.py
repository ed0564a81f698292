"""Python model of the encrypted convolution layer and its random-linear-combination (RLC) check: the type-1 path of the
reference service's myConv2d with rLCL / rLCR (src/convolution/Server.py, src/LeNet/Server.py) on gadgets_model.e2_add / e2_mul,
hmac and hashlib.  It is checked against recorded runs of the reference's own functions: tests/golden/layer_pins.json
(tests/golden/make_layer_pins.py), compared in tests/test_layer_pins.py.

The model is generic over the group it computes in:
  POINTS  the literal one: affine points of E2, None = the identity (one scalar multiplication costs ~10-17 ms)
  LOGS    discrete logarithms to the base G, integers mod E2_ORDER, 0 = the identity.  G has prime order E2_ORDER, so an image of
          pixels k_p * G (what vpin_synthetic_points produces) goes through the layer as plain modular arithmetic and every expected
          point is ONE scalar multiplication of G (log_point) -- what makes the larger shapes affordable.
"""
import hashlib
import hmac

import gadgets_model as GM

G = (GM.E2_GX, GM.E2_GY)
ORDER = GM.E2_ORDER


class ShapeError(Exception):
    """VPIN_ESHAPE: a multiplication operand or an addition accumulator is the identity"""


class VerifyError(Exception):
    """VPIN_EVERIFY: the two sides of the check differ"""


class Points:
    identity = None
    add = staticmethod(GM.e2_add)

    @staticmethod
    def mul(k, P):
        return None if P is None else GM.e2_mul(k, P)


class Logs:
    identity = 0

    @staticmethod
    def add(a, b):
        return (a + b) % ORDER

    @staticmethod
    def mul(k, a):
        return k * a % ORDER


POINTS, LOGS = Points, Logs

_log_cache = {}


def log_point(k):
    """k * G as an affine point, None for k = 0 (mod the order)"""
    k %= ORDER
    if k not in _log_cache:
        _log_cache[k] = GM.e2_mul(k, G) if k else None
    return _log_cache[k]


def synthetic_logs(seed, count):
    """the discrete logs of vpin_synthetic_points(seed, count)"""
    out, st = [], seed
    for _ in range(count):
        st, k = GM.splitmix64(st)
        out.append(k or 1)
    return out


def prf(key, t, prf_bytes):
    return int.from_bytes(hmac.new(bytes(key), str(t).encode("ascii"), hashlib.sha256).digest()[:prf_bytes], "big")


def out_dims(H, W, fh, fw, pad, stride):
    return (H + 2 * pad - fh) // stride + 1, (W + 2 * pad - fw) // stride + 1


def window(grp, plane, H, W, fh, fw, pad, stride, i, j):
    """the fh * fw elements under output (i, j), row-major; padding is the identity"""
    out = []
    for ii in range(fh):
        for jj in range(fw):
            r, c = i * stride + ii - pad, j * stride + jj - pad
            out.append(plane[r * W + c] if 0 <= r < H and 0 <= c < W else grp.identity)
    return out


def conv2d(grp, plane, H, W, filt, fh, fw, pad, stride):
    oh, ow = out_dims(H, W, fh, fw, pad, stride)
    out = []
    for i in range(oh):
        for j in range(ow):
            acc = grp.identity
            for w, x in zip(filt, window(grp, plane, H, W, fh, fw, pad, stride, i, j)):
                acc = grp.add(acc, grp.mul(w, x))
            out.append(acc)
    return out


def layer(grp, planes, H, W, filt, fh, fw, pad, stride, keys, prf_bytes):
    """planes: P lists of H * W group elements.  Returns dict(out = P lists of oh * ow elements, mults = [(w, B'[k])],
    adds = [(acc, T_k)] (an identity T_k is what the witness writes as rz = 1), left = P elements, Bp = P lists of fh * fw)."""
    oh, ow = out_dims(H, W, fh, fw, pad, stride)
    taps = fh * fw
    res = dict(out=[], mults=[], adds=[], left=[], Bp=[])
    for plane, key in zip(planes, keys):
        out = conv2d(grp, plane, H, W, filt, fh, fw, pad, stride)
        r = [prf(key, t, prf_bytes) for t in range(oh * ow)]
        left = grp.identity
        Bp = [grp.identity] * taps
        for t in range(oh * ow):
            left = grp.add(left, grp.mul(r[t], out[t]))
            win = window(grp, plane, H, W, fh, fw, pad, stride, t // ow, t % ow)
            for k in range(taps):
                Bp[k] = grp.add(Bp[k], grp.mul(r[t], win[k]))
        acc = grp.identity
        for k in range(taps):
            if Bp[k] == grp.identity:
                raise ShapeError(f"B'[{k}] is the identity")
            res["mults"].append((filt[k], Bp[k]))
            T = grp.mul(filt[k], Bp[k])
            if k == 0:
                acc = T
                continue
            if acc == grp.identity:
                raise ShapeError(f"the accumulator before tap {k} is the identity")
            res["adds"].append((acc, T))
            acc = grp.add(acc, T)
        if acc != left:
            raise VerifyError("sum_k w[k] * B'[k] != sum_t r_t * out[t]")
        res["out"].append(out)
        res["left"].append(left)
        res["Bp"].append(Bp)
    return res
