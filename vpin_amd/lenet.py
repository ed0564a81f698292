"""The whole encrypted LeNet inference over the C ABI (vpin_lenet_*): the server loop over the encrypted layers, the client's
rounds in between (decrypt, activation, encrypt again, one launch chain per round on the device) and the witness lists of the
seven labels L1 .. L7 for the prover.  An image goes in; the class scores, every round's values and the trace come out.

The network's constants are data, not code: `default_config` takes the filter and the connection table from the caller, or
reads them from the fixtures recorded off runs of the reference (tests/golden/layer_pins.json, inference_pins.json)."""
import ctypes as C
import json
import os

import numpy as np

from .capi import LENET_ROUND_FN, ConvTrace, DevInstance, LenetCfg, _chk, lib

RELU, REENCRYPT = 1, 2
LABELS = ("L1", "L2", "L3", "L4", "L5", "L6", "L7")
_GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def min_max_scaling(image):
    image = np.asarray(image)
    lo, hi = np.min(image), np.max(image)
    return np.clip((image - lo) / (hi - lo), a_min=0.001, a_max=0.9999999)


def fixed_point(values, bits=16):
    """real numbers -> the int32 fixed point the reference works on (truncation toward zero)"""
    return (np.asarray(values) * 2**bits).astype(np.int32)


def preprocess(image):
    """the client's min_max_scaling and 16-bit fixed point: an H x W (or 1 x 1 x H x W) image of reals -> int32 of the same shape"""
    return fixed_point(min_max_scaling(image))


class Config:
    """A vpin_lenet_cfg and the arrays it points to."""

    def __init__(self, filt, connect, w1, b1, w2, b2):
        self.c = LenetCfg()
        _chk(lib().vpin_lenet_cfg_default(C.byref(self.c)), "vpin_lenet_cfg_default")
        self.set_arrays(filt, connect, w1, b1, w2, b2)

    def set_arrays(self, filt, connect, w1, b1, w2, b2):
        c = self.c
        filt = [[int(v) for v in row] for row in filt]
        self.connect = np.ascontiguousarray(np.asarray(connect, dtype=np.uint8))
        self.filt = np.frombuffer(b"".join(v.to_bytes(16, "little") for row in filt for v in row), dtype=np.uint8).copy()
        self.w1, self.w2 = (np.ascontiguousarray(np.asarray(w, dtype=np.int64).astype(np.int32)) for w in (w1, w2))
        assert np.array_equal(self.w1, np.asarray(w1, dtype=np.int64)) and np.array_equal(self.w2, np.asarray(w2, dtype=np.int64))
        self.b1, self.b2 = (np.ascontiguousarray(np.asarray(b, dtype=np.int64)) for b in (b1, b2))
        c.f = len(filt)
        c.n2, c.n1 = self.connect.shape
        c.n3, c.N1 = self.w1.shape
        assert self.w2.shape[0] == c.N1 and self.b1.shape == (c.N1,)
        c.N2 = self.w2.shape[1]
        assert self.b2.shape == (c.N2,)
        p = lambda a: a.ctypes.data_as(C.c_void_p).value
        c.connect, c.filter_le16, c.w1, c.w2, c.b1, c.b2 = p(self.connect), p(self.filt), p(self.w1), p(self.w2), p(self.b1), p(self.b2)

    def set_rounds(self, relu=None, shift_bits=None, max_giant=None):
        for name, vals in (("relu", relu), ("shift_bits", shift_bits), ("max_giant", max_giant)):
            if vals is not None:
                assert len(vals) == 7
                for i, v in enumerate(vals):
                    getattr(self.c, name)[i] = int(v)

    def set_pool(self, k, stride, scale):
        self.c.pool_k, self.c.pool_stride = k, stride
        self.c.pool_scale_le16[:] = list(int(scale).to_bytes(16, "little"))

    def counts(self):
        out = (C.c_size_t * 32)()
        _chk(lib().vpin_lenet_cfg_counts(C.byref(self.c), out), "vpin_lenet_cfg_counts")
        o = [int(v) for v in out]
        return dict(labels=list(zip(o[0:7], o[7:14])), per_round=o[14:21], decryptions=o[21], encryptions=o[22], prf_keys=o[23], bias_r=o[24])


def default_config(w1, b1, w2, b2, filt=None, connect=None):
    """the reference's LeNet around fixed-point weights (n3 x N1 and N1 x N2 non-negative ints, N1 and N2 bias ints).  The filter
    (f x f ints) and the connection table (n2 x n1) are the caller's; where one is None it is read from the fixtures of the
    source tree, tests/golden/layer_pins.json and inference_pins.json, so a package installed without tests/ must pass both"""
    if filt is None or connect is None:
        missing = [n for n in ("layer_pins.json", "inference_pins.json") if not os.path.exists(os.path.join(_GOLDEN, n))]
        if missing:
            raise FileNotFoundError("default_config: no filter / connection table given and %s not found under %s; pass filt= and "
                                    "connect=" % (", ".join(missing), _GOLDEN))
        with open(os.path.join(_GOLDEN, "layer_pins.json")) as f:
            conv = next(c for c in json.load(f)["conv"] if c["name"] == "conv_lenet_7x6")
        with open(os.path.join(_GOLDEN, "inference_pins.json")) as f:
            table = json.load(f)["second_conv"][-1]["connect"]
        filt = np.array([int(v) for v in conv["filter"]], dtype=object).reshape(conv["fh"], conv["fw"]).tolist() if filt is None else filt
        connect = table if connect is None else connect
    return Config(filt, connect, w1, b1, w2, b2)


class Client:
    """vpin_lenet_client: the key, the two base tables, the discrete-log table and the queue of randomness"""

    def __init__(self, ctx, sk, nb, max_giant, rs):
        self.ctx = ctx
        h = C.c_void_p()
        k = ctx._u256s([sk])
        r = ctx._u256s(rs) if len(rs) else np.zeros(32, np.uint8)
        mg = (C.c_uint64 * 7)(*[int(v) for v in max_giant])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _chk(lib().vpin_lenet_client_create(ctx.h, p(k), nb, mg, p(r), len(rs), C.byref(h)), "vpin_lenet_client_create")
        self.h = h
        g, hh = C.c_void_p(), C.c_void_p()
        _chk(lib().vpin_lenet_client_bases(h, C.byref(g), C.byref(hh)), "vpin_lenet_client_bases")
        self.base_g, self.base_h = g, hh
        self.round_fn = C.cast(lib().vpin_lenet_client_round, C.c_void_p)
        self.user = h

    def encrypt(self, msgs, rs):
        """the image's encryption under the client's key -> (c1, c2), each (x, y, inf)"""
        return self.ctx.e2_encrypt(self.base_g, self.base_h, msgs, rs)

    def values(self, rnd):
        """(v, act) of round 1 .. 7 as int64 arrays"""
        v, a, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _chk(lib().vpin_lenet_client_values(self.h, rnd, C.byref(v), C.byref(a), C.byref(n)), "vpin_lenet_client_values")
        get = lambda p: np.frombuffer((C.c_int64 * n.value).from_address(p.value), dtype=np.int64).copy() if n.value else np.zeros(0, np.int64)
        return get(v), get(a)

    def free(self):
        if self.h:
            lib().vpin_lenet_client_free(self.h)
            self.h = None


def python_round(fn):
    """a vpin_lenet_round_fn around fn(round, relu, reencrypt, shift_bits, c1, c2) -> (c1_out, c2_out) or None, the ciphertexts
    as (x, y, inf) numpy triples.  An exception must not unwind through the C frames: the callback returns VPIN_EINVAL, keeps
    the exception in `.error`, and `run` raises it again once vpin_lenet_infer has returned"""

    def cb(user, rnd, flags, bits, x1, y1, f1, x2, y2, f2, cnt, ox1, oy1, of1, ox2, oy2, of2):
        view = lambda p, n: np.frombuffer((C.c_uint8 * n).from_address(p), dtype=np.uint8)
        try:
            c1 = (view(x1, 32 * cnt).reshape(cnt, 32).copy(), view(y1, 32 * cnt).reshape(cnt, 32).copy(), view(f1, cnt).copy())
            c2 = (view(x2, 32 * cnt).reshape(cnt, 32).copy(), view(y2, 32 * cnt).reshape(cnt, 32).copy(), view(f2, cnt).copy())
            out = fn(rnd, bool(flags & RELU), bool(flags & REENCRYPT), bits, c1, c2)
            if flags & REENCRYPT:
                for dst, src, n in zip((ox1, oy1, of1, ox2, oy2, of2), tuple(out[0]) + tuple(out[1]), (32 * cnt, 32 * cnt, cnt) * 2):
                    C.memmove(dst, np.ascontiguousarray(src, dtype=np.uint8).ctypes.data, n)
            return 0
        except Exception as e:  # noqa: BLE001
            wrapped.error = e
            return -1

    wrapped = LENET_ROUND_FN(cb)
    wrapped.error = None
    return wrapped


class Trace:
    """vpin_lenet_trace: per label the ConvTrace of its layer call (borrowed)"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def label(self, name):
        h = C.c_void_p()
        _chk(lib().vpin_lenet_trace_label(self.h, LABELS.index(name) + 1, C.byref(h)), "vpin_lenet_trace_label")
        t = ConvTrace(self.ctx, h)
        t.free = lambda: None  # borrowed: the Trace frees it
        return t

    def instances(self, name):
        hm, ha = C.c_void_p(), C.c_void_p()
        _chk(lib().vpin_lenet_trace_instances(self.ctx.h, self.h, LABELS.index(name) + 1, C.byref(hm), C.byref(ha)), "vpin_lenet_trace_instances")
        return (DevInstance(self.ctx, hm) if hm.value else None), (DevInstance(self.ctx, ha) if ha.value else None)

    def result(self):
        """the last layer's ciphertext -> (c1, c2), each (x, y, inf)"""
        x, y, f, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        _chk(lib().vpin_lenet_trace_result(self.h, C.byref(x), C.byref(y), C.byref(f), C.byref(n)), "vpin_lenet_trace_result")
        n = n.value
        get = lambda p, k: np.frombuffer((C.c_uint8 * k).from_address(p.value), dtype=np.uint8).copy()
        xs, ys, fs = get(x, 64 * n).reshape(2, n, 32), get(y, 64 * n).reshape(2, n, 32), get(f, 2 * n).reshape(2, n)
        return (xs[0], ys[0], fs[0]), (xs[1], ys[1], fs[1])

    def free(self):
        if self.h:
            lib().vpin_lenet_trace_free(self.h)
            self.h = None


def timings():
    out = (C.c_double * 16)()
    lib().vpin_lenet_last_timings(out)
    return dict(labels=[float(v) for v in out[0:7]], rounds=[float(v) for v in out[7:14]], total=float(out[14]))


def run(ctx, cfg, image_c1, image_c2, base_g, base_h, keys, bias_rs, round_fn, user=None):
    """vpin_lenet_infer -> Trace.  keys: 32-byte keys in call order; bias_rs: ints; round_fn: a LENET_ROUND_FN or a pointer"""
    x1, y1, f1 = ctx._points(*image_c1)
    x2, y2, f2 = ctx._points(*image_c2)
    k = np.frombuffer(b"".join(bytes(b) for b in keys), dtype=np.uint8).copy() if len(keys) else np.zeros(32, np.uint8)
    r = ctx._u256s(bias_rs) if len(bias_rs) else np.zeros(32, np.uint8)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = C.cast(round_fn, C.c_void_p)
    rc = lib().vpin_lenet_infer(ctx.h, C.byref(cfg.c), p(x1), p(y1), p(f1), p(x2), p(y2), p(f2), base_g, base_h, p(k), len(keys), p(r),
                                len(bias_rs), fn, user, C.byref(h))
    if rc:
        assert not h.value
        err, lib_text = getattr(round_fn, "error", None), lib().vpin_last_error().decode()
        if err is not None:  # the Python callback's own exception, with the round the driver names
            round_fn.error = None
            raise RuntimeError("the round callback raised [%s]" % lib_text) from err
        _chk(rc, "vpin_lenet_infer")
    return Trace(ctx, h)


def infer(ctx, cfg, client, image, image_rs, keys, bias_rs):
    """image: H x W ints (see preprocess).  Encrypts it under the client's key, runs the server loop against the ready-made
    client and returns (scores, rounds, trace): the N2 class scores, per round R1 .. R7 its (v, act), and the Trace"""
    c1, c2 = client.encrypt(np.asarray(image, dtype=np.int64).reshape(-1), image_rs)
    trace = run(ctx, cfg, c1, c2, client.base_g, client.base_h, keys, bias_rs, client.round_fn, client.user)
    rounds = [client.values(r) for r in range(1, 8)]
    return rounds[6][1], rounds, trace


def write_witness_files(trace, root):
    """the 7 x 8 JSON files the CLI reads, under root/rust_files/L1 .. L7"""
    from . import enc_conv
    for name in LABELS:
        enc_conv.write_witness_files(trace.label(name), root, name)
