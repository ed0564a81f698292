"""The whole encrypted LeNet inference over the C ABI (vpin_lenet_*): the server loop over the encrypted layers, the client's
rounds in between (decrypt, activation, encrypt again, one launch chain per round on the device) and the witness lists of the
seven labels L1 .. L7 for the prover.  An image goes in; the class scores, every round's values and the trace come out.

The network's constants are data, not code: `default_config` takes the filter and the connection table from the caller, or
reads them from the fixtures recorded off runs of the reference (tests/golden/layer_pins.json, inference_pins.json)."""
import ctypes as C
import json
import os

import numpy as np

from . import inference
from .capi import LenetCfg, _chk, lib
from .inference import RELU, REENCRYPT, fixed_point, min_max_scaling, preprocess, python_round  # noqa: F401  (one client protocol)

LABELS = ("L1", "L2", "L3", "L4", "L5", "L6", "L7")
_GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


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


class Client(inference.Client):
    """the ready-made client made for the seven rounds; `values(rnd)` counts them R1 .. R7, from 1"""
    first_round = 1

    def __init__(self, ctx, sk, nb, max_giant, rs):
        assert len(max_giant) == 7
        super().__init__(ctx, sk, nb, max_giant, rs)


class Trace(inference.Trace):
    """vpin_lenet_trace: per label the ConvTrace of its layer call (borrowed)"""
    prefix = "vpin_lenet_trace"

    def label(self, name):
        h = C.c_void_p()
        _chk(lib().vpin_lenet_trace_label(self.h, LABELS.index(name) + 1, C.byref(h)), "vpin_lenet_trace_label")
        return self._borrowed(h)

    def instances(self, name):
        return self._instances(LABELS.index(name) + 1)


def timings():
    out = (C.c_double * 16)()
    lib().vpin_lenet_last_timings(out)
    return dict(labels=[float(v) for v in out[0:7]], rounds=[float(v) for v in out[7:14]], total=float(out[14]))


def run(ctx, cfg, image_c1, image_c2, base_g, base_h, keys, bias_rs, round_fn, user=None):
    """vpin_lenet_infer -> Trace.  keys: 32-byte keys in call order; bias_rs: ints; round_fn: a LENET_ROUND_FN or a pointer"""
    return Trace(ctx, inference.run_infer("vpin_lenet_infer", ctx, cfg.c, image_c1, image_c2, base_g, base_h, keys, bias_rs, round_fn, user))


def infer(ctx, cfg, client, image, image_rs, keys, bias_rs):
    """image: H x W ints (see preprocess).  Encrypts it under the client's key, runs the server loop against the ready-made
    client and returns (scores, rounds, trace): the N2 class scores, per round R1 .. R7 its (v, act), and the Trace"""
    return inference.infer(run, ctx, cfg, client, image, image_rs, keys, bias_rs)


def infer_batch(ctx, cfg, client, images, image_rs, keys, bias_rs):
    """infer over B images at once: the layer list of `cfg` (net.from_lenet) through net.infer_batch, arguments and results as
    there.  The trace is a net.Trace: image b's label L(i + 1) is trace.image_layer(b, i)"""
    from . import net
    return net.infer_batch(ctx, net.from_lenet(cfg), client, images, image_rs, keys, bias_rs)


def write_witness_files(trace, root):
    """the 7 x 8 JSON files the CLI reads, under root/rust_files/L1 .. L7"""
    from . import enc_conv
    for name in LABELS:
        enc_conv.write_witness_files(trace.label(name), root, name)
