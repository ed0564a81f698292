"""The encrypted convolution layer of vPIN's inference server over the C ABI (vpin_enc_conv2d): ciphertext planes and a
filter in, the output ciphertext and the two gadget operation lists out -- as device instances for vpin_snark_prove_dev, or
as the witness files the reference's Python service writes, so that the unchanged CLI proves a real layer."""
import json
import os

import numpy as np


def conv_layer(ctx, c1, c2, filt, pad, stride, keys, prf_bytes=16):
    """c1, c2: the two ciphertext images, each (x, y, inf) with x, y of shape (planes, H, W, 32) uint8 and inf of shape
    (planes, H, W) (None: no identity pixels).  The c1 planes are visited first, then the c2 planes; keys: one 32-byte key
    per plane in that order.  filt: 2-D array-like of ints < 2^128.  Returns the ConvTrace."""
    xs, ys, infs = [], [], []
    shape = None
    for x, y, inf in (c1, c2):
        x = np.ascontiguousarray(x, dtype=np.uint8)
        assert x.ndim == 4 and x.shape[3] == 32 and (shape is None or x.shape[1:3] == shape), "planes of one H x W"
        shape = x.shape[1:3]
        xs.append(x.reshape(-1, 32))
        ys.append(np.ascontiguousarray(y, dtype=np.uint8).reshape(-1, 32))
        infs.append(np.zeros(xs[-1].shape[0], np.uint8) if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1))
    H, W = shape
    x, y, inf = np.concatenate(xs), np.concatenate(ys), np.concatenate(infs)
    rows = [list(r) for r in filt]
    fh, fw = len(rows), len(rows[0])
    return ctx.enc_conv2d(x, y, inf, x.shape[0] // (H * W), H, W, [int(v) for r in rows for v in r], fh, fw, pad, stride, keys, prf_bytes)


def write_witness_files(trace, root, label):
    """The trace's two operation lists as the 8 JSON files of one label under root/rust_files/<label>/ (the format of
    vpin_amd.gadgets.write_witness_files, which the CLI reads)."""
    pa = os.path.join(root, "rust_files", label, "pointAdd")
    pm = os.path.join(root, "rust_files", label, "pointMult")
    os.makedirs(pa, exist_ok=True)
    os.makedirs(pm, exist_ok=True)
    px, py, rx, ry, rz = trace.adds()
    for name, a in (("px", px), ("py", py), ("rx", rx), ("ry", ry)):
        with open(os.path.join(pa, f"point_add_{name}_byte.json"), "w") as f:
            json.dump(a.tolist(), f)
    with open(os.path.join(pa, "point_add_rz_byte.json"), "w") as f:
        json.dump([int(v) for v in rz], f)
    w, x, y = trace.mults()
    with open(os.path.join(pm, "weight.json"), "w") as f:
        json.dump([str(v) for v in w], f)
    with open(os.path.join(pm, "point_mult_px_byte.json"), "w") as f:
        json.dump(x.tolist(), f)
    with open(os.path.join(pm, "point_mult_py_byte.json"), "w") as f:
        json.dump(y.tolist(), f)
