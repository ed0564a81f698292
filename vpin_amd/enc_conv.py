"""The encrypted layers of vPIN's inference server over the C ABI (vpin_enc_conv2d, vpin_enc_conv2d_mc, vpin_enc_fc, vpin_enc_avgpool2d,
vpin_enc_add): ciphertext planes and a filter (or rows and a weight matrix, or a pooling window, or a second tensor) in, the output ciphertext and the two gadget
operation lists out -- as device instances for vpin_snark_prove_dev, or as the witness files the reference's Python service
writes, so that the unchanged CLI proves a real layer."""
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


def convmc_layer(ctx, groups, weights, connect, pad, stride, keys, prf_bytes=16):
    """The trained convolution layer (vpin_enc_conv2d_mc).  groups: a list of ciphertext images (the c1 and the c2 image, or batch
    elements), each (x, y, inf) with x, y of shape (C, H, W, 32) and inf of shape (C, H, W) or None; weights: n_out x C x fh x fw
    signed ints; connect: n_out x C (None: all connected); keys: one 32-byte key per (group, output channel), group-major.
    Returns the ConvTrace: groups * n_out output planes, group-major."""
    w = np.asarray(weights, dtype=np.int64)
    assert w.ndim == 4, "weights[o][c][ii][jj]"
    n_out, C_, fh, fw = w.shape
    parts = [_flat(g) for g in groups]
    shape = np.asarray(groups[0][0]).shape
    assert len(shape) == 4 and shape[0] == C_ and all(np.asarray(g[0]).shape == shape for g in groups), "groups of C planes of one H x W"
    x, y, inf = (np.concatenate([p[i] for p in parts]) for i in range(3))
    return ctx.enc_conv2d_mc(x, y, inf, len(groups), C_, n_out, shape[1], shape[2], w, connect, fh, fw, pad, stride, keys, prf_bytes)


def _flat(img):
    """(x, y, inf) of any leading shape -> x, y (n, 32) and inf (n)"""
    x, y, inf = img
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 32)
    y = np.ascontiguousarray(y, dtype=np.uint8).reshape(-1, 32)
    return x, y, (np.zeros(x.shape[0], np.uint8) if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1))


def fc_layer(ctx, c1, c2, weights, bias_c1, bias_c2, keys, prf_bytes=16):
    """c1, c2: the two ciphertext vectors, each (x, y, inf) with x, y of shape (K, 32); weights: K x N array-like of ints
    below 2^32; bias_c1, bias_c2: the encrypted bias, (x, y, inf) with x, y of shape (N, 32); keys: the c1 row's 32-byte
    key, then the c2 row's.  Returns the ConvTrace of vpin_enc_fc over the two rows."""
    rows, bias = [_flat(c1), _flat(c2)], [_flat(bias_c1), _flat(bias_c2)]
    w = np.asarray(weights, dtype=np.uint64)
    K, N = w.shape
    assert all(r[0].shape[0] == K for r in rows) and all(b[0].shape[0] == N for b in bias)
    cat = lambda parts, i: np.concatenate([p[i] for p in parts])
    return ctx.enc_fc(cat(rows, 0), cat(rows, 1), cat(rows, 2), 2, K, w, N, cat(bias, 0), cat(bias, 1), cat(bias, 2), keys, prf_bytes)


def avgpool_layer(ctx, c1, c2, k, stride, scale=None):
    """c1, c2 as for conv_layer: (x, y, inf) with x, y of shape (planes, H, W, 32).  scale defaults to the reference's
    fixed-point 1 / k^2 with 10 fractional bits.  Returns the ConvTrace of vpin_enc_avgpool2d, c1 planes first."""
    shape = np.asarray(c1[0]).shape
    assert len(shape) == 4 and np.asarray(c2[0]).shape[1:] == shape[1:], "planes of one H x W"
    parts = [_flat(c1), _flat(c2)]
    H, W = shape[1:3]
    x, y, inf = (np.concatenate([p[i] for p in parts]) for i in range(3))
    return ctx.enc_avgpool2d(x, y, inf, x.shape[0] // (H * W), H, W, k, stride, 2**10 // (k * k) if scale is None else scale)


def add_layer(ctx, first, second):
    """The addition layer (vpin_enc_add): out = first + second, point by point.  first, second: two encrypted tensors of one
    shape, each (x, y, inf) with x, y of shape (planes, H, W, 32) and inf of shape (planes, H, W) or None -- as the driver calls it,
    the C c1 planes and then the C c2 planes of each.  Returns the ConvTrace (Context.enc_add): additions only, no left sides"""
    shape = np.asarray(first[0]).shape
    assert len(shape) == 4 and np.asarray(second[0]).shape == shape, "two tensors of one planes x H x W"
    a, b = _flat(first), _flat(second)
    return ctx.enc_add(a[0], a[1], a[2], b[0], b[1], b[2], shape[0], shape[1], shape[2])


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
