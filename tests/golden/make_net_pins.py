#!/usr/bin/env python3
"""Pin the CNN A .. E inference to RUNS of the reference's own Python (src/cnn_networks/Server.py and Client.py), mechanically,
in the manner of make_layer_pins.py, whose stand-in curve, module loader and os.urandom / random.randrange queues it uses.

Run in the build container (the reference does not travel):

    python tests/golden/make_net_pins.py            # writes tests/golden/net_pins.json
    python tests/golden/make_net_pins.py --out F    # writes F instead

What it does.  On an 8 x 8 image it calls the server's functions in the order of inferenceCNN -- conv2_ciphertext,
avgPool_ciphertext, flattening, FC1, FC2 -- and between them the client's own decrypt_c1_c2, relu / shifting and
encryptFixedPointValue in the order of the client's main, once with the pooling (4, 4) and once with (2, 2), with
MultiCoreFeature = 0.  The fully connected weights are cut from version 1's files to K x 3 and 3 x 2.  It records the inputs,
the keys and r values in draw order, every round's decrypted and activated values, the final ciphertext and what the run left
in the four global lists.  The network's constants are read off the run or off the server's data: the filter from
weights_array, pad and stride from the arguments myConv2d was called with, the PRF bytes from pf against HMAC-SHA256
prefixes, the pooling scale from the caught return value, the pooling windows and weight files of the five versions from
KERNEL_STRIDE, MODEL_PATHS and VERSION_TO_FOLDER.  The schedule of the rounds (ReLU / shifting(., 26) / ReLU and
shifting(., 32) / ReLU) is what this script drives the client's functions with; it is recorded as "rounds".
The output holds inputs and recorded outputs only -- no reference text."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_layer_pins as LP  # noqa: E402

ROUNDS = [dict(relu=1, shift_bits=0), dict(relu=0, shift_bits=26), dict(relu=1, shift_bits=32), dict(relu=1, shift_bits=0)]
IMAGE_AT = (12, 12)  # the 8 x 8 crop of the preprocessed 32 x 32 image


def draw_key(label):
    return LP.hashlib.sha256(("net_pins/key/" + label).encode()).digest()


def draw_r(label, order):
    return int.from_bytes(LP.hashlib.sha256(("net_pins/r/" + label).encode()).digest(), "big") % (order - 2) + 1


def caught_calls(mod, fname):
    """like LP.caught, recording the arguments"""
    import contextlib

    @contextlib.contextmanager
    def cm():
        orig, seen = getattr(mod, fname), []

        def wrapper(*a, **kw):
            seen.append((a, kw))
            return orig(*a, **kw)

        setattr(mod, fname, wrapper)
        try:
            yield seen
        finally:
            setattr(mod, fname, orig)

    return cm()


def activate(client, values, rnd):
    a = values
    if rnd["relu"]:
        a = client.relu(a)
    if rnd["shift_bits"]:
        a = client.shifting(a, rnd["shift_bits"])
    return a


def ints(arr):
    return [int(v) for v in np.asarray(arr).reshape(-1)]


def case(pins, name, server, client, curve_info, sk, h, image, pool, weights):
    curve, q, order, G, identity = curve_info
    k, stride = pool
    w1f, b1f, w2f, b2f = weights
    H, W = image.shape
    rec = dict(name=name, H=H, W=W, pool=[k, stride], image=image.tolist(), keys=[], bias_r=[], client_r=[], rounds=[])
    rs = [draw_r("%s/image/%d" % (name, i), order) for i in range(H * W)]
    rec["image_r"] = ["%064x" % r for r in rs]
    with LP.deterministic(rs=rs, order=order):
        c1, c2 = client.encryptFixedPointValue(image.reshape(1, 1, H, W), curve, q, order, G, h, 0)
    rec["input"] = [pins.pids(c1.flatten()), pins.pids(c2.flatten())]

    def take_keys(n, what):
        ks = [draw_key("%s/%s/%d" % (name, what, i)) for i in range(n)]
        rec["keys"] += [x.hex() for x in ks]
        return ks

    def take_r(n, what, into):
        out = [draw_r("%s/%s/%d" % (name, what, i), order) for i in range(n)]
        rec[into] += ["%064x" % r for r in out]
        return out

    def interact(o1, o2, kind, expect):
        """the client's side of one round: decrypt (the table holds the baby steps of the expected values; a wrong expectation
        finds no entry and fails), activate, encrypt again unless it is the last round"""
        rnd = ROUNDS[len(rec["rounds"])]
        table, _ = LP.baby_table(G, expect, decoys=[1, 2, 3])
        with LP.deterministic():
            v = client.decrypt_c1_c2(sk, o1, o2, G, table, kind)
        assert ints(v) == [int(e) for e in expect], (name, len(rec["rounds"]))
        act = activate(client, v, rnd)
        last = len(rec["rounds"]) == len(ROUNDS) - 1
        rec["rounds"].append(dict(v=ints(v), act=ints(act)))
        if last:
            return None, None
        rs = take_r(np.asarray(act).size, "client/%d" % (len(rec["rounds"]) - 1), "client_r")
        with LP.deterministic(rs=rs, order=order):
            return client.encryptFixedPointValue(np.asarray(act), curve, q, order, G, h, kind)

    LP.clear_lists(server)
    with caught_calls(server, "myConv2d") as conv_calls, LP.caught(server, "realNumbersToFixedPointRepresentation") as fixed:
        with LP.deterministic(keys=take_keys(2, "conv")):
            o1, o2 = server.conv2_ciphertext(c1, c2, identity, q)
        taps = len(server.weights_array) // 2
        filt = np.array([int(w) for w in server.weights_array[:taps]], dtype=np.int64)
        a0, kw0 = conv_calls[0]
        pad, cstride = int(kw0["padding_size"]), int(kw0["stride"])
        fh, fw = (int(v) for v in a0[1].shape)
        assert fh * fw == taps and [int(v) for v in a0[1].flatten()] == filt.tolist()
        conv_plain = LP.plain_conv(image, filt.reshape(fh, fw), pad, cstride)
        e1, e2 = interact(o1, o2, 0, conv_plain.flatten().tolist())
        x = np.maximum(conv_plain, 0)

        n_fixed = len(fixed)
        with LP.deterministic():
            p1, p2 = server.avgPool_ciphertext(e1, e2, identity, k, stride)
            f1, f2 = server.flattening(p1, p2)
        scale = {int(s) for s in fixed[n_fixed:]}
        assert len(scale) == 1
        scale = scale.pop()
        oh, ow = (H - k) // stride + 1, (W - k) // stride + 1
        pooled = [scale * int(x[i * stride:i * stride + k, j * stride:j * stride + k].sum()) for i in range(oh) for j in range(ow)]
        e1, e2 = interact(f1, f2, 1, pooled)
        x = ints(rec["rounds"][1]["act"])

        K = len(x)
        w1, b1 = (w1f[:K] * 2**16).astype(np.int32), (b1f * 2**16).astype(np.int32)
        w2, b2 = (w2f * 2**16).astype(np.int32), (b2f * 2**16).astype(np.int32)
        for wf, bf, w, b, fn, what in ((w1f[:K], b1f, w1, b1, server.FC1, "fc1"), (w2f, b2f, w2, b2, server.FC2, "fc2")):
            N = len(b)
            rb = take_r(N, what + "/bias", "bias_r")
            with LP.deterministic(keys=take_keys(2, what), rs=rb, order=order):
                o1, o2 = fn(wf, bf, order, G, h, e1, e2, identity, q)
            expect = [sum(int(x[i]) * int(w[i][j]) for i in range(len(x))) + int(b[j]) for j in range(N)]
            e1, e2 = interact(o1, o2, 1, expect)
            x = ints(rec["rounds"][-1]["act"])
        rec["prf_bytes"] = LP.prf_bytes_of(server, draw_key("prf"))
    rec["result"] = [pins.pids(o1[0]), pins.pids(o2[0])]
    rec["conv"] = dict(fh=fh, fw=fw, pad=pad, stride=cstride, filter=filt.tolist())
    rec["pool_scale"] = scale
    rec["w1"], rec["b1"], rec["w2"], rec["b2"] = w1.tolist(), b1.tolist(), w2.tolist(), b2.tolist()
    rec.update(LP.read_lists(pins, server))
    LP.clear_lists(server)
    return rec


def main():
    out_path = os.path.join(HERE, "net_pins.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    LP.FILES = dict(cnn_server="src/cnn_networks/Server.py", cnn_client="src/cnn_networks/Client.py")
    mods, digests = LP.load_reference()
    server, client = mods["cnn_server"], mods["cnn_client"]
    server.MultiCoreFeature = 0
    curve, q, order, G, identity = client.curveE2Info()
    LP.self_check(curve, G, order)
    sk = draw_r("sk", order)
    with LP.deterministic(rs=[sk], order=order):
        info = client.keyGen()
    h = info[4]
    assert info[5] == sk
    curve_info = (curve, q, order, G, identity)

    model_dir = os.path.join(LP.REF, "src", "cnn_networks", "Pre_trained_model")
    load = lambda path: np.load(os.path.join(model_dir, os.path.basename(path)))
    v1 = server.MODEL_PATHS[1]
    weights = (load(v1["weight_fc1"])[:, :3], load(v1["bias_fc1"])[:3], load(v1["weight_fc2"])[:3, :2],
               load(os.path.join(model_dir, "bias_fc2_10.npy"))[:2])
    full = np.load(os.path.join(LP.REF, "src", "cnn_networks", "image_mnist_32_32.npy"))
    with LP.contextlib.redirect_stdout(LP.io.StringIO()):
        fixed = client.realNumbersToFixedPointRepresentation(client.min_max_scaling(full), 1, 16).reshape(32, 32)
    r0, c0 = IMAGE_AT
    image = np.array(fixed[r0:r0 + 8, c0:c0 + 8], dtype=np.int64)

    pins = LP.Pins()
    out = dict(about="recorded runs of the reference's own Python (tests/golden/make_net_pins.py); inputs and outputs only",
               multi_core_feature=0, reference_sha256=digests, sk="%064x" % sk, h=pins.pid(h), rounds=ROUNDS, image_at=list(IMAGE_AT))
    out["cases"] = [case(pins, "net_8x8_pool%d" % k, server, client, curve_info, sk, h, image, (k, k), weights) for k in (4, 2)]
    print("cases", file=sys.stderr)
    c0 = out["cases"][0]
    assert all(c["conv"] == c0["conv"] and c["prf_bytes"] == c0["prf_bytes"] for c in out["cases"])
    out["networks"] = {
        server.VERSION_TO_FOLDER[v]: dict(pool=[int(x) for x in server.KERNEL_STRIDE[v]],
                                          weight_fc1=os.path.basename(server.MODEL_PATHS[v]["weight_fc1"]),
                                          bias_fc1=os.path.basename(server.MODEL_PATHS[v]["bias_fc1"]),
                                          weight_fc2=os.path.basename(server.MODEL_PATHS[v]["weight_fc2"]), bias_fc2="bias_fc2_10.npy")
        for v in sorted(server.MODEL_PATHS)}
    out["network"] = dict(H=32, W=32, conv=c0["conv"], prf_bytes=c0["prf_bytes"], pool_scale_bits=10, weight_bits=16)
    for c in out["cases"]:
        assert c["pool_scale"] == int(2**10 / c["pool"][0]**2)
    out["points"] = pins.points

    txt = json.dumps(out, sort_keys=True, separators=(",", ":"))
    for key in ('"points":[', '"add_p":', '"add_r":', '"mult_points":', '"mult_weights":', '"input":', '"result":', '"image_r":',
                '"client_r":', '"cases":[', '"networks":', '"rounds":', '{"H":', '"keys":'):
        txt = txt.replace(key, "\n" + key)
    txt = txt.replace('"],["', '"],\n["')
    with open(out_path, "w") as f:
        f.write(txt + "\n")
    print("wrote %s: %d bytes, %d points" % (out_path, len(txt) + 1, len(pins.points)), file=sys.stderr)


if __name__ == "__main__":
    main()
