#!/usr/bin/env python3
"""Pin what joins the encrypted layers into the LeNet inference to RUNS of the reference's own Python, mechanically.

Run in the build container (the reference does not travel):

    python tests/golden/make_inference_pins.py            # writes tests/golden/inference_pins.json
    python tests/golden/make_inference_pins.py --out F    # writes F instead (tests/test_inference_pins.py compares the bytes)

In the manner of make_layer_pins.py, whose curve stand-in, module loader and randomness queues it imports: the reference's
src/LeNet/Server.py and src/LeNet/Client.py are loaded at run time and THEIR functions are called on small inputs:

  secondConv     6 planes of 6 x 6 -> 2 x 2, num_kernels_conv2 = 3 and = 16
  thirdConv      16 planes of 5 x 5 -> 1 x 1, its 120 kernels
  firstConv      2 kernels on a 6 x 6 image
  firstAvgPool   2 kernels on planes of 4 x 4
  relu, shifting (bits 26 and 33, values above 2^24, negative ones included), min_max_scaling,
  realNumbersToFixedPointRepresentation, all of Client.py

Recorded: the inputs, what the functions returned and what they left in the four global lists.  The connection table of
secondConv is READ OFF the run: the plane each callConv2_ciphertext call received is compared with the sums over every subset
of the input planes, and exactly one subset matches.  Nothing of the reference is restated.

To keep the file small the ciphertexts are stored as what they were encrypted from -- the message m and the randomness r of
every pixel, with a small key sk, so that (c1, c2) = (r G, (m + r sk) G) -- and every list of points as its length and a
SHA-256 over this serialisation:
  points   per point x then y, 32 bytes big-endian each; the identity as 64 zero bytes; concatenated in list order
  weights  the decimal strings joined by ","
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_layer_pins as L  # noqa: E402


def draw(label, count, lo, hi):
    return L.draw_small("inference_pins/" + label, count, lo, hi)


def point_bytes(P):
    return b"\0" * 64 if P.x() is None else int(P.x()).to_bytes(32, "big") + int(P.y()).to_bytes(32, "big")


def digest_points(seq):
    seq = list(seq)
    return dict(n=len(seq), sha256=hashlib.sha256(b"".join(point_bytes(P) for P in seq)).hexdigest())


def digest_weights(seq):
    seq = [str(int(w)) for w in seq]
    return dict(n=len(seq), sha256=hashlib.sha256(",".join(seq).encode()).hexdigest())


def read_lists(mod):
    return dict(mult_weights=digest_weights(mod.weights_array), mult_points=digest_points(mod.points_mult),
                add_p=digest_points(mod.point_one_Add), add_r=digest_points(mod.point_two_Add))


def encrypt_planes(client, curve_info, h, label, n, H, W, lo, hi):
    """n planes of H x W small messages under small r -> (messages, rs, c1 planes, c2 planes), the planes as the server holds
    them: 4-d object arrays (1, 1, H, W)"""
    order = curve_info[2]
    msgs = [draw("%s/m/%d" % (label, p), H * W, lo, hi) for p in range(n)]
    rs = [draw("%s/r/%d" % (label, p), H * W, 1, 2**20) for p in range(n)]
    c1, c2 = [], []
    for p in range(n):
        a, b = L.encrypt_image(client, curve_info, h, np.array(msgs[p], dtype=np.int64).reshape(1, 1, H, W), rs[p])
        c1.append(a)
        c2.append(b)
    assert order > 2**40
    return msgs, rs, c1, c2


class Recorded:
    """the arguments of every call of mod.fname while the reference's other functions call it"""

    def __init__(self, mod, fname):
        self.mod, self.fname, self.args = mod, fname, []

    def __enter__(self):
        self.orig = getattr(self.mod, self.fname)

        def wrapper(*a, **kw):
            self.args.append(a)
            return self.orig(*a, **kw)

        setattr(self.mod, self.fname, wrapper)
        return self.args

    def __exit__(self, *exc):
        setattr(self.mod, self.fname, self.orig)


def flat(planes):
    """a list of 4-d (1, 1, H, W) arrays -> the points plane-major, row-major"""
    return [P for pl in planes for P in np.asarray(pl, dtype=object).reshape(-1)]


def read_off_table(G, rs, sums_c1, n_in):
    """row o of the table: the one subset of the input planes whose c1 pixel (0, 0) sums to what conv call o received"""
    table = []
    for s in sums_c1:
        target = np.asarray(s, dtype=object).reshape(-1)[0]
        hits = [bits for bits in range(1, 1 << n_in)
                if G * (sum(rs[j][0] for j in range(n_in) if (bits >> j) & 1)) == target]
        assert len(hits) == 1, hits
        table.append([(hits[0] >> j) & 1 for j in range(n_in)])
    return table


def second_conv_case(mod, client, curve_info, h, planes, n2):
    _, q, order, G, identity = curve_info
    msgs, rs, c1, c2 = planes
    keys = [L.draw_key("inference_pins/second_conv/%d/%d" % (n2, i)) for i in range(2 * n2)]
    L.clear_lists(mod)
    with L.deterministic(keys=keys), Recorded(mod, "callConv2_ciphertext") as calls:
        o1, o2 = mod.secondConv(len(c1), n2, identity, q, c1, c2)
    assert len(calls) == 2 * n2 and len(o1) == n2 and len(o2) == n2
    sums = [a[0] for a in calls]  # c1 of row 0, c2 of row 0, c1 of row 1, ..
    out = [o for pair in zip(o1, o2) for o in pair]
    case = dict(n1=len(c1), n2=n2, H=6, W=6, keys=[k.hex() for k in keys], connect=read_off_table(G, rs, sums[0::2], len(c1)),
                sums=digest_points(flat(sums)), output=digest_points(flat(out)), call_order="row 0 c1, row 0 c2, row 1 c1, ..",
                **read_lists(mod))
    return case


def third_conv_case(mod, client, curve_info, h):
    _, q, order, G, identity = curve_info
    msgs, rs, c1, c2 = encrypt_planes(client, curve_info, h, "third_conv", 16, 5, 5, -40, 40)
    keys = [L.draw_key("inference_pins/third_conv/%d" % i) for i in range(240)]
    L.clear_lists(mod)
    with L.deterministic(keys=keys), Recorded(mod, "callConv2_ciphertext") as calls:
        o1, o2 = mod.thirdConv(16, 120, c1, c2, identity, q)
    assert len(calls) == 240 and o1.shape == (1, 120) and o2.shape == (1, 120)
    sums = [a[0] for a in calls]
    all16 = G * sum(rs[j][0] for j in range(16))  # every kernel takes all 16 planes: checked, not assumed
    assert all(np.asarray(s, dtype=object).reshape(-1)[0] == all16 for s in sums[0::2])
    return dict(n2=16, n3=120, H=5, W=5, messages=msgs, r=rs, keys_label="sha256('layer_pins/key/inference_pins/third_conv/<i>'), i = 0 .. 239",
                keys_sha256=hashlib.sha256(b"".join(keys)).hexdigest(), connect_all=True, sums=digest_points(flat(sums[:2])),
                output_c1=digest_points(o1.reshape(-1)), output_c2=digest_points(o2.reshape(-1)),
                call_order="kernel 0 c1, kernel 0 c2, kernel 1 c1, ..", **read_lists(mod))


def first_conv_case(mod, client, curve_info, h):
    _, q, order, G, identity = curve_info
    msgs, rs, c1, c2 = encrypt_planes(client, curve_info, h, "first_conv", 1, 6, 6, 0, 65535)
    keys = [L.draw_key("inference_pins/first_conv/%d" % i) for i in range(4)]
    L.clear_lists(mod)
    with L.deterministic(keys=keys):
        o1, o2 = mod.firstConv(2, c1[0], c2[0], identity, q)
    out = [o for pair in zip(o1, o2) for o in pair]
    return dict(kernels=2, H=6, W=6, messages=msgs[0], r=rs[0], keys=[k.hex() for k in keys], output=digest_points(flat(out)),
                call_order="kernel 0 c1, kernel 0 c2, kernel 1 c1, kernel 1 c2", **read_lists(mod))


def first_pool_case(mod, client, curve_info, h):
    _, q, order, G, identity = curve_info
    msgs, rs, c1, c2 = encrypt_planes(client, curve_info, h, "first_pool", 2, 4, 4, -500, 500)
    L.clear_lists(mod)
    with L.deterministic():
        o1, o2 = mod.firstAvgPool(2, identity, 2, 2, c1, c2)
    assert not mod.points_mult
    out = [o for pair in zip(o1, o2) for o in pair]
    return dict(kernels=2, H=4, W=4, k=2, stride=2, messages=msgs, r=rs, output=digest_points(flat(out)),
                call_order="kernel 0 c1, kernel 0 c2, kernel 1 c1, kernel 1 c2", add_p=digest_points(mod.point_one_Add),
                add_r=digest_points(mod.point_two_Add))


def shifting_inputs(bits):
    """values above 2^24 up to what int32 holds after the shift: ties of the rounding into float32 (to even, both ways), values
    one below a power of two (they round up and carry), drawn ones of every size in between, both signs"""
    top = 31 + bits - 16
    vals = [0, 1, -1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**26 - 1, 2**30 - 1, -(2**30 - 1), 2**(top - 1) - 1,
            -(2**(top - 1) - 1), 2**(top - 1), -(2**(top - 1)), 2**top - 2**(top - 24), -(2**top - 2**(top - 24))]
    for e in range(25, top - 1):
        for i, frac in enumerate(draw("shifting/%d/%d" % (bits, e), 3, 0, 2**24 - 1)):
            v = (1 << e) + (frac << (e - 24)) + (1 << (e - 25)) * (i % 2) + draw("shifting/%d/%d/lo" % (bits, e), 1, 0, 2**(e - 25) - 1)[0] * (i // 2)
            vals += [v, -v]
    return vals


def client_case(client):
    out = {}
    for bits in (26, 33):
        vals = shifting_inputs(bits)
        got = client.shifting(np.array(vals, dtype=np.float64), bits)
        assert got.dtype == np.int32 and all(float(v) == v for v in vals)
        out["shifting_%d" % bits] = dict(bits=bits, values=[str(v) for v in vals], results=[int(g) for g in got])
    rv = [0, 1, -1, 5, -2**30, 2**37, -(2**37), 123456789, -123456789]
    out["relu"] = dict(values=[str(v) for v in rv], results=[str(int(g)) for g in client.relu(np.array(rv, dtype=np.float64))])
    img = (np.array(draw("image", 16, 0, 4000), dtype=np.float32).reshape(1, 1, 4, 4) - np.float32(500.0)) / np.float32(1000.0)
    scaled = client.min_max_scaling(img)
    fixed = client.realNumbersToFixedPointRepresentation(scaled, 1, 16)
    assert scaled.dtype == np.float32 and fixed.dtype == np.int32
    out["preprocess"] = dict(shape=[4, 4], image_f32_le=img.astype("<f4").tobytes().hex(), scaled_f32_le=scaled.astype("<f4").tobytes().hex(),
                             fixed=[int(v) for v in fixed.reshape(-1)])
    return out


def main():
    out_path = os.path.join(HERE, "inference_pins.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    mods, digests = L.load_reference()
    lenet, client = mods["lenet_server"], mods["lenet_client"]
    lenet.MultiCoreFeature = 0
    curve, q, order, G, identity = client.curveE2Info()
    L.self_check(curve, G, order)
    sk = draw("sk", 1, 2**29, 2**30)[0]
    with L.deterministic(rs=[sk], order=order):
        info = client.keyGen()
    h = info[4]
    assert info[5] == sk
    curve_info = (curve, q, order, G, identity)

    out = dict(about="recorded runs of the reference's own Python (tests/golden/make_inference_pins.py); inputs and outputs only",
               serialisation="points: x then y, 32 bytes big-endian each, the identity 64 zero bytes, concatenated; weights: decimal "
                             "strings joined by ','; a list is stored as its length n and the SHA-256 of that",
               ciphertexts="pixel (m, r) is (c1, c2) = (r G, (m + r sk) G)", multi_core_feature=0, sk=sk,
               reference_sha256={k: v for k, v in digests.items() if "LeNet" in k})
    out["client"] = client_case(client)
    print("client", file=sys.stderr)
    planes = encrypt_planes(client, curve_info, h, "second_conv", 6, 6, 6, -300, 300)
    out["second_conv_input"] = dict(messages=planes[0], r=planes[1])
    out["second_conv"] = [second_conv_case(lenet, client, curve_info, h, planes, n2) for n2 in (3, 16)]
    print("second_conv", file=sys.stderr)
    out["first_conv"] = first_conv_case(lenet, client, curve_info, h)
    out["first_pool"] = first_pool_case(lenet, client, curve_info, h)
    print("first_conv, first_pool", file=sys.stderr)
    out["third_conv"] = third_conv_case(lenet, client, curve_info, h)
    L.clear_lists(lenet)

    txt = json.dumps(out, sort_keys=True, separators=(",", ":"))
    for key in ('"client":', '"second_conv":', '"second_conv_input":', '"first_conv":', '"first_pool":', '"third_conv":', '"messages":',
                '"r":', '"keys":', '"values":', '"results":', '"connect":'):
        txt = txt.replace(key, "\n" + key)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(txt + "\n")
    print("wrote %s: %d bytes" % (out_path, len(txt) + 1), file=sys.stderr)


if __name__ == "__main__":
    main()
