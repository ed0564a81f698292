"""What a batch of B images through ONE inference (vpin_net_infer_batch) is, said twice: put together from B single runs, and as a
model of the batch driver on enc_conv_model's groups.  The rule is that a batch is byte for byte B single inferences, everything
image-major: the input and the keys and bias r are the images' own one after the other; a layer is one call over the planes
[b][half][plane], so its output, lists and left sides are the single runs' one after the other; a round is one callback over the
values of all images; the ready-made client consumes its queue of r stage by stage -- round 0 of all images, round 1 of all
images, .. (the input's r are handed to the encryption directly).  The layers' models, the groups and the client are imported from
net_model, convmc_model and fcs_model; nothing of them is restated.

Also here: the inputs of the batch tests (tests/test_gpu_net_batch.py, tests/test_gpu_net_batch_wire.py, tests/test_net_batch_model.py)
for the small trained network of fcs_model: per image a 10 x 10 crop of the reference's image, its own keys, bias r and client r."""
import convmc_model as CM
import elgamal_model as EL
import enc_conv_model as EM
import enc_fc_model as FM
import fcs_model as TM
import net_model as NM


# ---- a batch from its images' single runs -----------------------------------------------------------------------------------

def flat(per_image):
    """image-major: the images' own lists one after the other (points, keys, bias r, image r)"""
    return [v for one in per_image for v in one]


def stage_counts(cfg):
    """per round that encrypts again, the values of one image: what that round takes off the client's queue of r"""
    return [oC * oH * oW for l, (_, (oC, oH, oW)) in zip(cfg["layers"], CM.net_shapes(cfg)) if l.get("round") and l["round"]["reencrypt"]]


def client_queue(cfg, per_image_rs):
    """the batch's queue of r from the queues the images' single runs consume: stage after stage the r of all images"""
    out, pos = [], 0
    for n in stage_counts(cfg):
        for rs in per_image_rs:
            out += rs[pos:pos + n]
        pos += n
    assert all(len(rs) == pos for rs in per_image_rs)
    return out


def part(seq, b, B):
    """the b-th of B equal parts: image b's share of anything image-major"""
    n = len(seq) // B
    assert n * B == len(seq)
    return seq[b * n:(b + 1) * n]


def concat_rounds(per_image_rounds):
    """per round (v, act) over the whole batch from the images' own [(v, act)]"""
    return [tuple([x for rounds in per_image_rounds for x in rounds[r][i]] for i in range(2)) for r in range(len(per_image_rounds[0]))]


def concat_layers(per_image_layers):
    """per layer the model's dict of the one call over all images: out (planes), mults, adds and left of the images' own calls"""
    return [{k: [v for layers in per_image_layers for v in layers[i].get(k, [])] for k in ("out", "mults", "adds", "left")}
            for i in range(len(per_image_layers[0]))]


def concat_labels(labels):
    """the batch's label: the images' labels one after the other"""
    return dict(mults=[m for l in labels for m in l["mults"]], adds=[a for l in labels for a in l["adds"]])


# ---- the batch driver's model ---------------------------------------------------------------------------------------------------

def infer_batch_model(grp, cfg, c1, c2, keys, biases, client):
    """fcs_model.net_infer_model over B images in ONE call per layer and ONE round per round.  c1, c2: per image its C * H * W
    elements; keys: per image its keys in the order a single run consumes them; biases: per image, per layer that has one, (c1
    elements, c2 elements); client as for the single model, given the values of all images at once.  Returns (layers, label) with the
    layers as the one call's dicts and label = dict(mults, adds) in image order"""
    B = len(c1)
    keys, biases = [list(k) for k in keys], [list(b) for b in biases]
    take = lambda n: [k.pop(0) for k in keys for _ in range(n)]  # a step's keys of all images, image after image
    layers, rnd = [], 0
    for l, ((C, H, W), _) in zip(cfg["layers"], CM.net_shapes(cfg)):
        per = H * W
        planes = [c[b][p * per:(p + 1) * per] for b in range(B) for c in (c1, c2) for p in range(C)]  # [b][half][plane]
        if l["kind"] == "conv":
            res = EM.layer(grp, planes, H, W, l["filter"], l["fh"], l["fw"], l["pad"], l["stride"], take(2 * C), cfg["prf_bytes"])
        elif l["kind"] == "convmc":
            args = (grp, planes, C, l["n_out"], H, W, l["w"], l["connect"], l["fh"], l["fw"], l["pad"], l["stride"])
            if l.get("bias") is not None:
                bias = [v for one in biases for half in one.pop(0) for v in half]  # group g = 2 b + half
                res = TM.layer_bias(*args, bias, take(2 * l["n_out"]), cfg["prf_bytes"])
            else:
                res = CM.layer(*args, take(2 * l["n_out"]), cfg["prf_bytes"])
        elif l["kind"] == "pool":
            res = FM.avgpool(grp, planes, H, W, l["k"], l["stride"], l["scale"])
        else:
            rows = [list(c[b]) for b in range(B) for c in (c1, c2)]  # row 2 b: image b's c1 row
            bias = [list(half) for one in biases for half in one.pop(0)]
            res = (TM.fc_signed if l["kind"] == "fcs" else FM.fc)(grp, rows, C * H * W, l["w"], l["N"], bias, take(2), cfg["prf_bytes"])
        layers.append(res)
        planes_out = len(res["out"]) // B
        halves = [[[v for plane in res["out"][b * planes_out + h * planes_out // 2:b * planes_out + (h + 1) * planes_out // 2] for v in plane]
                   for b in range(B)] for h in range(2)]
        c1, c2 = halves
        if l.get("round"):
            r = l["round"]
            ans = client(rnd, r["relu"], r["shift_bits"], r["reencrypt"], flat(c1), flat(c2))
            rnd += 1
            if r["reencrypt"]:
                c1, c2 = ([part(a, b, B) for b in range(B)] for a in ans)
    assert not any(keys) and not any(biases)
    image_label = lambda b, key: [v for res in layers for v in part(res.get(key, []), b, B)]
    return layers, dict(mults=[m for b in range(B) for m in image_label(b, "mults")], adds=[a for b in range(B) for a in image_label(b, "adds")])


# ---- the inputs of the batch tests: the small trained network, an image, keys and r per b -----------------------------------------

CROPS = ((11, 11), (9, 13), (13, 8), (7, 16))  # (row, column) of image b's 10 x 10 crop of the reference's 32 x 32 image; 0: fcs_model's


def trained_images(B):
    full = NM.reference_image()
    out = [[int(v) for v in full[i:i + 10, j:j + 10].reshape(-1)] for i, j in CROPS[:B]]
    assert out[0] == [int(v) for v in TM.trained_image().reshape(-1)]
    return out


def trained_inputs(B):
    """per image b < B of the trained network: image, image_r, keys, bias_r, client_r, all seeded by b; image 0 has the inputs of
    tests/test_gpu_net_trained.py"""
    model = TM.trained_config()
    counts = TM.net_counts(model)
    seed = lambda base, b: base + 0x100 * b
    return dict(model=model, counts=counts, images=trained_images(B),
                image_r=[EL.splitmix_scalars(seed(0x7A1, b), 100) for b in range(B)],
                bias_r=[EL.splitmix_scalars(seed(0x7A2, b), counts["bias_r"]) for b in range(B)],
                client_r=[EL.splitmix_scalars(seed(0x7A3, b), counts["encryptions"] - 100) for b in range(B)],
                keys=[[NM.net_key(300 + 1000 * b + i) for i in range(counts["prf_keys"])] for b in range(B)])


# ---- the inputs of the unsigned kinds' batch: a pinned 8 x 8 case of net_pins.json and a seeded second image ----------------------

def pinned_inputs(pins, case):
    """B = 2 over the 8 x 8 network of `case` (CONV, POOL, FC, FC): image 0 is the pin's image under the pin's keys and r, image 1 a
    seeded image in the pin's value range under keys and r of its own"""
    model = NM.pinned_config(case, pins)
    counts = NM.counts(model)
    n = case["H"] * case["W"]
    lo, hi = min(v for row in case["image"] for v in row), max(v for row in case["image"] for v in row)
    hexes = lambda key: [int(r, 16) for r in case[key]]
    return dict(model=model, counts=counts, sk=int(pins["sk"], 16),
                images=[[v for row in case["image"] for v in row], [lo + r % (hi - lo + 1) for r in EL.splitmix_scalars(0x8B0, n)]],
                image_r=[hexes("image_r"), EL.splitmix_scalars(0x8B1, n)],
                bias_r=[hexes("bias_r"), EL.splitmix_scalars(0x8B2, counts["bias_r"])],
                client_r=[hexes("client_r"), EL.splitmix_scalars(0x8B3, counts["encryptions"] - n)],
                keys=[[bytes.fromhex(k) for k in case["keys"]], [NM.net_key(700 + i) for i in range(counts["prf_keys"])]])
