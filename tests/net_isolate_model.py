"""What vpin_net_infer_isolated is, on the models: the batch driver (net_batch_model.infer_batch_model) with images that leave.
An image is named by its SLOT of the batch handed in; keys and biases stay indexed by slot.  A layer call runs over the live
slots; when the layers' models raise ShapeError the images that refuse are found by running the layer on every live image ALONE
(images do not interact, so an image refuses in the batch exactly when it refuses alone), they leave with a status, and the call
runs again over the others.  The client's callback is told the slots at hand and may name slots that leave after the round.
Nothing of the layers is restated: the calls go through infer_batch_model over one layer at a time.

Also here: the inputs of the refusal tests that the CPU and the GPU tests share (tests/test_net_isolate_model.py,
tests/test_gpu_net_isolate.py), chosen so that the models refuse only what is planted."""
import convmc_model as CM
import elgamal_model as EL
import enc_conv_model as EM
import net_batch_model as BM

ESHAPE = -5


def one_layer_cfg(cfg, i, dims):
    """the network that is layer i of cfg alone, without its round: what infer_batch_model runs for one layer call"""
    C, H, W = dims
    return dict(cfg, C=C, H=H, W=W, layers=[{k: v for k, v in cfg["layers"][i].items() if k != "round"}])


def layer_call(grp, cfg, i, dims, c1, c2, keys, biases):
    """layer i over the images given (per image its elements, its keys of this layer, its bias pair or None) -> the call's dict"""
    no_client = lambda *a: (_ for _ in ()).throw(AssertionError("a single layer has no round"))
    layers, _ = BM.infer_batch_model(grp, one_layer_cfg(cfg, i, dims), c1, c2, keys, [[b] if b is not None else [] for b in biases], no_client)
    return layers[0]


def infer_isolated_model(grp, cfg, c1, c2, keys, biases, client):
    """c1, c2, keys, biases per slot as for infer_batch_model.  client(slots, rnd, relu, shift_bits, reencrypt, c1, c2) ->
    ((c1, c2) or None, the slots that leave after the round).  Returns (calls, statuses): per layer dict(slots = the images of the
    call that succeeded, res = its dict), and per slot None or (code, layer, round, text)"""
    B = len(c1)
    live = list(range(B))
    c1, c2 = {b: list(c1[b]) for b in live}, {b: list(c2[b]) for b in live}
    status = [None] * B
    kpos, bpos, rnd, calls = 0, 0, 0, []
    for i, (l, ((C, H, W), _)) in enumerate(zip(cfg["layers"], CM.net_shapes(cfg))):
        n_keys = 2 * C if l["kind"] == "conv" else 2 * l["n_out"] if l["kind"] == "convmc" else 0 if l["kind"] == "pool" else 2
        has_bias = l["kind"] in ("fc", "fcs") or (l["kind"] == "convmc" and l.get("bias") is not None)
        call = lambda slots: layer_call(grp, cfg, i, (C, H, W), [c1[b] for b in slots], [c2[b] for b in slots],
                                        [keys[b][kpos:kpos + n_keys] for b in slots], [biases[b][bpos] if has_bias else None for b in slots])
        while True:
            try:
                res = call(live)
                break
            except EM.ShapeError as whole:
                refusing = {}
                for b in live:
                    try:
                        call([b])
                    except EM.ShapeError as e:
                        refusing[b] = str(e)
                if not refusing:
                    raise whole
                for b, text in refusing.items():
                    status[b] = (ESHAPE, i, -1, text)
                live = [b for b in live if b not in refusing]
                if not live:
                    raise EM.ShapeError("no image is left")
        kpos += n_keys
        bpos += 1 if has_bias else 0
        calls.append(dict(slots=list(live), res=res))
        planes = len(res["out"]) // len(live)
        for at, b in enumerate(live):
            mine = res["out"][at * planes:(at + 1) * planes]
            c1[b] = [v for plane in mine[:planes // 2] for v in plane]
            c2[b] = [v for plane in mine[planes // 2:] for v in plane]
        if l.get("round"):
            r = l["round"]
            ans, leaving = client(list(live), rnd, r["relu"], r["shift_bits"], r["reencrypt"], BM.flat([c1[b] for b in live]),
                                  BM.flat([c2[b] for b in live]))
            if r["reencrypt"]:
                for at, b in enumerate(live):
                    c1[b], c2[b] = BM.part(ans[0], at, len(live)), BM.part(ans[1], at, len(live))
            assert set(leaving) <= set(live)
            for b in leaving:
                status[b] = (ESHAPE, i, rnd, "dropped in the round")
            live = [b for b in live if b not in leaving]
            rnd += 1
            if not live:
                raise EM.ShapeError("no image is left")
    return calls, status


def image_part(call, b, key):
    """slot b's share of a layer call's out, mults, adds or left"""
    return BM.part(call["res"].get(key, []), call["slots"].index(b), len(call["slots"]))


# ---- the refusal lists: one call per layer kind with planted identities ----------------------------------------------------------

FCS_CASE = dict(P=4, K=2, N=2, W=[[3, -2], [-5, 7]], seed=0x150, identity_rows=(1, 3), prf_bytes=13)
CONV_CASE = dict(P=3, H=3, W=3, filt=[2, 3, 5, 7], f=2, seed=0x151, identity_planes=(1,), prf_bytes=13)
POOL_CASE = dict(P=3, H=2, W=2, k=2, scale=3, seed=0x152, first_pixel_identity=(2,))
CONVMC_CASE = dict(groups=4, C=1, n_out=1, H=3, W=3, f=2, w=[[[3, -2, 5, 7]]], seed=0x153, identity_groups=(2,), prf_bytes=13)


def case_logs(case, n, identity):
    """the case's n discrete logarithms (those of vpin_synthetic_points(seed, n)), 0 = the identity where `identity` says"""
    logs = EM.synthetic_logs(case["seed"], n)
    return [0 if identity(i) else k for i, k in enumerate(logs)]


def case_keys(n):
    import net_model as NM
    return [NM.net_key(1500 + i) for i in range(n)]


def fcs_case_logs():
    c = FCS_CASE
    x = case_logs(c, c["P"] * c["K"], lambda i: i // c["K"] in c["identity_rows"] and i % c["K"] == 0)
    bias = EM.synthetic_logs(c["seed"] + 0x1000, c["P"] * c["N"])
    return x, bias


def conv_case_logs():
    c = CONV_CASE
    per = c["H"] * c["W"]
    return case_logs(c, c["P"] * per, lambda i: i // per in c["identity_planes"])


def pool_case_logs():
    c = POOL_CASE
    per = c["H"] * c["W"]
    return case_logs(c, c["P"] * per, lambda i: i // per in c["first_pixel_identity"] and i % per == 0)


def convmc_case_logs():
    c = CONVMC_CASE
    per = c["C"] * c["H"] * c["W"]
    return case_logs(c, c["groups"] * per, lambda i: i // per in c["identity_groups"])


# ---- the two-round network of the drop tests: two signed FC layers 8 -> 4 -> 2 -------------------------------------------------------

def two_round_model():
    w1 = [[((3 * k + 5 * j) % 7) - 3 for j in range(4)] for k in range(8)]
    w2 = [[2, -1], [-3, 1], [1, 2], [-2, -2]]
    rnd = lambda relu, re: dict(relu=relu, shift_bits=0, reencrypt=re)
    return dict(C=1, H=2, W=4, prf_bytes=13, layers=[dict(kind="fcs", N=4, w=w1, bias=[5, -7, 0, 11], round=rnd(1, True)),
                                                     dict(kind="fcs", N=2, w=w2, bias=[-3, 4], round=rnd(0, False))])


TWO_ROUND_IMAGES = [[3, -50, 7, 9, 11, 13, 15, -17], [-4, 8, 21, -6, 10, 2, -30, 5], [1, 2, 3, 4, 5, 6, 7, 8], [9, -9, 8, -8, 7, -7, 6, 60]]
TWO_ROUND_SKS = [0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER, 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % EL.ORDER,
                 EL.ORDER - 1]


def two_round_inputs():
    """per slot b < 4 of the two-round network: image, image r, keys, bias r and the queue of r of the slot's client; sks: the keys
    of three clients (in process a client per image: slot b under sks[b])"""
    import net_model as NM
    return dict(model=two_round_model(), sks=TWO_ROUND_SKS, images=TWO_ROUND_IMAGES,
                image_r=[EL.splitmix_scalars(0x1600 + b, 8) for b in range(4)], bias_r=[EL.splitmix_scalars(0x1610 + b, 6) for b in range(4)],
                client_r=[EL.splitmix_scalars(0x1620 + b, 4) for b in range(4)], keys=[[NM.net_key(1600 + 10 * b + i) for i in range(4)] for b in range(4)])
