"""The smallest network the LeNet architecture allows, for the tests of LeNet as a layer list (tests/test_net_lenet_cfg.py,
tests/test_gpu_net_lenet.py): a 2 x 2 filter over an 11 x 11 image, so 10 -> 5 -> 4 -> 2 -> 1 x 1; n1 = 2, n2 = 3 with the table
[[1,1],[0,1],[1,0]], n3 = 4, FC 4 -> 3 -> 2; pool scale 1 and the rounds' shifts chosen so that every decrypted value of the three
images stays within 2^16 baby steps times 64 giant steps (BOUND; the GPU test asserts it on the plaintext model first)."""
import hashlib

import elgamal_model as EL
import lenet_model as LM

NB, GIANT = 1 << 16, 64
BOUND = NB * GIANT
PRF = 13
CFG = dict(H=11, W=11, n1=2, n2=3, n3=4, connect=[[1, 1], [0, 1], [1, 0]], f=2, filter=[1, 2, 3, 1], pool_k=2, pool_stride=2, pool_scale=1,
           rounds=[(1, 0), (0, 17), (1, 0), (0, 18), (1, 20), (1, 19), (1, 0)], N1=3, N2=2)
W1 = [[1, 0, 3], [2, 1, 0], [0, 3, 1], [1, 1, 2]]
B1 = [-7000, 5, 1234]
W2 = [[1, 2], [3, 0], [0, 1]]
B2 = [-9, 10000]
COUNTS = LM.counts(CFG)
N_PIX = CFG["H"] * CFG["W"]


def image(b):
    """image b: small signed pixels, another pattern per image"""
    return [[((7 + 2 * b) * i * i + (3 + b) * j + i * j + 5 * b) % 17 - 8 for j in range(11)] for i in range(11)]


def keys(b):
    return [hashlib.sha256(b"tiny-lenet/key/%d/%d" % (b, i)).digest() for i in range(COUNTS["prf_keys"])]


def image_r(b):
    return EL.splitmix_scalars(0x2E10 + b, N_PIX)


def bias_r(b):
    return EL.splitmix_scalars(0x2E20 + b, COUNTS["bias_r"])


def client_r(b):
    """what image b's client draws in a run of its own: one r per value it encrypts again, R1 .. R6"""
    return EL.splitmix_scalars(0x2E30 + b, COUNTS["encryptions"] - N_PIX)


def batch_queue(bs):
    """the queue of one client that holds the images `bs` of a batch: round after round, image after image, each image's own r"""
    out, at = [], 0
    for n in COUNTS["per_round"][:-1]:
        for b in bs:
            out += client_r(b)[at:at + n]
        at += n
    return out


def make_cfg(VL, cfg=CFG, w1=W1, b1=B1, w2=W2, b2=B2, giants=None):
    """the vpin_amd.lenet.Config of a model dict"""
    f = cfg["f"]
    out = VL.Config([cfg["filter"][i * f:(i + 1) * f] for i in range(f)], cfg["connect"], w1, b1, w2, b2)
    out.c.H, out.c.W = cfg["H"], cfg["W"]
    out.set_pool(cfg["pool_k"], cfg["pool_stride"], cfg["pool_scale"])
    out.set_rounds(relu=[r[0] for r in cfg["rounds"]], shift_bits=[r[1] for r in cfg["rounds"]], max_giant=giants or [GIANT] * 7)
    return out
