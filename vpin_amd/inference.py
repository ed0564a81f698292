"""What the two encrypted inferences over the C ABI share (vpin_amd.lenet, vpin_amd.net): the client's preprocessing, the
ready-made client (vpin_net_client_*), a round as a Python callback, the common part of their traces and the marshalling around
a `*_infer` call."""
import ctypes as C

import numpy as np

from .capi import LENET_ROUND_FN, ConvTrace, DevInstance, NetRoundPoolSpec, ProofExpect, VpinError, WireRoundSpec, _chk, lib

RELU, REENCRYPT, MAXPOOL = 1, 2, 4


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


class Client:
    """vpin_net_client: the key, the two base tables, the discrete-log table and the queue of randomness, for len(max_giant)
    rounds, which `values` counts from `first_round`"""
    first_round = 0

    def __init__(self, ctx, sk, nb, max_giant, rs):
        self.ctx, self.n_rounds = ctx, len(max_giant)
        h = C.c_void_p()
        k = ctx._u256s([sk])
        r = ctx._u256s(rs) if len(rs) else np.zeros(32, np.uint8)
        mg = (C.c_uint64 * len(max_giant))(*[int(v) for v in max_giant])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _chk(lib().vpin_net_client_create(ctx.h, p(k), nb, len(max_giant), mg, p(r), len(rs), C.byref(h)), "vpin_net_client_create")
        self.h = h
        g, hh = C.c_void_p(), C.c_void_p()
        _chk(lib().vpin_net_client_bases(h, C.byref(g), C.byref(hh)), "vpin_net_client_bases")
        self.base_g, self.base_h = g, hh
        self.round_fn = C.cast(lib().vpin_net_client_round, C.c_void_p)
        self.user = h

    def encrypt(self, msgs, rs):
        """the input's encryption under the client's key -> (c1, c2), each (x, y, inf)"""
        return self.ctx.e2_encrypt(self.base_g, self.base_h, msgs, rs)

    def run(self, wire, image, image_rs, schedule):
        """vpin_net_client_run: the client's endpoint over a vpin_amd.wire.Wire.  Encrypts the image (ints) under image_rs, sends
        HELLO and INPUT and serves the rounds of `schedule` ([(flags, shift_bits, cnt)], net.schedule) and no others -> (scores,
        rounds) as `infer` returns them"""
        m = np.ascontiguousarray(np.array([int(v) for v in np.asarray(image).reshape(-1)], dtype=np.int64))
        r = self.ctx._u256s(image_rs)
        assert len(image_rs) == m.shape[0]
        spec = (WireRoundSpec * max(1, len(schedule)))(*[WireRoundSpec(int(f), int(b), int(n)) for f, b, n in schedule])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _chk(lib().vpin_net_client_run(self.h, wire.h, p(m), p(r), m.shape[0], spec, len(schedule)), "vpin_net_client_run")
        rounds = [self.values(self.first_round + i) for i in range(len(schedule))]
        return rounds[-1][1], rounds

    def verify(self, wire, verifier, n_images, expectation, seed=None):
        """vpin_net_client_verify: behind DONE, the proofs of this client's n_images images off the wire, each record the next of
        `expectation` ([(label, is_mult, n_ops)], net.proof_expectation: the client's own, as the schedule is), its commitment the
        one `verifier` (net.Verifier) derives, all in one batch verification.  seed: 32 bytes, or None for the library's own
        randomness -> the verdicts [image][k] (True = accept).  A rejection raises nothing: `verifier.last_text` names the first"""
        spec = (ProofExpect * max(1, len(expectation)))(*[ProofExpect(int(l), int(m), int(n)) for l, m, n in expectation])
        ok = np.zeros(max(1, n_images * len(expectation)), np.uint8)
        sd = None if seed is None else np.frombuffer(bytes(seed), dtype=np.uint8).copy()
        assert sd is None or sd.size == 32
        rc = lib().vpin_net_client_verify(verifier.h, wire.h, n_images, spec, len(expectation), None if sd is None else sd.ctypes.data_as(C.c_void_p),
                                          ok.ctypes.data_as(C.c_void_p))
        if rc not in (0, -6):
            raise VpinError(rc, "vpin_net_client_verify")
        verifier.last_text = lib().vpin_last_error().decode(errors="replace") if rc else ""
        out = [[bool(v) for v in ok[i * len(expectation):(i + 1) * len(expectation)]] for i in range(n_images)]
        assert (rc == 0) == all(all(row) for row in out)
        return out

    def values(self, rnd):
        """(v, act) of round first_round .. first_round + n_rounds - 1 as int64 arrays; act is the shorter one of a round that pooled"""
        v, a, n, m = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _chk(lib().vpin_net_client_values(self.h, rnd - self.first_round, C.byref(v), C.byref(a), C.byref(n)), "vpin_net_client_values")
        _chk(lib().vpin_net_client_act_count(self.h, rnd - self.first_round, C.byref(m)), "vpin_net_client_act_count")
        get = lambda p, k: np.frombuffer((C.c_int64 * k).from_address(p.value), dtype=np.int64).copy() if k else np.zeros(0, np.int64)
        return get(v, n.value), get(a, m.value)

    def set_pools(self, pools):
        """vpin_net_client_set_pools: the client's own pooling schedule, per round (H, W, k, stride), all zero for a round that
        does not pool (net.pool_schedule).  A round whose VPIN_LENET_MAXPOOL flag disagrees with it is refused before anything
        is decrypted"""
        assert len(pools) == self.n_rounds
        spec = (NetRoundPoolSpec * max(1, len(pools)))(*[NetRoundPoolSpec(*[int(v) for v in p]) for p in pools])
        _chk(lib().vpin_net_client_set_pools(self.h, spec, len(pools)), "vpin_net_client_set_pools")
        return self

    def free(self):
        if self.h:
            lib().vpin_net_client_free(self.h)
            self.h = None


def python_round(fn):
    """a vpin_lenet_round_fn around fn(round, relu, reencrypt, shift_bits, c1, c2) -> (c1_out, c2_out) or None, the ciphertexts
    as (x, y, inf) numpy triples.  An exception must not unwind through the C frames: the callback returns VPIN_EINVAL, keeps
    the exception in `.error`, and `run_infer` raises it again once the driver has returned"""

    def cb(user, rnd, flags, bits, x1, y1, f1, x2, y2, f2, cnt, ox1, oy1, of1, ox2, oy2, of2):
        view = lambda p, n: np.frombuffer((C.c_uint8 * n).from_address(p), dtype=np.uint8)
        try:
            c1 = (view(x1, 32 * cnt).reshape(cnt, 32).copy(), view(y1, 32 * cnt).reshape(cnt, 32).copy(), view(f1, cnt).copy())
            c2 = (view(x2, 32 * cnt).reshape(cnt, 32).copy(), view(y2, 32 * cnt).reshape(cnt, 32).copy(), view(f2, cnt).copy())
            out = fn(rnd, bool(flags & RELU), bool(flags & REENCRYPT), bits, c1, c2)
            if flags & REENCRYPT:
                m = cnt
                if flags & MAXPOOL:  # a round that pools takes back the pooled count (vpin_net_round_pool)
                    shape = (C.c_size_t * 5)()
                    _chk(lib().vpin_net_round_pool(shape), "vpin_net_round_pool")
                    planes, H, W, k, stride = (int(v) for v in shape)
                    m = planes * ((H - k) // stride + 1) * ((W - k) // stride + 1)
                for dst, src, n in zip((ox1, oy1, of1, ox2, oy2, of2), tuple(out[0]) + tuple(out[1]), (32 * m, 32 * m, m) * 2):
                    C.memmove(dst, np.ascontiguousarray(src, dtype=np.uint8).ctypes.data, n)
            return 0
        except Exception as e:  # noqa: BLE001
            wrapped.error = e
            return -1

    wrapped = LENET_ROUND_FN(cb)
    wrapped.error = None
    return wrapped


class Trace:
    """what the traces of both drivers share; `prefix` is vpin_lenet_trace or vpin_net_trace"""
    prefix = None

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def _borrowed(self, h):
        t = ConvTrace(self.ctx, h)
        t.free = lambda: None  # borrowed: the Trace frees it
        return t

    def _instances(self, *label):
        hm, ha = C.c_void_p(), C.c_void_p()
        name = self.prefix + "_instances"
        _chk(getattr(lib(), name)(self.ctx.h, self.h, *label, C.byref(hm), C.byref(ha)), name)
        return (DevInstance(self.ctx, hm) if hm.value else None), (DevInstance(self.ctx, ha) if ha.value else None)

    images = 1

    def result_images(self):
        """the images whose ciphertexts result() holds"""
        return self.images

    def result(self):
        """the last layer's ciphertext -> (c1, c2), each (x, y, inf); of a batch, every array with the image in front"""
        x, y, f, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        _chk(getattr(lib(), self.prefix + "_result")(self.h, C.byref(x), C.byref(y), C.byref(f), C.byref(n)), self.prefix + "_result")
        n, b = n.value, self.result_images()
        get = lambda p, k: np.frombuffer((C.c_uint8 * k).from_address(p.value), dtype=np.uint8).copy()
        xs, ys, fs = get(x, 64 * n * b).reshape(b, 2, n, 32), get(y, 64 * n * b).reshape(b, 2, n, 32), get(f, 2 * n * b).reshape(b, 2, n)
        if b == 1:
            xs, ys, fs = xs[0], ys[0], fs[0]
            return (xs[0], ys[0], fs[0]), (xs[1], ys[1], fs[1])
        return (xs[:, 0], ys[:, 0], fs[:, 0]), (xs[:, 1], ys[:, 1], fs[:, 1])

    def free(self):
        if self.h:
            getattr(lib(), self.prefix + "_free")(self.h)
            self.h = None


def run_infer(name, ctx, cfg_c, c1, c2, base_g, base_h, keys, bias_rs, round_fn, user, batch=None, pubs=None, key_of_image=None, status=None):
    """`name` = vpin_lenet_infer or vpin_net_infer over the C configuration cfg_c -> the trace's handle.  c1, c2: (x, y, inf) of
    the input points; keys: 32-byte keys in call order; bias_rs: ints; round_fn: a LENET_ROUND_FN (python_round) or a pointer.
    batch: the B of vpin_net_infer_batch, which takes it behind the configuration; everything is then image-major.
    pubs: for vpin_net_infer_multi, which takes public keys [(x, y)] as Python ints and key_of_image[B] where the others take base_h.
    status: for vpin_net_infer_isolated, its array of B vpin_net_image_status in front of the trace"""
    x1, y1, f1 = ctx._points(*c1)
    x2, y2, f2 = ctx._points(*c2)
    k = np.frombuffer(b"".join(bytes(b) for b in keys), dtype=np.uint8).copy() if len(keys) else np.zeros(32, np.uint8)
    r = ctx._u256s(bias_rs) if len(bias_rs) else np.zeros(32, np.uint8)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = C.cast(round_fn, C.c_void_p)
    under = [base_h]
    if pubs is not None:
        hx, hy = ctx._u256s([x for x, _ in pubs]), ctx._u256s([y for _, y in pubs])
        ko = np.ascontiguousarray(np.array([int(v) for v in key_of_image], dtype=np.uint32))
        assert ko.shape[0] == batch
        under = [p(hx), p(hy), len(pubs), p(ko)]
    rc = getattr(lib(), name)(ctx.h, C.byref(cfg_c), *([] if batch is None else [batch]), p(x1), p(y1), p(f1), p(x2), p(y2), p(f2), base_g, *under,
                              p(k), len(keys), p(r), len(bias_rs), fn, user, *([] if status is None else [status]), C.byref(h))
    if rc:
        assert not h.value
        err, lib_text = getattr(round_fn, "error", None), lib().vpin_last_error().decode()
        if err is not None:  # the Python callback's own exception, with the round the driver names
            round_fn.error = None
            raise RuntimeError("the round callback raised [%s]" % lib_text) from err
        _chk(rc, name)
    return h


def infer(run, ctx, cfg, client, image, image_rs, keys, bias_rs):
    """Encrypts the image (ints, see preprocess) under the client's key, runs the module's `run` against the ready-made client
    and returns (scores, rounds, trace): the last round's activated values, per round its (v, act), and the Trace"""
    c1, c2 = client.encrypt(np.asarray(image, dtype=np.int64).reshape(-1), image_rs)
    trace = run(ctx, cfg, c1, c2, client.base_g, client.base_h, keys, bias_rs, client.round_fn, client.user)
    rounds = [client.values(client.first_round + r) for r in range(client.n_rounds)]
    return rounds[-1][1], rounds, trace
