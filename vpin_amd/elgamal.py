"""The client side of vPIN's exponential ElGamal on E2 over the C ABI (vpin_e2_base_*, vpin_e2_encrypt[_keyed], vpin_e2_dlog_*,
vpin_e2_decrypt): key generation, batched encryption of signed integers and batched decryption with a discrete-log table that
stays in device memory.  Ciphertexts are the (x, y, inf) numpy triples the encrypted layers of vpin_amd.enc_conv take and
return, so a layer's output decrypts, goes through the caller's activation in numpy and is encrypted again for the next layer.
The randomness and the key are the caller's: explicit Python ints below the group order."""
import numpy as np

ORDER = 7237005577332262213973186563042994240704759454384003648147593987722918659549  # of E2's group (prime)
# 2^24 baby steps (0.8 GB): a value of the reference's range, +-2^35, is at most 2^11 giant steps away.  tools/time_e2_client.py
# measures the sizes
DEFAULT_NB = 1 << 24
DEFAULT_MAX_GIANT = 1 << 11


class BaseTable:
    """Window table of a fixed base point (None: the generator G); `point` = (x, y) as Python ints."""

    def __init__(self, ctx, point=None, w=None):
        self.ctx = ctx
        self.h = ctx.e2_base_create(None if point is None else point[0], None if point is None else point[1], w)

    def mul(self, scalars):
        """scalars[i] * B -> (x, y, inf)"""
        return self.ctx.e2_base_mul(self.h, scalars)

    def free(self):
        if self.h is not None:
            self.ctx.e2_base_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class DlogTable:
    """The baby steps j * G, 0 <= j < nb, in device memory."""

    def __init__(self, ctx, nb=DEFAULT_NB):
        self.ctx = ctx
        self.h = ctx.e2_dlog_create(nb)
        self.nb, self.device_bytes = ctx.e2_dlog_info(self.h)

    def solve(self, points, max_giant=DEFAULT_MAX_GIANT):
        """points: (x, y, inf) -> (v, found) with points[i] = v[i] * G, |v| <= max_giant * nb + nb - 1"""
        return self.ctx.e2_dlog_solve(self.h, points[0], points[1], points[2], max_giant)

    def free(self):
        if self.h is not None:
            self.ctx.e2_dlog_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def point_of(triple, i=0):
    """element i of an (x, y, inf) triple as (x, y) Python ints, or None for the identity"""
    x, y, inf = triple
    x, y = np.asarray(x).reshape(-1, 32), np.asarray(y).reshape(-1, 32)
    if np.asarray(inf).reshape(-1)[i]:
        return None
    return int.from_bytes(bytes(x[i]), "little"), int.from_bytes(bytes(y[i]), "little")


def keygen(base_g, sk):
    """the public key H = sk * G as (x, y) Python ints"""
    assert 0 < sk < ORDER
    return point_of(base_g.mul([sk]))


def encrypt(base_g, base_h, msgs, rs):
    """msgs: signed ints (any shape), rs: as many ints in 1 .. n - 1.  Returns (c1, c2), each (x, y, inf) with x, y of shape
    msgs.shape + (32,)"""
    m = np.asarray(msgs, dtype=np.int64)
    c1, c2 = base_g.ctx.e2_encrypt(base_g.h, base_h.h, m.reshape(-1), list(rs))
    shaped = lambda t: (t[0].reshape(m.shape + (32,)), t[1].reshape(m.shape + (32,)), t[2].reshape(m.shape))
    return shaped(c1), shaped(c2)


def encrypt_keyed(base_g, pubs, key_of, msgs, rs):
    """encrypt with a public key per element and no table of any H (vpin_e2_encrypt_keyed): pubs = [(x, y)] as Python ints (keygen),
    element i under pubs[key_of[i]]; msgs, rs and the result as for encrypt, key_of of msgs' shape"""
    m = np.asarray(msgs, dtype=np.int64)
    c1, c2 = base_g.ctx.e2_encrypt_keyed(base_g.h, list(pubs), np.asarray(key_of).reshape(-1), m.reshape(-1), list(rs))
    shaped = lambda t: (t[0].reshape(m.shape + (32,)), t[1].reshape(m.shape + (32,)), t[2].reshape(m.shape))
    return shaped(c1), shaped(c2)


def decrypt(table, sk, c1, c2, max_giant=DEFAULT_MAX_GIANT):
    """-> (values, found): int64 and bool arrays of the ciphertext's shape; found is False where the message lies outside
    +-(max_giant * nb + nb - 1)"""
    shape = np.asarray(c1[2]).shape if c1[2] is not None else np.asarray(c1[0]).shape[:-1]
    v, f = table.ctx.e2_decrypt(table.h, sk, c1, c2, max_giant)
    return v.reshape(shape), f.astype(bool).reshape(shape)
