"""Python model of the wire format of an encrypted inference between two processes, on plain integers: a point of E2 packed
into 32 bytes (x, the parity of y, an identity bit), the square root in F_q that unpacking takes, and the 24-byte frame header.
E2 is y^2 = x^3 + a x + b over F_q with q = 5 (mod 8); its group order is prime and the only multiple of itself inside the Hasse
interval, so every point of the curve is in the group and unpacking needs no subgroup check.

A packed point is one 256-bit little-endian integer: bits 0 .. 252 the canonical x < q, bit 253 zero, bit 254 the identity (all
other bits zero then), bit 255 bit 0 of the canonical y."""
import struct

import gadgets_model as GM

Q = GM.Q
A, B = GM.E2_A, GM.E2_B
G = (GM.E2_GX, GM.E2_GY)

BIT_RESERVED, BIT_IDENTITY, BIT_PARITY = 1 << 253, 1 << 254, 1 << 255
X_MASK = (1 << 253) - 1
SQRT_EXP = (Q - 5) // 8  # Atkin's exponent: 250 bits, 71 of them set


class WireError(ValueError):
    """a rejection, with the rule in words the library's texts use too"""


def rhs(x):
    return (x * x * x + A * x + B) % Q


def sqrt(n):
    """a square root of n in F_q by Atkin's form for q = 5 (mod 8), or None: beta = (2 n)^((q - 5) / 8), i = 2 n beta^2 (a root of
    -1 when n is a square), y = n beta (i - 1); the root is never trusted unchecked"""
    n %= Q
    beta = pow(2 * n, SQRT_EXP, Q)
    i = 2 * n * beta * beta % Q
    y = n * beta * (i - 1) % Q
    return y if y * y % Q == n else None


def on_curve(P):
    return P is None or (0 <= P[0] < Q and 0 <= P[1] < Q and P[1] * P[1] % Q == rhs(P[0]))


def lift(x, parity=0):
    """the point over x whose y has that parity, or None when x is not on the curve"""
    y = sqrt(rhs(x))
    if y is None:
        return None
    return (x, y if (y & 1) == parity else Q - y)


def pack(P):
    """a point (None: the identity) -> 32 bytes"""
    if P is None:
        return BIT_IDENTITY.to_bytes(32, "little")
    if not on_curve(P):
        raise WireError("not on the curve E2")
    return (P[0] | ((P[1] & 1) << 255)).to_bytes(32, "little")


def unpack(b):
    """32 bytes -> a point (None: the identity); WireError names the rule"""
    v = int.from_bytes(bytes(b), "little")
    if v & BIT_IDENTITY:
        if v != BIT_IDENTITY:
            raise WireError("the identity bit is set together with other bits")
        return None
    if v & BIT_RESERVED:
        raise WireError("bit 253 is set")
    x = v & X_MASK
    if x >= Q:
        raise WireError("x is not below q")
    P = lift(x, v >> 255)
    if P is None:
        raise WireError("x is not on the curve E2")
    return P


# ---- frames --------------------------------------------------------------------------------------------------------------
MAGIC = b"VPW1"
HELLO, INPUT, ROUND, REPLY, DONE, ERROR = 1, 2, 3, 4, 5, 6
TYPES = (HELLO, INPUT, ROUND, REPLY, DONE, ERROR)
HEADER_LEN = 24
MAX_CNT = 1 << 24
MAX_ERROR_TEXT = 1024


def header(type_, flags=0, shift_bits=0, round_=0, cnt=0, payload_len=0, reserved=0, magic=MAGIC):
    return magic + struct.pack("<BBBBIIQ", type_, flags, shift_bits, reserved, round_, cnt, payload_len)


def payload_ok(type_, cnt, payload_len):
    """what the type and cnt imply for the payload"""
    if type_ == HELLO:
        return cnt == 1 and payload_len == 32
    if type_ in (INPUT, ROUND):
        return cnt >= 1 and payload_len == 64 * cnt
    if type_ == REPLY:
        return payload_len == 64 * cnt
    if type_ == DONE:
        return cnt == 0 and payload_len == 0
    return cnt == 0 and 4 <= payload_len <= 4 + MAX_ERROR_TEXT


def decode(b):
    """24 bytes -> dict; WireError names the rule, in the order the library checks them"""
    if len(b) != HEADER_LEN:
        raise WireError("a header is 24 bytes")
    if b[:4] != MAGIC:
        raise WireError("wrong magic")
    type_, flags, shift_bits, reserved, round_, cnt, payload_len = struct.unpack("<BBBBIIQ", b[4:])
    if type_ not in TYPES:
        raise WireError("unknown type")
    if reserved:
        raise WireError("the reserved byte is not zero")
    if cnt > MAX_CNT:
        raise WireError("cnt is above VPIN_WIRE_MAX_CNT")
    if not payload_ok(type_, cnt, payload_len):
        raise WireError("payload_len is not what the type and cnt imply")
    return dict(type=type_, flags=flags, shift_bits=shift_bits, round=round_, cnt=cnt, payload_len=payload_len)


def traffic(n_input, schedule):
    """bytes and frames each way for one inference: schedule = [(flags, shift_bits, cnt)] per round.  Client -> server: HELLO (one
    point), INPUT, a REPLY per round (an empty one where nothing is encrypted again); server -> client: a ROUND per round, DONE"""
    REENCRYPT = 2
    up_frames, up_cnt = 2 + len(schedule), n_input + sum(c for f, _, c in schedule if f & REENCRYPT)
    down_frames, down_cnt = len(schedule) + 1, sum(c for _, _, c in schedule)
    return dict(up_bytes=HEADER_LEN * up_frames + 64 * up_cnt + 32, up_frames=up_frames,
                down_bytes=HEADER_LEN * down_frames + 64 * down_cnt, down_frames=down_frames)
