"""The wire format without a GPU: the model's packed points against fixed vectors and the curve's small x (tests/wire_model.py on
plain integers), the library's header codec against the model for every type and every rejection of vpin_wire_header_decode, and
two vpin_wire objects over a socketpair and over pipes: frames both ways, a peer that closes mid-header and mid-payload and a
silent peer, each VPIN_ECOMM with its text within a second and with the process alive."""
import os
import socket
import time

import pytest

import gadgets_model as GM
import wire_model as WM

Q = WM.Q
ON_CURVE_TO_36 = [0, 1, 2, 3, 4, 8, 9, 10, 12, 13, 15, 16, 25, 28, 31, 35, 36]


def test_pack_vectors():
    assert WM.G[1] % 2 == 0
    assert WM.pack(WM.G).hex() == "74a7eb7c9dce1e21936a3597795040247267cda53cba65f570abb33b6bfd150a"
    P0 = WM.lift(0, 0)
    assert P0 is not None and P0[1] * P0[1] % Q == WM.B and P0[1] % 2 == 0
    assert WM.pack(P0) == bytes(32)
    assert WM.pack((0, Q - P0[1])) == bytes(31) + b"\x80"
    assert WM.pack(None) == bytes(31) + b"\x40"
    assert WM.unpack(bytes(32)) == P0 and WM.unpack(bytes(31) + b"\x80") == (0, Q - P0[1]) and WM.unpack(bytes(31) + b"\x40") is None


def test_the_small_x_on_the_curve():
    assert Q % 8 == 5 and WM.SQRT_EXP.bit_length() == 250 and bin(WM.SQRT_EXP).count("1") == 71
    assert [x for x in range(37) if WM.lift(x) is not None] == ON_CURVE_TO_36
    assert WM.lift(Q - 1) is not None and WM.lift(Q - 2) is None
    for x in ON_CURVE_TO_36 + [Q - 1]:
        for par in (0, 1):
            P = WM.lift(x, par)
            assert WM.on_curve(P) and P[1] % 2 == par and WM.unpack(WM.pack(P)) == P


def test_round_trip_and_negation_on_multiples_of_g():
    P = None
    for _ in range(1, 33):
        P = GM.e2_add(P, WM.G)
        b, nb = WM.pack(P), WM.pack((P[0], Q - P[1]))
        assert WM.unpack(b) == P and WM.unpack(nb) == (P[0], Q - P[1])
        assert b[:31] == nb[:31] and b[31] ^ nb[31] == 0x80  # -P differs from P in bit 255 only


@pytest.mark.parametrize("v, rule", [
    (5, "not on the curve"), (6, "not on the curve"), (7, "not on the curve"), (Q - 2, "not on the curve"),
    (Q, "x is not below q"), (Q + 1, "x is not below q"), (1 | WM.BIT_RESERVED, "bit 253"),
    (WM.BIT_IDENTITY | 1, "identity bit"), (WM.BIT_IDENTITY | WM.BIT_PARITY, "identity bit")])
def test_unpack_rejections_of_the_model(v, rule):
    with pytest.raises(WM.WireError, match=rule):
        WM.unpack(v.to_bytes(32, "little"))
    with pytest.raises(WM.WireError, match="not on the curve"):
        WM.pack((1, 1))


# ---- the library's codec ---------------------------------------------------------------------------------------------------
FRAMES = [dict(type_=WM.HELLO, cnt=1, payload_len=32), dict(type_=WM.INPUT, cnt=100, payload_len=6400),
          dict(type_=WM.ROUND, flags=3, shift_bits=26, round_=4, cnt=9408, payload_len=64 * 9408),
          dict(type_=WM.REPLY, round_=4, cnt=9408, payload_len=64 * 9408), dict(type_=WM.REPLY, round_=6),
          dict(type_=WM.DONE), dict(type_=WM.ERROR, payload_len=4), dict(type_=WM.ERROR, payload_len=4 + 1024),
          dict(type_=WM.ROUND, flags=255, shift_bits=255, round_=2**32 - 1, cnt=WM.MAX_CNT, payload_len=64 * WM.MAX_CNT)]


@pytest.mark.parametrize("f", FRAMES, ids=lambda f: "type%d-%d" % (f["type_"], f.get("cnt", 0)))
def test_header_codec_is_the_models(f):
    from vpin_amd import wire as W
    b = W.header_encode(**f)
    assert b == WM.header(**f) and len(b) == W.HEADER_LEN == WM.HEADER_LEN
    assert W.header_decode(b) == WM.decode(b)
    assert W.header_decode(b) == dict(type=f["type_"], flags=f.get("flags", 0), shift_bits=f.get("shift_bits", 0), round=f.get("round_", 0),
                                      cnt=f.get("cnt", 0), payload_len=f.get("payload_len", 0))


BAD_HEADERS = [
    (WM.header(WM.DONE, magic=b"VPW2"), "wrong magic"), (WM.header(WM.DONE, magic=b"\0\0\0\0"), "wrong magic"),
    (WM.header(0), "unknown type 0"), (WM.header(7), "unknown type 7"), (WM.header(255), "unknown type 255"),
    (WM.header(WM.DONE, reserved=1), "the reserved byte is not zero"),
    (WM.header(WM.INPUT, cnt=WM.MAX_CNT + 1, payload_len=64 * (WM.MAX_CNT + 1)), "above VPIN_WIRE_MAX_CNT"),
    (WM.header(WM.ROUND, cnt=2**32 - 1, payload_len=64 * (2**32 - 1)), "above VPIN_WIRE_MAX_CNT"),
    (WM.header(WM.HELLO, cnt=1, payload_len=64), "payload_len 64 is not what type 1 and cnt 1 imply"),
    (WM.header(WM.HELLO, cnt=2, payload_len=32), "not what type 1 and cnt 2 imply"),
    (WM.header(WM.INPUT, cnt=2, payload_len=64), "not what type 2 and cnt 2 imply"),
    (WM.header(WM.INPUT, cnt=0, payload_len=0), "not what type 2 and cnt 0 imply"),
    (WM.header(WM.ROUND, cnt=1, payload_len=2**64 - 1), "not what type 3"),
    (WM.header(WM.REPLY, cnt=0, payload_len=1), "not what type 4"),
    (WM.header(WM.DONE, cnt=1), "not what type 5"), (WM.header(WM.DONE, payload_len=1), "not what type 5"),
    (WM.header(WM.ERROR, payload_len=3), "not what type 6"), (WM.header(WM.ERROR, payload_len=4 + 1025), "not what type 6"),
    (WM.header(WM.ERROR, cnt=1, payload_len=8), "not what type 6")]


@pytest.mark.parametrize("b, rule", BAD_HEADERS, ids=[str(i) for i in range(len(BAD_HEADERS))])
def test_every_decode_rejection_is_reached_and_named(b, rule):
    import vpin_amd
    from vpin_amd import wire as W
    with pytest.raises(WM.WireError):
        WM.decode(b)
    with pytest.raises(vpin_amd.VpinError, match=rule) as e:
        W.header_decode(b)
    assert e.value.code == -1 and "vpin_wire_header_decode" in str(e.value)


def test_encode_applies_the_same_rules():
    import vpin_amd
    from vpin_amd import wire as W
    with pytest.raises(vpin_amd.VpinError, match="vpin_wire_header_encode: payload_len"):
        W.header_encode(WM.INPUT, cnt=3, payload_len=64)
    with pytest.raises(vpin_amd.VpinError, match="unknown type"):
        W.header_encode(0)


# ---- the stream over descriptors ---------------------------------------------------------------------------------------------
def _socket_pair(timeout_ms=300):
    from vpin_amd import wire as W
    a, b = socket.socketpair()
    return (a, b), W.Wire.from_fds(a.fileno(), a.fileno(), timeout_ms), W.Wire.from_fds(b.fileno(), b.fileno(), timeout_ms)


def _pipe_pair(timeout_ms=300):
    from vpin_amd import wire as W
    r1, w1 = os.pipe()
    r2, w2 = os.pipe()
    return (r1, w1, r2, w2), W.Wire.from_fds(r1, w2, timeout_ms), W.Wire.from_fds(r2, w1, timeout_ms)


def _close(ends):
    for e in ends:
        try:
            e.close() if hasattr(e, "close") else os.close(e)
        except OSError:
            pass


@pytest.mark.parametrize("pair", [_socket_pair, _pipe_pair], ids=["socketpair", "pipes"])
def test_frames_both_ways(pair):
    ends, wa, wb = pair()
    points = bytes(range(64)) * 5
    wa.send(WM.HELLO, bytes(32), cnt=1)
    wa.send(WM.ROUND, points, flags=3, shift_bits=26, round_=2, cnt=5)
    assert wb.recv() == (dict(type=WM.HELLO, flags=0, shift_bits=0, round=0, cnt=1, payload_len=32), bytes(32))
    assert wb.recv() == (dict(type=WM.ROUND, flags=3, shift_bits=26, round=2, cnt=5, payload_len=320), points)
    wb.send(WM.REPLY, points[::-1], round_=2, cnt=5)
    wb.send(WM.REPLY, round_=3)
    wb.send_error(-5, "no such round")
    wb.send(WM.DONE)
    assert wa.recv()[1] == points[::-1] and wa.recv()[0]["payload_len"] == 0
    h, p = wa.recv()
    assert h["type"] == WM.ERROR and p == (-5).to_bytes(4, "little", signed=True) + b"no such round"
    assert wa.recv()[0]["type"] == WM.DONE
    up, down = 2 * 24 + 32 + 320, 4 * 24 + 320 + 4 + 13
    assert wa.stats() == dict(bytes_sent=up, bytes_received=down, frames_sent=2, frames_received=4)
    assert wb.stats() == dict(bytes_sent=down, bytes_received=up, frames_sent=4, frames_received=2)
    wa.free(); wb.free()
    _close(ends)


def test_a_frame_longer_than_the_buffer_is_refused_before_its_payload_is_read():
    import vpin_amd
    ends, wa, wb = _socket_pair()
    wa.send(WM.INPUT, bytes(128), cnt=2)
    with pytest.raises(vpin_amd.VpinError, match="longer than the buffer") as e:
        wb.recv(cap=64)
    assert e.value.code == -1
    wa.free(); wb.free()
    _close(ends)


def _raw_write(ends, b):
    """bytes from the second side without a Wire: its socket, or the write end of the pipe the first side reads"""
    ends[1].send(b) if hasattr(ends[1], "send") else os.write(ends[1], b)


def _close_peer(ends):
    """the second side goes away: its socket, or its pipe ends (w1 and r2)"""
    _close(ends[1:2] if hasattr(ends[1], "send") else ends[1:3])


def _fails_with_ecomm(wire_call, text):
    import vpin_amd
    t0 = time.monotonic()
    with pytest.raises(vpin_amd.VpinError, match=text) as e:
        wire_call()
    assert e.value.code == -7 and time.monotonic() - t0 < 1.0


@pytest.mark.parametrize("pair", [_socket_pair, _pipe_pair], ids=["socketpair", "pipes"])
def test_a_closed_or_silent_peer_is_ecomm_with_its_text(pair):
    # a silent peer: the time-out
    ends, wa, wb = pair(300)
    _fails_with_ecomm(wa.recv, "timed out after 300 ms waiting for the peer, after 0 of 24 bytes")
    wa.free(); wb.free()
    _close(ends)
    # closed mid-header
    ends, wa, wb = pair(300)
    raw = WM.header(WM.INPUT, cnt=2, payload_len=128)
    _raw_write(ends, raw[:17])
    wb.free()
    _close_peer(ends)
    _fails_with_ecomm(wa.recv, "the peer closed the stream after 17 of 24 bytes")
    wa.free()
    _close(ends)
    # closed mid-payload
    ends, wa, wb = pair(300)
    _raw_write(ends, raw + bytes(50))
    wb.free()
    _close_peer(ends)
    _fails_with_ecomm(wa.recv, "the peer closed the stream after 50 of 128 bytes")
    # and writing to the closed peer is an error return, never SIGPIPE: the process is still here to assert it
    _fails_with_ecomm(lambda: [wa.send(WM.INPUT, bytes(128), cnt=2) for _ in range(2)], "the peer closed the stream after 0 of 24 bytes were sent")
    wa.free()
    _close(ends)


def test_a_malformed_header_from_the_peer_is_einval_not_an_allocation():
    import vpin_amd
    ends, wa, wb = _socket_pair()
    ends[1].send(WM.header(WM.INPUT, cnt=2**32 - 1, payload_len=2**63))
    with pytest.raises(vpin_amd.VpinError, match="above VPIN_WIRE_MAX_CNT") as e:
        wa.recv()
    assert e.value.code == -1
    wa.free(); wb.free()
    _close(ends)


def test_create_rejections():
    import vpin_amd
    from vpin_amd import wire as W
    a, b = socket.socketpair()
    with pytest.raises(vpin_amd.VpinError, match="timeout_ms must be positive"):
        W.Wire.from_fds(a.fileno(), a.fileno(), 0)
    with pytest.raises(vpin_amd.VpinError, match="a descriptor is negative"):
        W.Wire.from_fds(-1, a.fileno(), 100)
    a.close(); b.close()


def test_traffic_of_the_model():
    # one round that encrypts again and one that does not, 100 inputs
    t = WM.traffic(100, [(3, 26, 50), (1, 0, 10)])
    assert t == dict(up_bytes=24 * 4 + 64 * 150 + 32, up_frames=4, down_bytes=24 * 3 + 64 * 60, down_frames=3)
