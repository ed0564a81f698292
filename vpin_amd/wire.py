"""The byte stream of an encrypted inference between two processes over the C ABI (vpin_wire_*): frames of a 24-byte header and
packed points over two descriptors the caller owns -- pipes, a socketpair, a connected socket.  The library opens, listens on and
connects nothing; a Wire needs no context and no GPU.  `net.serve` and `net.Client.run` are the two endpoints.  Behind DONE the
same stream carries proof records (vpin_proof_*): a 40-byte header of their own, `Wire.send_proof` and `Wire.recv_proof`."""
import ctypes as C

import numpy as np

from .capi import ProofHeader, WireHeader, _chk, lib

HELLO, INPUT, ROUND, REPLY, DONE, ERROR = 1, 2, 3, 4, 5, 6
HEADER_LEN = 24
MAX_CNT = 1 << 24
MAX_TEXT = 1024


def header_encode(type_, flags=0, shift_bits=0, round_=0, cnt=0, payload_len=0):
    """vpin_wire_header_encode -> 24 bytes"""
    h = WireHeader(type_, flags, shift_bits, round_, cnt, payload_len)
    out = np.zeros(HEADER_LEN, np.uint8)
    _chk(lib().vpin_wire_header_encode(C.byref(h), out.ctypes.data_as(C.c_void_p)), "vpin_wire_header_encode")
    return bytes(out)


def header_decode(b):
    """vpin_wire_header_decode of 24 bytes -> dict"""
    buf = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    assert buf.size == HEADER_LEN
    h = WireHeader()
    _chk(lib().vpin_wire_header_decode(buf.ctypes.data_as(C.c_void_p), C.byref(h)), "vpin_wire_header_decode")
    return dict(type=h.type, flags=h.flags, shift_bits=h.shift_bits, round=h.round, cnt=h.cnt, payload_len=h.payload_len)


PROOF, PROOF_END, PROOF_ERROR = 1, 2, 3
PROOF_HEADER_LEN = 40
PROOF_MAX_OPS = 1 << 24
_PROOF_FIELDS = ("kind", "is_mult", "image", "label", "n_ops", "proof_len", "comm_len")


def gadget_sizes(is_mult, n_ops):
    """what bounds a proof record of that shape: dict(proof_max, comm, rows), rows those of comm_para and of comm_input"""
    L = lib()
    return dict(proof_max=int(L.vpin_gadget_proof_max_bytes(int(is_mult), n_ops)), comm=int(L.vpin_gadget_comm_bytes(int(is_mult), n_ops)),
                rows=int(L.vpin_gadget_vars_rows(int(is_mult), n_ops)))


def _proof_header(kind, is_mult=0, image=0, label=0, n_ops=0, proof_len=0, comm_len=0):
    return ProofHeader(kind, is_mult, image, label, n_ops, proof_len, comm_len)


def _proof_dict(h):
    return {k: int(getattr(h, k)) for k in _PROOF_FIELDS}


def proof_header_encode(kind, is_mult=0, image=0, label=0, n_ops=0, proof_len=0, comm_len=0):
    """vpin_proof_header_encode -> 40 bytes"""
    h = _proof_header(kind, is_mult, image, label, n_ops, proof_len, comm_len)
    out = np.zeros(PROOF_HEADER_LEN, np.uint8)
    _chk(lib().vpin_proof_header_encode(C.byref(h), out.ctypes.data_as(C.c_void_p)), "vpin_proof_header_encode")
    return bytes(out)


def proof_header_decode(b):
    """vpin_proof_header_decode of 40 bytes -> dict"""
    buf = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    assert buf.size == PROOF_HEADER_LEN
    h = ProofHeader()
    _chk(lib().vpin_proof_header_decode(buf.ctypes.data_as(C.c_void_p), C.byref(h)), "vpin_proof_header_decode")
    return _proof_dict(h)


def proof_payload_len(header):
    """the payload's bytes under a header (a dict as proof_header_decode gives it)"""
    h = _proof_header(**{k: header.get(k, 0) for k in _PROOF_FIELDS})
    return int(lib().vpin_proof_payload_len(C.byref(h)))


def split_proof_payload(header, payload):
    """a PROOF record's payload -> dict(proof, comm, comm_para, comm_input)"""
    n, c = header["proof_len"], header["comm_len"]
    half = (len(payload) - n - c) // 2
    return dict(proof=payload[:n], comm=payload[n:n + c], comm_para=payload[n + c:n + c + half], comm_input=payload[n + c + half:])


class Wire:
    """vpin_wire over two descriptors; closes neither"""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_fds(cls, rfd, wfd, timeout_ms):
        h = C.c_void_p()
        _chk(lib().vpin_wire_fd_create(rfd, wfd, timeout_ms, C.byref(h)), "vpin_wire_fd_create")
        return cls(h)

    def stats(self):
        out = (C.c_uint64 * 4)()
        _chk(lib().vpin_wire_stats(self.h, out), "vpin_wire_stats")
        return dict(bytes_sent=int(out[0]), bytes_received=int(out[1]), frames_sent=int(out[2]), frames_received=int(out[3]))

    def timings(self, slot):
        """host-clock ms this side spent in slot 0 (HELLO and INPUT) or 1 + r (round r): dict(pack, unpack, send, recv)"""
        out = (C.c_double * 4)()
        _chk(lib().vpin_wire_timings(self.h, slot, out), "vpin_wire_timings")
        return dict(zip(("pack", "unpack", "send", "recv"), (float(v) for v in out)))

    def send(self, type_, payload=b"", flags=0, shift_bits=0, round_=0, cnt=0):
        """one frame; payload_len is the payload's length"""
        p = np.frombuffer(bytes(payload), dtype=np.uint8).copy() if len(payload) else None
        h = WireHeader(type_, flags, shift_bits, round_, cnt, len(payload))
        _chk(lib().vpin_wire_send(self.h, C.byref(h), None if p is None else p.ctypes.data_as(C.c_void_p)), "vpin_wire_send")

    def recv(self, cap=1 << 20):
        """one frame -> (header dict, payload bytes)"""
        h = WireHeader()
        buf = np.zeros(max(cap, 1), np.uint8)
        _chk(lib().vpin_wire_recv(self.h, C.byref(h), buf.ctypes.data_as(C.c_void_p), cap), "vpin_wire_recv")
        return (dict(type=h.type, flags=h.flags, shift_bits=h.shift_bits, round=h.round, cnt=h.cnt, payload_len=h.payload_len),
                bytes(buf[:h.payload_len]))

    def send_proof(self, kind, payload=b"", is_mult=0, image=0, label=0, n_ops=0, proof_len=None, comm_len=0):
        """one proof record (vpin_proof_send); proof_len of an ERROR record defaults to the payload's length"""
        p = np.frombuffer(bytes(payload), dtype=np.uint8).copy() if len(payload) else None
        if proof_len is None:
            proof_len = len(payload) if kind == PROOF_ERROR else 0
        h = _proof_header(kind, is_mult, image, label, n_ops, proof_len, comm_len)
        if p is not None and len(payload) < int(lib().vpin_proof_payload_len(C.byref(h))):  # the library reads that many bytes
            raise ValueError("Wire.send_proof: the payload is shorter than the header says")
        _chk(lib().vpin_proof_send(self.h, C.byref(h), None if p is None else p.ctypes.data_as(C.c_void_p)), "vpin_proof_send")

    def recv_proof(self, cap=1 << 22):
        """one proof record -> (header dict, payload bytes); a payload above cap is VPIN_EINVAL and is not read"""
        h = ProofHeader()
        buf = np.zeros(max(cap, 1), np.uint8)
        _chk(lib().vpin_proof_recv(self.h, C.byref(h), buf.ctypes.data_as(C.c_void_p), cap), "vpin_proof_recv")
        return _proof_dict(h), bytes(buf[:int(lib().vpin_proof_payload_len(C.byref(h)))])

    def send_error(self, code, text):
        _chk(lib().vpin_wire_send_error(self.h, code, text.encode()), "vpin_wire_send_error")

    def free(self):
        if self.h:
            lib().vpin_wire_free(self.h)
            self.h = None
