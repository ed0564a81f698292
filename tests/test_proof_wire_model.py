"""The proof records behind DONE without a GPU: the library's 40-byte header codec (vpin_proof_header_encode / _decode) against the
model of tests/proof_wire_model.py on good records and on every rejection, the sizes a shape allows against literal values, and
records over a socketpair with Wire.send_proof and Wire.recv_proof: both ways, a payload cut short, a buffer that is too small."""
import ctypes as C
import socket

import pytest

import proof_wire_model as PM

EINVAL, ECOMM = -1, -7

# (is_mult, n_ops) -> comm bytes, proof bytes at most, rows of comm_para / comm_input: what vpin_dev_instance_comm_bytes and
# vpin_dev_instance_proof_max_bytes report for the instances of these shapes (tests/test_gpu_net_proofs.py asserts that equality on
# the device): the small trained network's label (130 multiplications, 632 additions) and one multiplication
SIZES = {(1, 130): (163904, 222480, 512), (0, 632): (24640, 101544, 128), (1, 1): (12352, 87936, 64)}


def sized(kind, is_mult, n_ops, proof_len=None, **kw):
    """a record's fields with the shape's comm_len and, by default, its largest proof_len"""
    return dict(kind=kind, is_mult=is_mult, n_ops=n_ops, comm_len=PM.comm_bytes(is_mult, n_ops),
                proof_len=PM.proof_max_bytes(is_mult, n_ops) if proof_len is None else proof_len, **kw)


GOOD = [sized(PM.PROOF, 1, 130, 180000), sized(PM.PROOF, 0, 632, 0, image=3, label=7), sized(PM.PROOF, 1, 1, image=2**32 - 1, label=2**32 - 1),
        sized(PM.PROOF, 1, PM.MAX_OPS), sized(PM.PROOF, 0, PM.MAX_OPS, 1), sized(PM.PROOF, 0, 1), sized(PM.PROOF, 1, 130),
        dict(kind=PM.END), dict(kind=PM.END, image=14), dict(kind=PM.END, image=2**32 - 1),
        dict(kind=PM.ERROR, proof_len=4), dict(kind=PM.ERROR, proof_len=4 + 1024)]


@pytest.mark.parametrize("f", GOOD, ids=[str(i) for i in range(len(GOOD))])
def test_header_codec_is_the_models(f):
    from vpin_amd import wire as W
    b = W.proof_header_encode(**f)
    assert b == PM.header(**f) and len(b) == W.PROOF_HEADER_LEN == PM.HEADER_LEN == 40
    full = dict(dict(is_mult=0, image=0, label=0, n_ops=0, proof_len=0, comm_len=0), **f)
    assert W.proof_header_decode(b) == PM.decode(b) == full
    assert W.proof_payload_len(full) == PM.payload_len(full)


@pytest.mark.parametrize("shape", sorted(SIZES), ids=str)
def test_the_sizes_of_a_shape_are_the_recorded_ones(shape):
    from vpin_amd import capi
    from vpin_amd import wire as W
    comm, proof_max, rows = SIZES[shape]
    assert W.gadget_sizes(*shape) == dict(proof_max=proof_max, comm=comm, rows=rows)
    assert (PM.comm_bytes(*shape), PM.proof_max_bytes(*shape), PM.rows(*shape)) == SIZES[shape]
    # and what the prover's own size functions say of the shape vpin_gadget_shape counts by emitting an operation
    L = capi.lib()
    nc, nv, nnz = capi.gadget_shape("mult" if shape[0] else "add", shape[1])
    assert (nc, nv, tuple(nnz)) == PM.dims(*shape)
    r = capi.R1CS()
    r.num_cons, r.num_vars, r.num_inputs = nc, nv, shape[0]
    for m in range(3):
        r.nnz[m] = nnz[m]
    assert (L.vpin_spark_comm_bytes(C.byref(r)), L.vpin_snark_proof_max_bytes(C.byref(r))) == (comm, proof_max)


@pytest.mark.parametrize("is_mult", [0, 1])
def test_the_sizes_follow_the_emitted_operation_at_every_power_of_two(is_mult):
    from vpin_amd import capi
    from vpin_amd import wire as W
    for n in sorted({1, 2, 3, 5, 130, 632, PM.MAX_OPS} | {(1 << k) + d for k in range(1, 24, 3) for d in (-1, 0, 1)}):
        nc, nv, nnz = capi.gadget_shape("mult" if is_mult else "add", n)
        assert (nc, nv, tuple(nnz)) == PM.dims(is_mult, n), n
        assert W.gadget_sizes(is_mult, n) == dict(proof_max=PM.proof_max_bytes(is_mult, n), comm=PM.comm_bytes(is_mult, n), rows=PM.rows(is_mult, n)), n


C130, P130 = SIZES[1, 130][0], SIZES[1, 130][1]
BAD = [
    (PM.header(PM.END, magic=b"VPP2"), "wrong magic"), (PM.header(PM.END, magic=b"VPW1"), "wrong magic"),
    (PM.header(0), "unknown kind 0"), (PM.header(4), "unknown kind 4"), (PM.header(255, reserved=1), "unknown kind 255"),
    (PM.header(PM.END, reserved=1), "the reserved bytes are not zero"), (PM.header(PM.END, reserved=0x100), "the reserved bytes are not zero"),
    (PM.header(PM.PROOF, 2, n_ops=130, proof_len=1, comm_len=C130), "is_mult 2 is above 1"),
    (PM.header(PM.PROOF, 1, n_ops=0, comm_len=C130), "n_ops 0 is outside 1 .. VPIN_PROOF_MAX_OPS"),
    (PM.header(PM.PROOF, 1, n_ops=PM.MAX_OPS + 1, comm_len=C130), "n_ops 16777217 is outside 1 .. VPIN_PROOF_MAX_OPS"),
    (PM.header(PM.PROOF, 0, n_ops=2**64 - 1, proof_len=2**64 - 1, comm_len=2**64 - 1), "is outside 1 .. VPIN_PROOF_MAX_OPS"),
    (PM.header(PM.PROOF, 1, n_ops=130, proof_len=P130 + 1, comm_len=C130), "proof_len 222481 is above the 222480 bytes a proof of 130 multiplications can take"),
    (PM.header(PM.PROOF, 0, n_ops=632, proof_len=2**63, comm_len=24640), "is above the 101544 bytes a proof of 632 additions can take"),
    (PM.header(PM.PROOF, 1, n_ops=130, proof_len=1, comm_len=C130 - 1), "comm_len 163903 is not the 163904 bytes of the commitment of 130 multiplications"),
    (PM.header(PM.PROOF, 1, n_ops=130, proof_len=1, comm_len=PM.comm_bytes(1, 131) + 32), "comm_len"),
    (PM.header(PM.PROOF, 0, n_ops=130, proof_len=1, comm_len=C130), "is not the 10304 bytes of the commitment of 130 additions"),
    (PM.header(PM.END, is_mult=1), "END: a field that must be zero is not"), (PM.header(PM.END, label=1), "END: a field that must be zero is not"),
    (PM.header(PM.END, n_ops=1), "END: a field"), (PM.header(PM.END, proof_len=1), "END: a field"), (PM.header(PM.END, comm_len=1), "END: a field"),
    (PM.header(PM.ERROR, image=1, proof_len=8), "ERROR: a field that must be zero is not"), (PM.header(PM.ERROR, is_mult=1, proof_len=8), "ERROR: a field"),
    (PM.header(PM.ERROR, label=1, proof_len=8), "ERROR: a field"), (PM.header(PM.ERROR, n_ops=1, proof_len=8), "ERROR: a field"),
    (PM.header(PM.ERROR, comm_len=1, proof_len=8), "ERROR: a field"),
    (PM.header(PM.ERROR, proof_len=3), "ERROR: proof_len 3 is outside 4 .. 4 \\+ VPIN_WIRE_MAX_TEXT"),
    (PM.header(PM.ERROR, proof_len=4 + 1025), "ERROR: proof_len 1029 is outside")]


@pytest.mark.parametrize("b, rule", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_rejection_is_reached_and_named_by_decode_and_by_encode(b, rule):
    import struct

    import vpin_amd
    from vpin_amd import wire as W
    assert PM.comm_bytes(0, 130) == 10304  # 48 + 8 + 32 * 2^((12 + 4) / 2) + 8 + 32 * 2^((12 + 1) / 2)
    with pytest.raises(PM.ProofWireError):
        PM.decode(b)
    with pytest.raises(vpin_amd.VpinError, match=rule) as e:
        W.proof_header_decode(b)
    assert e.value.code == EINVAL and "vpin_proof_header_decode: " in str(e.value)
    if b[:4] != PM.MAGIC or "reserved" in rule:  # what a header struct cannot say
        return
    kind, is_mult, _, image, label, n_ops, proof_len, comm_len = struct.unpack("<BBHIIQQQ", b[4:])
    with pytest.raises(vpin_amd.VpinError, match=rule) as e:
        W.proof_header_encode(kind, is_mult, image, label, n_ops, proof_len, comm_len)
    assert e.value.code == EINVAL and "vpin_proof_header_encode: " in str(e.value)


# ---- records over a socketpair -------------------------------------------------------------------------------------------------
def _pair(timeout_ms=300):
    from vpin_amd import wire as W
    a, b = socket.socketpair()
    return (a, b), W.Wire.from_fds(a.fileno(), a.fileno(), timeout_ms), W.Wire.from_fds(b.fileno(), b.fileno(), timeout_ms)


def _close(ends, *wires):
    for w in wires:
        w.free()
    for e in ends:
        e.close()


SHAPE = (0, 4)  # four additions: a commitment of 1600 bytes and 8 rows on each side


def _record(proof_len=700, image=1, label=2):
    n = proof_len + PM.comm_bytes(*SHAPE) + 64 * PM.rows(*SHAPE)
    payload = bytes((7 * i + 3) % 251 for i in range(n))
    return dict(is_mult=SHAPE[0], n_ops=SHAPE[1], image=image, label=label, proof_len=proof_len, comm_len=PM.comm_bytes(*SHAPE)), payload


def test_records_both_ways_and_behind_frames():
    from vpin_amd import wire as W
    ends, wa, wb = _pair()
    f, payload = _record()
    assert (PM.comm_bytes(*SHAPE), PM.rows(*SHAPE), len(payload)) == (1600, 8, 700 + 1600 + 512)
    wa.send(W.DONE)  # the records follow DONE on the same stream
    wa.send_proof(W.PROOF, payload, **f)
    wa.send_proof(W.PROOF_END, image=1)
    wb.send_proof(W.PROOF_ERROR, (-5).to_bytes(4, "little", signed=True) + b"not the next record")
    assert wb.recv()[0]["type"] == W.DONE
    h, p = wb.recv_proof()
    assert h == dict(kind=W.PROOF, **f) and p == payload
    parts = W.split_proof_payload(h, p)
    assert [len(parts[k]) for k in ("proof", "comm", "comm_para", "comm_input")] == [700, 1600, 256, 256] and b"".join(parts.values()) == payload
    assert wb.recv_proof() == (dict(kind=W.PROOF_END, is_mult=0, image=1, label=0, n_ops=0, proof_len=0, comm_len=0), b"")
    h, p = wa.recv_proof()
    assert h["kind"] == W.PROOF_ERROR and h["proof_len"] == 23 and p == (-5).to_bytes(4, "little", signed=True) + b"not the next record"
    up, down = 24 + 2 * 40 + len(payload), 40 + 23
    assert wa.stats() == dict(bytes_sent=up, bytes_received=down, frames_sent=3, frames_received=1)
    assert wb.stats() == dict(bytes_sent=down, bytes_received=up, frames_sent=1, frames_received=3)
    _close(ends, wa, wb)


def test_a_truncated_payload_is_ecomm_with_the_byte_counts():
    import vpin_amd
    ends, wa, wb = _pair()
    f, payload = _record()
    ends[0].send(PM.header(PM.PROOF, **f) + payload[:1000])
    wa.free()
    ends[0].close()
    with pytest.raises(vpin_amd.VpinError, match="the peer closed the stream after 1000 of 2812 bytes") as e:
        wb.recv_proof()
    assert e.value.code == ECOMM
    wb.free()
    ends[1].close()
    # and cut inside the header
    ends, wa, wb = _pair()
    ends[0].send(PM.header(PM.PROOF, **f)[:33])
    wa.free()
    ends[0].close()
    with pytest.raises(vpin_amd.VpinError, match="the peer closed the stream after 33 of 40 bytes") as e:
        wb.recv_proof()
    assert e.value.code == ECOMM
    wb.free()
    ends[1].close()


def test_a_cap_below_the_payload_reads_no_payload():
    import vpin_amd
    ends, wa, wb = _pair()
    f, payload = _record()
    wa.send_proof(1, payload, **f)
    with pytest.raises(vpin_amd.VpinError, match="vpin_proof_recv: the record's payload is longer than the buffer") as e:
        wb.recv_proof(cap=f["proof_len"] - 1)
    assert e.value.code == EINVAL and wb.stats()["bytes_received"] == 40  # the header alone
    assert ends[1].recv(1 << 16) == payload  # the payload is still in the stream
    _close(ends, wa, wb)


def test_a_malformed_header_from_the_peer_is_einval_not_an_allocation():
    import vpin_amd
    ends, wa, wb = _pair()
    ends[0].send(PM.header(PM.PROOF, 1, n_ops=130, proof_len=2**62, comm_len=C130))
    with pytest.raises(vpin_amd.VpinError, match="proof_len 4611686018427387904 is above") as e:
        wb.recv_proof()
    assert e.value.code == EINVAL and wb.stats()["bytes_received"] == 40
    _close(ends, wa, wb)


def test_send_refuses_a_record_whose_payload_is_missing():
    import vpin_amd
    ends, wa, wb = _pair()
    f, _ = _record()
    with pytest.raises(vpin_amd.VpinError, match="vpin_proof_send: the record has a payload and none is given"):
        wa.send_proof(1, b"", **f)
    assert wa.stats()["bytes_sent"] == 0
    _close(ends, wa, wb)


def test_abi_version_and_symbols():
    from vpin_amd import capi
    from vpin_amd import net as VN
    L = capi.lib()
    assert L.vpin_abi_version() >= 10 and VN.STAGE_PROOFS == -5
    for name in ("vpin_proof_header_encode", "vpin_proof_header_decode", "vpin_proof_send", "vpin_proof_recv", "vpin_gadget_proof_max_bytes",
                 "vpin_gadget_comm_bytes", "vpin_net_send_proofs", "vpin_net_server_send_proofs", "vpin_net_verifier_create",
                 "vpin_net_verifier_shape", "vpin_net_verifier_stats", "vpin_net_client_verify"):
        assert hasattr(L, name), name
