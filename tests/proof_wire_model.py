"""A model of the proof records that follow DONE on the inference stream (include/vpin_hip.h, "proofs over the wire"): the 40-byte
header, its rules, and the sizes a shape (is_mult, n_ops) allows, on plain integers.  The sizes are worked out here from the
gadgets' per-operation counts and the formulas of the commitment and the proof, not read from the library."""
import struct

PROOF, END, ERROR = 1, 2, 3
HEADER_LEN = 40
MAX_OPS = 1 << 24
MAX_TEXT = 1024
MAGIC = b"VPP1"

# one operation of a gadget: constraints, variables, entries of A, B, C (point_mult.rs at n = 128, point_addition.rs)
OP = {1: dict(cons=27 * 128 + 8, vars=27 * 128 + 10, nnz=(5260, 4488, 3201)), 0: dict(cons=10, vars=15, nnz=(16, 14, 10))}


class ProofWireError(ValueError):
    pass


def ceil_log2(n):
    return max(0, (n - 1).bit_length())


def dims(is_mult, n_ops):
    """padded num_cons, num_vars (Instance::new) and the entries of A, B, C"""
    op = OP[is_mult]
    cons, nvars = op["cons"] * n_ops, op["vars"] * n_ops + 1
    return (2 if cons <= 1 else 1 << ceil_log2(cons)), 1 << ceil_log2(nvars), tuple(k * n_ops for k in op["nnz"])


def rows(is_mult, n_ops):
    """the rows of comm_para and of comm_input, 32 bytes each"""
    return 1 << (ceil_log2(dims(is_mult, n_ops)[1]) // 2)


def _spark(is_mult, n_ops):
    nc, nv, nnz = dims(is_mult, n_ops)
    nx, ny = ceil_log2(nc), ceil_log2(2 * nv)
    lgN = max(ceil_log2(k) for k in nnz)
    return nc, nv, lgN, max(nx, ny)


def comm_bytes(is_mult, n_ops):
    """bincode(R1CSCommitment): six u64 and the row commitments of the ops and the mem polynomials"""
    _, _, lgN, lgM = _spark(is_mult, n_ops)
    return 48 + 8 + 32 * (1 << ((lgN + 4) // 2)) + 8 + 32 * (1 << ((lgM + 1) // 2))


def proof_max_bytes(is_mult, n_ops):
    nc, nv, lgN, lgM = _spark(is_mult, n_ops)
    lx, ly, ell = ceil_log2(nc), ceil_log2(2 * nv), ceil_log2(nv)
    b = 8 + 32 * (1 << (ell // 2)) + (lx + ly) * 400 + 2048 + 64 * (ell - ell // 2) + 96
    b += 8 + 32 * (1 << ((lgN + 3) // 2)) + 64 * 32
    b += lgN * (lgN * 104 + 64 + 24 * 32 + 64) + 18 * 32 + 64
    b += lgM * (lgM * 104 + 64 + 8 * 32 + 64) + 64
    b += 3 * (16 + 64 * 40 + 128 + 64) + 40 * 32 + 1024
    return b


def header(kind, is_mult=0, image=0, label=0, n_ops=0, proof_len=0, comm_len=0, magic=MAGIC, reserved=0):
    """the 40 bytes, whatever they say"""
    return magic + struct.pack("<BBHIIQQQ", kind, is_mult, reserved, image, label, n_ops, proof_len, comm_len)


def check(h):
    """the rules of both directions on a dict -> the name of the rule broken, or None"""
    if h["kind"] not in (PROOF, END, ERROR):
        return "unknown kind %d" % h["kind"]
    if h["kind"] == END:
        return "END: a field that must be zero is not" if any(h[k] for k in ("is_mult", "label", "n_ops", "proof_len", "comm_len")) else None
    if h["kind"] == ERROR:
        if any(h[k] for k in ("is_mult", "image", "label", "n_ops", "comm_len")):
            return "ERROR: a field that must be zero is not"
        return None if 4 <= h["proof_len"] <= 4 + MAX_TEXT else "ERROR: proof_len %d is outside" % h["proof_len"]
    if h["is_mult"] > 1:
        return "is_mult %d is above 1" % h["is_mult"]
    if not 1 <= h["n_ops"] <= MAX_OPS:
        return "n_ops %d is outside 1 .. VPIN_PROOF_MAX_OPS" % h["n_ops"]
    if h["proof_len"] > proof_max_bytes(h["is_mult"], h["n_ops"]):
        return "proof_len %d is above" % h["proof_len"]
    if h["comm_len"] != comm_bytes(h["is_mult"], h["n_ops"]):
        return "comm_len %d is not" % h["comm_len"]
    return None


def decode(b):
    """40 bytes -> dict, or ProofWireError naming the rule"""
    assert len(b) == HEADER_LEN
    if b[:4] != MAGIC:
        raise ProofWireError("wrong magic")
    kind, is_mult, reserved, image, label, n_ops, proof_len, comm_len = struct.unpack("<BBHIIQQQ", b[4:])
    h = dict(kind=kind, is_mult=is_mult, image=image, label=label, n_ops=n_ops, proof_len=proof_len, comm_len=comm_len)
    if kind in (PROOF, END, ERROR) and reserved:
        raise ProofWireError("the reserved bytes are not zero")
    why = check(h)
    if why:
        raise ProofWireError(why)
    return h


def payload_len(h):
    if h["kind"] == ERROR:
        return h["proof_len"]
    if h["kind"] != PROOF:
        return 0
    return h["proof_len"] + h["comm_len"] + 64 * rows(h["is_mult"], h["n_ops"])
