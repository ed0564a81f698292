"""GPU parity: fixed-base window-table MSM / Hyrax commitment (HIP, through the C ABI) against
the CPU oracle's Pippenger on the same generators and scalars (bit-exact compressed points)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pymodel as M

pytestmark = pytest.mark.gpu
Q = M.Q


@pytest.fixture(scope="module")
def ctx():
    import vpin_amd
    c = vpin_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens34(ctx):
    xyzt, og = O.gens_stream_xyzt(34)  # R = 32 plus gens_1 base and h
    return ctx.gens_create(xyzt), og


def structured_scalars(rng, n):
    """witness-like mix: zeros, bits, small values, q-1, full-width"""
    vals = []
    for _ in range(n):
        k = rng.random()
        vals.append(0 if k < 0.35 else 1 if k < 0.45 else int(rng.integers(0, 2**16)) if k < 0.5
                    else Q - 1 if k < 0.53 else int(rng.integers(0, 2**62)) ** 4 % Q)
    return vals


def test_single_base_multiples(ctx, gens34):
    g, og = gens34
    L = O.lib()
    # k * g[0] for edge scalars, against the oracle's double-and-add
    for k in (1, 2, 127, 128, 129, 255, 256, 257, 2**128 + 129, Q - 1, Q - 128, (Q - 1) // 2):
        s = M.ints_to_table([k])
        got = ctx.gens_msm(g, s, 1, 1)
        exp = O.Ge()
        L.ge_scalarmul_bytes(C.byref(exp), (C.c_uint8 * 32)(*k.to_bytes(32, "little")), C.byref(og[0]))
        out = (C.c_uint8 * 32)()
        L.ge_compress(out, C.byref(exp))
        assert bytes(got[0]) == bytes(out), k


def test_all_zero_row_is_identity(ctx, gens34):
    g, _ = gens34
    got = ctx.gens_msm(g, np.zeros((32, 4), dtype=np.uint64), 1, 32)
    assert bytes(got[0]) == bytes(32)


@pytest.mark.parametrize("Ls,Rs", [(1, 32), (4, 32), (8, 16), (16, 4), (32, 1)])
def test_hyrax_commit_vs_oracle(ctx, gens34, Ls, Rs):
    g, og = gens34
    rng = np.random.default_rng(Ls * 100 + Rs)
    Z = M.ints_to_table(structured_scalars(rng, Ls * Rs))
    blinds = M.ints_to_table([int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)])
    dZ = ctx.upload(Z)
    got = ctx.hyrax_commit(g, dZ, blinds, 33)
    exp = O.hyrax_commit(Z, Ls, blinds, og, 33)
    assert np.array_equal(got, exp)


def test_commit_pair_and_homomorphism(ctx, gens34):
    """comm(para) + comm(input) == comm(para+input) under summed blinds
    (the assert at proof_point_mult.rs:69-73, for every row)."""
    g, og = gens34
    rng = np.random.default_rng(5)
    Ls, Rs = 4, 32
    a = structured_scalars(rng, Ls * Rs)
    b = structured_scalars(rng, Ls * Rs)
    ba = [int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)]
    bb = [int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)]
    Za, Zb = ctx.upload(M.ints_to_table(a)), ctx.upload(M.ints_to_table(b))
    ca, cb, cs = ctx.hyrax_commit_pair(g, Za, Zb, M.ints_to_table(ba), M.ints_to_table(bb), 33)
    assert np.array_equal(ca, O.hyrax_commit(M.ints_to_table(a), Ls, M.ints_to_table(ba), og, 33))
    assert np.array_equal(cb, O.hyrax_commit(M.ints_to_table(b), Ls, M.ints_to_table(bb), og, 33))
    Zs = ctx.upload(M.ints_to_table([(x + y) % Q for x, y in zip(a, b)]))
    cs2 = ctx.hyrax_commit(g, Zs, M.ints_to_table([(x + y) % Q for x, y in zip(ba, bb)]), 33)
    assert np.array_equal(cs, cs2)


def test_linearity_at_scale(ctx):
    """Size-independent property on a 256x256 commitment (conv-3 shape): commit(a*Z) row i equals
    a * commit(Z) row i -- checked through the oracle's scalar multiplication of the decompressed row."""
    xyzt, og = O.gens_stream_xyzt(258)
    g = ctx.gens_create(xyzt)
    rng = np.random.default_rng(8)
    Ls = Rs = 256
    vals = structured_scalars(rng, Ls * Rs)
    a = 0x1234567890ABCDEF1234567890ABCDEF
    Z1 = ctx.upload(M.ints_to_table(vals))
    Z2 = ctx.upload(M.ints_to_table([v * a % Q for v in vals]))
    zero_bl = np.zeros((Ls, 4), dtype=np.uint64)
    c1 = ctx.hyrax_commit(g, Z1, zero_bl, 257)
    c2 = ctx.hyrax_commit(g, Z2, zero_bl, 257)
    L = O.lib()
    for i in (0, 1, 77, 255):
        p = O.Ge()
        assert L.ge_decompress(C.byref(p), c1[i].ctypes.data_as(C.c_void_p)) == 1
        q = O.Ge()
        L.ge_scalarmul_bytes(C.byref(q), (C.c_uint8 * 32)(*a.to_bytes(32, "little")), C.byref(p))
        out = (C.c_uint8 * 32)()
        L.ge_compress(out, C.byref(q))
        assert bytes(out) == bytes(c2[i])
    # and three rows against the oracle's Pippenger directly
    exp = O.hyrax_commit(M.ints_to_table(vals[:3 * Rs]), 3, zero_bl[:3], og, 257)
    assert np.array_equal(c1[:3], exp)
    g.free()


def test_constant_rows_use_the_prefix_sum_base(ctx):
    """Rows of one repeated scalar (the padding tails of the SPARK polynomials) take the s * (g_0 + ... + g_{R-1})
    path; rows that only look constant at the probed positions, all-zero rows and ordinary rows do not.  All must
    match the oracle's Pippenger, with and without a blind."""
    Ls, Rs = 8, 256
    xyzt, og = O.gens_stream_xyzt(Rs + 2)
    g = ctx.gens_create(xyzt)
    rng = np.random.default_rng(21)
    s0 = int(rng.integers(1, 2**62)) ** 4 % Q
    rows = [
        [s0] * Rs,                                             # constant, full width
        [Q - 1] * Rs,                                          # constant, q - 1
        [1] * Rs,                                              # constant, one
        [0] * Rs,                                              # all zero
        [s0] * 7 + [s0 + 1] + [s0] * (Rs - 8),                 # passes the probes (0, 1, R/2, R-1), not constant
        [s0] * (Rs - 1) + [5],                                 # fails the last probe
        structured_scalars(rng, Rs),
        [2] * (Rs // 2) + [3] * (Rs // 2),
    ]
    Z = M.ints_to_table([v for r in rows for v in r])
    dZ = ctx.upload(Z)
    for blinds in (np.zeros((Ls, 4), dtype=np.uint64), M.ints_to_table([int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)])):
        got = ctx.hyrax_commit(g, dZ, blinds, Rs + 1)
        exp = O.hyrax_commit(Z, Ls, blinds, og, Rs + 1)
        assert np.array_equal(got, exp)
    g.free()


@pytest.mark.parametrize("budget_gb,bits,windows", [(1, 6, 43), (4, 7, 37), (10, 8, 32)])
def test_narrowest_windows_under_a_tiny_budget(ctx, budget_gb, bits, windows):
    """16386 generators under a table budget far below the 71 GB of 12-bit windows (a nearly full device: gens_build caps every
    table at a third of the free memory): 8-, 7- and 6-bit windows -- the narrowest, taken even when over budget -- give the
    oracle's bytes.  (Round 5: below the 7-bit table's 3.7 GB the layout said c = 6 with the 7-bit table's 37 windows of 64 entries.)"""
    Rs, Ls = 16384, 2
    xyzt, og = O.gens_stream_xyzt(Rs + 2)
    g = ctx.gens_shared(f"test_tiny_budget_{budget_gb}", xyzt, budget_gb)
    lay = (C.c_size_t * 6)()
    L = __import__("vpin_amd").lib()
    L.vpin_gens_layout.argtypes = [C.c_void_p, C.c_void_p]
    assert L.vpin_gens_layout(g.h, lay) == 0
    assert (lay[0], lay[1]) == (bits, windows), list(lay)
    rng = np.random.default_rng(budget_gb)
    vals = structured_scalars(rng, Ls * Rs)
    vals[:6] = [Q - 1, (Q - 1) // 2, 1 << 252, (1 << 252) - 1, 1, 0]
    Z = M.ints_to_table(vals)
    blinds = M.ints_to_table([int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)])
    dZ = ctx.upload(Z)
    got = ctx.hyrax_commit(g, dZ, blinds, Rs + 1)
    assert np.array_equal(got, O.hyrax_commit(Z, Ls, blinds, og, Rs + 1))
    assert np.array_equal(ctx.hyrax_commit_pippenger(g, dZ, blinds, Rs + 1), got)
    # a few-row MSM over the same table (the kernels that split a scalar's windows over lanes)
    s = M.ints_to_table(vals[:64])
    one = ctx.gens_msm(g, s, 1, 64)
    assert np.array_equal(one, O.hyrax_commit(s, 1, np.zeros((1, 4), dtype=np.uint64), og, Rs + 1))
    dZ.free()


def test_shared_device_hint_changes_nothing_but_occupancy(ctx, gens34):
    """vpin_ctx_set_shared_device only lowers the MSM's workgroups per CU: same commitment bytes"""
    g, og = gens34
    rng = np.random.default_rng(31)
    Ls, Rs = 4, 32
    Z = M.ints_to_table(structured_scalars(rng, Ls * Rs))
    blinds = M.ints_to_table([int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)])
    dZ = ctx.upload(Z)
    a = ctx.hyrax_commit(g, dZ, blinds, 33)
    ctx.set_shared_device(True)
    try:
        b = ctx.hyrax_commit(g, dZ, blinds, 33)
    finally:
        ctx.set_shared_device(False)
    assert np.array_equal(a, b) and np.array_equal(a, O.hyrax_commit(Z, Ls, blinds, og, 33))


def test_shape_errors(ctx, gens34):
    import vpin_amd
    g, _ = gens34
    Z = ctx.upload(np.zeros((64, 4), dtype=np.uint64))
    with pytest.raises(vpin_amd.VpinError) as ei:
        ctx.hyrax_commit(g, Z, np.zeros((1, 4), dtype=np.uint64), 33)  # R = 64 > 34 generators
    assert ei.value.code == -5


def test_commit_rows_blocks_equal_the_whole_commitment(ctx, gens34):
    """vpin_hyrax_commit_rows: any block of rows, with or without blinds, equals the same rows of vpin_hyrax_commit
    and of the oracle (the row split of vpin_amd/dist.py rests on this)"""
    import ctypes as C
    import vpin_amd
    L = vpin_amd.lib()
    L.vpin_hyrax_commit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
    g, og = gens34
    rng = np.random.default_rng(77)
    Ls, Rs = 16, 32
    Z = M.ints_to_table(structured_scalars(rng, Ls * Rs))
    blinds = M.ints_to_table([int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)])
    dZ = ctx.upload(Z)
    whole = ctx.hyrax_commit(g, dZ, blinds, 33)
    assert np.array_equal(whole, O.hyrax_commit(Z, Ls, blinds, og, 33))
    zero = np.zeros((Ls, 4), dtype=np.uint64)
    whole0 = O.hyrax_commit(Z, Ls, zero, og, 33)
    for row0, nrows in ((0, 16), (0, 4), (4, 4), (13, 3), (15, 1)):
        out = np.zeros((nrows, 32), dtype=np.uint8)
        b = np.ascontiguousarray(blinds[row0:row0 + nrows])
        assert L.vpin_hyrax_commit_rows(ctx.h, g.h, dZ.h, Ls, row0, nrows, b.ctypes.data_as(C.c_void_p), 33,
                                        out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, whole[row0:row0 + nrows]), (row0, nrows)
        assert L.vpin_hyrax_commit_rows(ctx.h, g.h, dZ.h, Ls, row0, nrows, None, 33, out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, whole0[row0:row0 + nrows]), (row0, nrows)
    out = np.zeros((4, 32), dtype=np.uint8)
    assert L.vpin_hyrax_commit_rows(ctx.h, g.h, dZ.h, Ls, 14, 4, None, 33, out.ctypes.data_as(C.c_void_p)) == -5  # rows past L
    assert L.vpin_hyrax_commit_rows(ctx.h, g.h, dZ.h, Ls, 0, 0, None, 33, out.ctypes.data_as(C.c_void_p)) == -1  # no rows


def test_table_write_roundtrip(ctx):
    t = ctx.alloc(64)
    a = M.ints_to_table(list(range(1, 17)))
    t.write(8, a)
    got = t.read()
    assert np.array_equal(got[8:24], a) and not got[:8].any() and not got[24:].any()
    import vpin_amd
    with pytest.raises(vpin_amd.VpinError):
        t.write(60, a)
    t.free()


def test_tables_in_128_byte_slots_give_the_same_commitments(ctx):
    """VPIN_TABLE_SLOT=128 (round 6; what bench.py asks for when every rank owns its GPU): the slot size is a property of a table,
    read when it is built.  A two-segment-free table of 2050 generators in 128-byte slots beside the default 96-byte ones: row
    commitments (table walk and buckets -- the bucket method reads multiple 1 of window 0), constant rows (prefix-sum bases) and a
    few-row MSM against the oracle's Pippenger, and against the same commitments from a 96-byte table."""
    import os
    Rs, Ls = 2048, 8
    xyzt, og = O.gens_stream_xyzt(Rs + 2)
    L = __import__("vpin_amd").lib()
    L.vpin_gens_entry_bytes.restype = C.c_size_t
    g96 = ctx.gens_shared("test_slot_96", xyzt, 2)
    os.environ["VPIN_TABLE_SLOT"] = "128"
    try:
        assert L.vpin_gens_entry_bytes() == 128
        g128 = ctx.gens_shared("test_slot_128", xyzt, 2)
    finally:
        del os.environ["VPIN_TABLE_SLOT"]
    assert L.vpin_gens_entry_bytes() == 96
    rng = np.random.default_rng(128)
    vals = structured_scalars(rng, Ls * Rs)
    vals[:6] = [Q - 1, (Q - 1) // 2, 1 << 252, (1 << 252) - 1, 1, 0]
    vals[3 * Rs:4 * Rs] = [vals[3 * Rs]] * Rs            # a constant row: s * (g_0 + ... + g_{R-1})
    Z = M.ints_to_table(vals)
    blinds = M.ints_to_table([int(rng.integers(0, 2**62)) ** 4 % Q for _ in range(Ls)])
    dZ = ctx.upload(Z)
    exp = O.hyrax_commit(Z, Ls, blinds, og, Rs + 1)
    for g in (g128, g96):
        assert np.array_equal(ctx.hyrax_commit(g, dZ, blinds, Rs + 1), exp)
        assert np.array_equal(ctx.hyrax_commit_pippenger(g, dZ, blinds, Rs + 1), exp)
        s = M.ints_to_table(vals[:64])
        one = ctx.gens_msm(g, s, 1, 64)
        assert np.array_equal(one, O.hyrax_commit(s, 1, np.zeros((1, 4), dtype=np.uint64), og, Rs + 1))
    dZ.free()
