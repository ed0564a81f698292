"""Block sizes that fit one freed slot: on a context created with a CU mask every one-workgroup kernel of a proof (the sat
sum-checks' tail rounds, the resident tail of the product layers, the small eq tables, the tree tops) runs 256 threads, on
every other context its 512 or 1024.  Same field elements either way: whole SNARKs against tests/golden/config_digests.json
on both kinds of context, tail rounds against the CPU oracle on both, and a proof beside a row commitment on the same 64 CUs.

The SNARK sizes enter the resident tail with 1024 (3_32-mult), 512 (A-add), 256 (7_256-add) and fewer than 64 (3_32-add)
pairs per circuit: above, at and below the quad-lane threshold of a 256-thread workgroup (64 pairs) and with fewer live waves
than the workgroup has.

Tail rounds: a table of the C ABI has a power-of-two length (check_tabs, vpin_table_upload: VPIN_ESHAPE otherwise), so a tail
round has 512, 256, 128, .., 1 pairs and 257 or 65 pairs cannot be asked of the library; test_odd_lengths_are_refused pins that.
The chains below run every power of two from 512 down to 1 through each tail kernel: 512 is two full passes of a 256-thread
workgroup, 256 one, 128 and below leave waves without a pair.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O
import pymodel as M
from test_gpu_cumask import GOLD, SEED_C, SEED_P, _cus, _prove
from test_gpu_sumcheck import rand_table

pytestmark = pytest.mark.gpu
Q = M.Q
SHARED = (24, 32)  # the last 8 CUs of every XCD: 64 CUs, what bench.py's three small lanes share
KINDS = ("masked", "unmasked")


@pytest.fixture(scope="module")
def ctxs():
    import vpin_amd
    cs = {"masked": vpin_amd.Context(0, cu_mask=_cus(*SHARED)), "unmasked": vpin_amd.Context(0)}
    yield cs
    for c in cs.values():
        c.close()


# ---- whole SNARKs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["3_32-add", "3_32-mult", "A-add", "7_256-add"])
def test_snark_bytes_masked_and_unmasked(ctxs, key):
    got = {k: _prove(ctxs[k], key) for k in KINDS}
    assert got["masked"] == GOLD[key]["snark_sha256"], key
    assert got["unmasked"] == got["masked"], key


# ---- one tail round of each kernel, every power of two from 512 pairs down ----------------------------------------------

ELL = 11  # 2048 entries: the first round streams (1024 pairs), every later one is a tail round


@pytest.fixture(scope="module")
def tables4():
    rng = np.random.default_rng(2600)
    return [rand_table(rng, 1 << ELL, zero_frac=0.25 if k else 0.0) for k in range(4)], [rand_table(rng, 1)[0] for _ in range(ELL)]


@pytest.mark.parametrize("kind", KINDS)
def test_sc_tail4_rounds_vs_oracle(ctxs, tables4, kind):
    """sc_tail_kernel<4, false> (evaluate, fold apart) and sc_tail_kernel<4, true> (fused) at 512 .. 1 pairs"""
    ctx = ctxs[kind]
    host0, rs = tables4
    for fused in (False, True):
        host = [h.copy() for h in host0]
        dev = [ctx.upload(t) for t in host]
        n = 1 << ELL
        if fused:
            assert np.array_equal(ctx.sc_cubic_round(*dev), O.sc_cubic_round(*host))
        for j in range(ELL - 1 if fused else ELL):
            if not fused:
                assert np.array_equal(ctx.sc_cubic_round(*dev), O.sc_cubic_round(*host)), (kind, "eval", n // 2)
                ctx.sc_bind(dev, rs[j])
                host = [O.bound_top(t, rs[j]) for t in host]
            else:
                got = ctx.sc_cubic_bind_round(*dev, rs[j])
                host = [O.bound_top(t, rs[j]) for t in host]
                assert np.array_equal(got, O.sc_cubic_round(*host)), (kind, "fused", n // 4)
            n //= 2
            for t, h in zip(dev, host):
                assert len(t) == n and np.array_equal(t.read(), h), (kind, fused, n)
        for t in dev:
            t.free()


@pytest.mark.parametrize("kind", KINDS)
def test_sc_tail2_rounds_vs_oracle(ctxs, tables4, kind):
    """sc_tail_kernel<2, false> and <2, true> at 512 .. 1 pairs"""
    ctx = ctxs[kind]
    host0, rs = tables4
    for fused in (False, True):
        host = [h.copy() for h in host0[:2]]
        dev = [ctx.upload(t) for t in host]
        n = 1 << ELL
        for j in range(ELL - 1 if fused else ELL):
            if not fused:
                assert np.array_equal(ctx.sc_quad_round(*dev), O.sc_quad_round(*host)), (kind, "eval", n // 2)
                ctx.sc_bind(dev, rs[j])
                host = [O.bound_top(t, rs[j]) for t in host]
            else:
                got = ctx.sc_quad_bind_round(*dev, rs[j])
                host = [O.bound_top(t, rs[j]) for t in host]
                assert np.array_equal(got, O.sc_quad_round(*host)), (kind, "fused", n // 4)
            n //= 2
            for t, h in zip(dev, host):
                assert np.array_equal(t.read(), h), (kind, fused, n)
        for t in dev:
            t.free()


def _cubic3(L):
    vp = C.c_void_p
    L.vpin_eq_suffix_tables.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.vpin_sc_cubic3_round.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.vpin_sc_cubic3_bind_round.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.vpin_sc_cubic3_lead_round.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    return vp


@pytest.mark.parametrize("kind", KINDS)
def test_sc_tail3_rounds_vs_oracle(ctxs, tables4, kind):
    """sc_tail3_kernel in its four forms at 512 .. 1 pairs.  The plain form's three sums, scaled by the round's eq factors, are
    the oracle's four-table round.  The leading-coefficient form returns t(0), the x^2 coefficient c of the round's quadratic
    t(x) = a + b x + c x^2 and, in the first round, t(1).  With the plain sums S(x) = t(x) at x = 0, 2, 3: t(0) = S(0),
    6c = S(0) - 3 S(2) + 2 S(3), 2b = S(2) - S(0) - 4c and 2 t(1) = 2a + 2b + 2c."""
    import vpin_amd
    ctx = ctxs[kind]
    L = vpin_amd.lib()
    vp = _cubic3(L)
    _, rs = tables4
    rng = np.random.default_rng(2601)
    # start lengths chosen so that 512, 256, 64, 2 and 1 pairs are met by a FIRST round (no fold: t(1) is returned) and every
    # power of two from 512 down by a folding round (ell = 11: the first round streams 1024 pairs)
    for ell in (11, 10, 9, 7, 2, 1):
        n = 1 << ell
        tau = rand_table(rng, ell)
        host = [O.eq_evals(tau)] + [rand_table(rng, n, zero_frac=0.3) for _ in range(3)]
        dev = [ctx.upload(t) for t in host[1:]]
        lead = [t.clone() for t in dev]
        pyr = vp()
        assert L.vpin_eq_suffix_tables(ctx.h, tau.ctypes.data_as(vp), ell, C.byref(pyr)) == 0
        tau_i = M.table_to_ints(tau)
        s, r = 1, None
        for j in range(ell):
            out, lout = np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
            if j == 0:
                assert L.vpin_sc_cubic3_round(ctx.h, pyr, ell, 1, dev[0].h, dev[1].h, dev[2].h, out.ctypes.data_as(vp)) == 0
            else:
                assert L.vpin_sc_cubic3_bind_round(ctx.h, pyr, ell, j + 1, dev[0].h, dev[1].h, dev[2].h, r.ctypes.data_as(vp),
                                                   out.ctypes.data_as(vp)) == 0
                host = [O.bound_top(t, r) for t in host]
            assert L.vpin_sc_cubic3_lead_round(ctx.h, pyr, ell, j + 1, lead[0].h, lead[1].h, lead[2].h,
                                               r.ctypes.data_as(vp) if j else None, lout.ctypes.data_as(vp)) == 0
            S = M.table_to_ints(out)
            t = tau_i[j]
            got = [S[0] * s * (1 - t) % Q, S[1] * s * (3 * t - 1) % Q, S[2] * s * (5 * t - 2) % Q]
            assert got == M.table_to_ints(O.sc_cubic_round(*host)), (kind, ell, j)
            for d, ld, h in zip(dev, lead, host[1:]):
                assert np.array_equal(d.read(), h) and np.array_equal(ld.read(), h), (kind, ell, j)
            # t(x) = a + b x + c x^2 through S(0), S(2), S(3)
            Ld = M.table_to_ints(lout)
            c6 = (S[0] - 3 * S[1] + 2 * S[2]) % Q
            assert Ld[0] == S[0] and 6 * Ld[1] % Q == c6, (kind, ell, j)
            if j == 0:
                b2 = (S[1] - S[0] - 4 * Ld[1]) % Q  # 2b
                assert 2 * Ld[2] % Q == (2 * S[0] + b2 + 2 * Ld[1]) % Q, (kind, ell)
            r = rs[j]
            ri = M.table_to_ints(r.reshape(1, 4))[0]
            s = s * (t * ri + (1 - t) * (1 - ri)) % Q
        L.vpin_table_free(ctx.h, pyr)
        for t in dev + lead:
            t.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ell", [0, 3, 8, 9, 10, 12])
def test_eq_tables_and_pyramids_vs_oracle(ctxs, kind, ell):
    """eq_head_kernel (ell <= 9), eq_table_fused_kernel (from 10), eq_pyramid_top_kernel (ell <= 10) and
    eq_pyramid_fused_kernel (from 11) in both block sizes"""
    import vpin_amd
    ctx = ctxs[kind]
    L = vpin_amd.lib()
    vp = _cubic3(L)
    L.vpin_table_read.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    rng = np.random.default_rng(2700 + ell)
    tau = rand_table(rng, max(ell, 1))[:ell]
    t = ctx.eq_table(tau)
    exp = O.eq_evals(tau) if ell else np.array([M.to_mont_limbs(1)], dtype=np.uint64)
    assert np.array_equal(t.read(), exp)
    t.free()
    if ell == 0:
        return
    pyr = vp()
    assert L.vpin_eq_suffix_tables(ctx.h, tau.ctypes.data_as(vp), ell, C.byref(pyr)) == 0
    n = 1 << ell
    out = np.zeros((n, 4), dtype=np.uint64)
    assert L.vpin_table_read(ctx.h, pyr, 0, n, out.ctypes.data_as(vp)) == 0
    for k in range(1, ell + 1):
        off = n - (2 << (ell - k))
        lvl = O.eq_evals(tau[k:]) if k < ell else M.ints_to_table([1])
        assert np.array_equal(out[off:off + (1 << (ell - k))], lvl), (kind, ell, k)
    L.vpin_table_free(ctx.h, pyr)


def test_odd_lengths_are_refused(ctxs):
    """257 or 65 pairs would be tables of 514 or 130 entries: not a shape of the library"""
    import vpin_amd
    for n in (2 * 257, 4 * 257, 2 * 65, 4 * 65):
        with pytest.raises(vpin_amd.VpinError):
            ctxs["masked"].upload(np.zeros((n, 4), dtype=np.uint64))


# ---- a proof beside a row commitment on the same 64 CUs -----------------------------------------------------------------

ROWS = COLS = 2048  # 2^22 scalars


@pytest.fixture(scope="module")
def commitment():
    """a 2^22-scalar polynomial, its blinds, the generator stream and the oracle's 2048 row commitments.  One scalar in sixteen
    is of full length, the others are below 2^16 or zero (the oracle's bucket method skips zero digits: about a second)"""
    rng = np.random.default_rng(2622)
    pool_ints = [0] * 64 + [int(x) for x in rng.integers(1, 1 << 16, size=896)] + \
                [int.from_bytes(rng.bytes(32), "little") % Q for _ in range(60)] + [Q - 1, Q - 2, 1, 2]
    pool = M.ints_to_table(pool_ints)
    Z = np.ascontiguousarray(pool[rng.integers(0, len(pool_ints), size=ROWS * COLS)])
    blinds = M.ints_to_table([int.from_bytes(rng.bytes(32), "little") % Q for _ in range(ROWS)])
    xyzt, og = O.gens_stream_xyzt(COLS + 2)
    exp = O.hyrax_commit(Z, ROWS, blinds, og, COLS + 1, threads=16)
    return Z, blinds, xyzt, exp


def test_proof_beside_a_row_commitment_on_the_same_cus(commitment):
    """bench.py's step at its smallest: two contexts on the same 64-CU mask, one committing rows three workgroups to a CU, the
    other proving 3_32-add through its 256-thread tails.  No timing is asserted; both results are the oracle's."""
    import vpin_amd
    Z, blinds, xyzt, exp = commitment
    committer = vpin_amd.Context(0, cu_mask=_cus(*SHARED))
    prover = vpin_amd.Context(0, cu_mask=_cus(*SHARED))
    got, errs = {}, []
    try:
        g = committer.gens_shared("test_tail_block", xyzt, 2)
        dZ = committer.upload(Z)
        assert _prove(prover, "3_32-add") == GOLD["3_32-add"]["snark_sha256"]  # generators and tables of the proof are built
        go = threading.Barrier(2)

        def commit():
            try:
                go.wait()
                got["commit"] = [committer.hyrax_commit(g, dZ, blinds, COLS + 1) for _ in range(2)]
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))

        def prove():
            try:
                go.wait()
                got["proof"] = [_prove(prover, "3_32-add") for _ in range(3)]
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))

        ts = [threading.Thread(target=commit), threading.Thread(target=prove)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        dZ.free()
    finally:
        prover.close()
        committer.close()
    assert not errs, errs
    for c in got["commit"]:
        assert np.array_equal(c, exp)
    assert got["proof"] == [GOLD["3_32-add"]["snark_sha256"]] * 3
