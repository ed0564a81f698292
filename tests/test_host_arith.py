"""The host arithmetic (vpin_amd/csrc/host/field.h, curve.h and the UniPoly / eq / batch-inversion helpers of prover_common.h),
function by function through tests/hostarith/hostarith.cpp on the vectors of tests/host_vectors.py.  Host code on the CPU: no
test here needs a GPU.  Every comparison is exact, against Python integers (pymodel.py, pymodel_group.py); field elements are
compared as values AND as limb bounds.  tests/test_host_vectors.py asserts that the vectors reach the classes they are named
for.  The group and F_q vectors also go through the oracle's exported ge_* / fq_* functions: the oracle is the root of every
parity claim and its group code was pinned to the RFC vectors only.

VPIN_HOSTTEST_LIB runs the module against another build of the harness (a mutated copy of the headers: DESIGN.md 2.6)."""
import ctypes as C
import os
import subprocess

import pytest

import host_vectors as HV
import hostarith_lib as H
import oracle_lib as O
import pymodel_group as PG

P, Q = HV.P, HV.Q
GROUPS = HV.groups()


def _ids(prefixes):
    return [n for n in GROUPS if n.startswith(prefixes)]


def _run(name):
    grp = GROUPS[name]
    grp.check(H.run(grp.fn, grp.rows))


def test_the_harness_declares_what_the_vectors_use():
    tab = H.table()
    for name, grp in GROUPS.items():
        assert grp.fn in tab, name
        assert all(len(r) == tab[grp.fn][0] for r in grp.rows), name
    assert {g.fn for g in GROUPS.values()} == set(tab), "a function of the harness has no vectors"


@pytest.mark.parametrize("name", _ids("fq_"))
def test_fq(name):
    _run(name)


@pytest.mark.parametrize("name", _ids(("unipoly_", "combine_bot", "host_eq")))
def test_unipoly_eq_helpers(name):
    _run(name)


@pytest.mark.parametrize("name", _ids("fe_"))
def test_fe(name):
    _run(name)


def test_sqrt_ratio_m1():
    _run("sqrt_ratio_m1")


@pytest.mark.parametrize("name", _ids(("pt_add", "pt_dbl", "pt_equals", "pt_compress", "pt_decompress", "pt_from_uniform_bytes",
                                       "pt_elligator", "pt_to_xyzt", "pt_from_xyzt", "fb_add_niels")))
def test_point(name):
    _run(name)


def test_wnaf5_digits():
    _run("wnaf5")


@pytest.mark.parametrize("name", _ids(("pt_mul_bytes", "pt_mul2_bytes", "fb_mul_acc")))
def test_scalar_mul(name):
    _run(name)


# ---- the same vectors through the oracle ---------------------------------------------------------------------------------------
def _ofq(x):
    return O.fq_from_limbs(HV.words(x))


def test_oracle_fq_on_the_same_vectors():
    L = O.lib()
    L.fq_montgomery_reduce.restype = O.Fq
    for a, b in HV.FQ_PAIRS:
        fa, fb = _ofq(a), _ofq(b)
        assert L.fq_add(C.byref(fa), C.byref(fb)).limbs() == HV.words((a + b) % Q), (a, b)
        assert L.fq_sub(C.byref(fa), C.byref(fb)).limbs() == HV.words((a - b) % Q), (a, b)
        assert L.fq_mul(C.byref(fa), C.byref(fb)).limbs() == HV.words(a * b * HV.RINV % Q), (a, b)
    for a in HV.FQ_VALUES:
        fa = _ofq(a)
        assert L.fq_neg(C.byref(fa)).limbs() == HV.words(-a % Q)
        assert L.fq_square(C.byref(fa)).limbs() == HV.words(a * a * HV.RINV % Q)
        out = (C.c_uint8 * 32)()
        m = O.fq_from_limbs(HV.mont(a))
        L.fq_to_bytes(out, C.byref(m))
        assert int.from_bytes(bytes(out), "little") == a
    for x in HV.FQ_MONT_REDUCE:
        r = (C.c_uint64 * 8)(*HV.words(x, 8))
        assert L.fq_montgomery_reduce(r).limbs() == HV.words(x * HV.RINV % Q), hex(x)
    for x in HV.FQ_WIDE:
        b = (C.c_uint8 * 64)(*x.to_bytes(64, "little"))
        assert L.fq_from_bytes_wide(b).limbs() == HV.mont(x % Q), hex(x)
    for x in HV.FQ_INVERT:
        m = O.fq_from_limbs(HV.mont(x))
        assert L.fq_invert(C.byref(m)).limbs() == HV.mont(pow(x, Q - 2, Q)), hex(x)
    for x in HV.FQ_U64:
        assert L.fq_from_u64(x).limbs() == HV.mont(x)


def _oge(pt):
    g = O.Ge()
    b = (C.c_uint8 * 128)(*b"".join(c.to_bytes(32, "little") for c in (pt.X, pt.Y, pt.Z, pt.T)))
    O.lib().ge_from_xyzt(C.byref(g), b)
    return g


def _opt(g):
    b = (C.c_uint8 * 128)()
    O.lib().ge_to_xyzt(b, C.byref(g))
    raw = bytes(b)
    ws = [w for i in range(4) for w in HV.fe_limbs(int.from_bytes(raw[32 * i:32 * i + 32], "little"))]
    return HV.pt_of(ws)


def test_oracle_group_on_the_same_vectors():
    L = O.lib()
    every = [PG.Pt.identity()] + HV.base_points()
    r = O.Ge()
    for a in every:
        ga = _oge(a)
        L.ge_double(C.byref(r), C.byref(ga))
        assert _opt(r).encode() == (a + a).encode()
        for b in every:
            gb = _oge(b)
            L.ge_add(C.byref(r), C.byref(ga), C.byref(gb))
            assert _opt(r).encode() == (a + b).encode()
            L.ge_sub(C.byref(r), C.byref(ga), C.byref(gb))
            assert _opt(r).encode() == (a - b).encode()
        out = (C.c_uint8 * 32)()
        for c in HV.coset(a):   # the four representatives: equal bytes, equal points
            gc = _oge(c)
            L.ge_compress(out, C.byref(gc))
            assert bytes(out) == a.encode()
            assert L.ge_eq(C.byref(gc), C.byref(ga)) == 1
        gn = _oge(-a)
        assert L.ge_eq(C.byref(gn), C.byref(ga)) == int(a == PG.Pt.identity())
    for name, s in HV.decompress_all():
        b = (C.c_uint8 * 32)(*s.to_bytes(32, "little"))
        pt = PG.decode(bytes(b))
        assert L.ge_decompress(C.byref(r), b) == int(pt is not None), (name, hex(s))
        if pt is not None:
            got = _opt(r)
            assert (got.X, got.Y, got.Z, got.T) == (pt.X, pt.Y, pt.Z, pt.T), (name, hex(s))
    B, G0 = PG.basepoint(), HV.gens_point(0)
    gB, gG = _oge(B), _oge(G0)
    for name, s in HV.mul_scalars():
        sb = (C.c_uint8 * 32)(*s.to_bytes(32, "little"))
        L.ge_scalarmul_bytes(C.byref(r), sb, C.byref(gB))
        assert _opt(r).encode() == HV._smul(s, "B", B).encode(), name
    for name, s in HV.fb_cases():
        m = O.fq_from_limbs(HV.mont(s))
        L.ge_scalarmul(C.byref(r), C.byref(m), C.byref(gG))
        assert _opt(r).encode() == HV._smul(s, "gens[0]", G0).encode(), name
    stream = HV.gens_stream(4)
    for i in range(4):
        b = (C.c_uint8 * 64)(*stream[64 * i:64 * i + 64])
        L.ge_from_uniform_bytes(C.byref(r), b)
        assert _opt(r).encode() == HV.gens_point(i).encode()


# ---- the same code under the sanitizers, as a program of its own ---------------------------------------------------------------
def test_sanitizer_program(tmp_path):
    """tests/hostarith/hostarith_main.cpp built with -fsanitize=address,undefined, run as a child process on every group: no
    report, exit status 0, and the printed results equal the expected values.  Nothing sanitized is loaded into this process."""
    from vpin_amd import build as vbuild
    exe = vbuild.build_hosttest_program(str(tmp_path / "hostarith_main"))
    vec = tmp_path / "vectors.txt"
    HV.write_vector_file(str(vec), GROUPS)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, str(vec)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, f"exit {p.returncode}\n{err[-4000:]}"
    outs = HV.parse_output(p.stdout.decode(), GROUPS)
    for name, grp in GROUPS.items():
        grp.check(outs[name])

