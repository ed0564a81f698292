"""The model of the client's ElGamal (tests/elgamal_model.py) without a GPU: it round-trips, its baby-step / giant-step walk
keeps to its range, and the client entry points of the library are declared, exported and reject a NULL context."""
import ctypes as C

import pytest

import elgamal_model as EM

NAMES = ["vpin_e2_base_create", "vpin_e2_base_free", "vpin_e2_base_mul", "vpin_e2_encrypt", "vpin_e2_dlog_create", "vpin_e2_dlog_free",
         "vpin_e2_dlog_info", "vpin_e2_dlog_solve", "vpin_e2_decrypt", "vpin_e2_mul256", "vpin_e2_base_create_w"]


@pytest.fixture(scope="module")
def table():
    return EM.baby_steps(64)


def test_model_round_trips(table):
    sk = 0x1234567890ABCDEF1234567890ABCDEF
    H = EM.keygen(sk)
    msgs = [0, 1, -1, 65535, -65535]
    rs = EM.splitmix_scalars(0xE1, len(msgs))
    for m, r in zip(msgs, rs):
        c1, c2 = EM.encrypt(H, m, r)
        assert EM.decrypt(table, 64, sk, c1, c2, 1024) == m


def test_model_walk_range(table):
    """nb = 64, max_giant = 3: the last value in range is 3 * 64 + 63, the identity is j = 0"""
    assert EM.bsgs(table, 64, None, 0) == 0
    for v in (63, -63, 64, -64, 255, -255):
        assert EM.bsgs(table, 64, EM.mul(v), 3) == v
    assert EM.bsgs(table, 64, EM.mul(256), 3) is None and EM.bsgs(table, 64, EM.mul(-256), 3) is None
    assert EM.bsgs(table, 64, EM.mul(64), 0) is None


def test_library_declares_and_exports_the_client():
    import vpin_amd
    L = vpin_amd.lib()
    assert set(NAMES) <= set(vpin_amd.declared_symbols())
    assert all(hasattr(L, n) for n in NAMES)


def test_null_context_is_einval():
    import vpin_amd
    L = vpin_amd.lib()
    buf = (C.c_uint8 * 64)()
    b = C.cast(buf, C.c_void_p)
    calls = {
        "vpin_e2_base_create": lambda h: L.vpin_e2_base_create(None, None, None, C.byref(h)),
        "vpin_e2_base_create_w": lambda h: L.vpin_e2_base_create_w(None, None, None, 8, C.byref(h)),
        "vpin_e2_base_mul": lambda h: L.vpin_e2_base_mul(None, b, b, 1, b, b, b),
        "vpin_e2_mul256": lambda h: L.vpin_e2_mul256(None, b, b, b, b, 1, b, b, b),
        "vpin_e2_encrypt": lambda h: L.vpin_e2_encrypt(None, b, b, b, b, 1, b, b, b, b, b, b),
        "vpin_e2_dlog_create": lambda h: L.vpin_e2_dlog_create(None, 64, C.byref(h)),
        "vpin_e2_dlog_solve": lambda h: L.vpin_e2_dlog_solve(None, b, b, b, b, 1, 1, b, b),
        "vpin_e2_decrypt": lambda h: L.vpin_e2_decrypt(None, b, b, b, b, b, b, b, b, 1, 1, b, b),
    }
    for name, call in calls.items():
        h = C.c_void_p(1)
        assert call(h) == -1, name
        assert b"null" in L.vpin_last_error(), name
        if "create" in name:
            assert not h.value, name
    assert L.vpin_e2_dlog_info(None, None) == -1
    L.vpin_e2_base_free(None)
    L.vpin_e2_dlog_free(None)
