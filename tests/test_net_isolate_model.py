"""Images that leave a running batch, on the models and without a GPU (vpin_net_infer_isolated, vpin_enc_last_refusals): the
isolated driver's model (tests/net_isolate_model.py) over the layers' models on discrete logarithms.  A batch that loses an image
equals the single runs of the survivors under their slots' keys, whether a layer refuses the image at the first layer, at a later
one (an identity in its reply), or the round drops it; the ShapeError of enc_conv_model, enc_fc_model, fcs_model and convmc_model
is raised for exactly the planted units of the inputs that the GPU tests share, and for no other.  Also the host side of the
interface: the new symbols, the ABI version and the refusals of null arguments."""
import numpy as np
import pytest

import convmc_model as CM
import enc_conv_model as EM
import enc_fc_model as FM
import fcs_model as TM
import net_batch_model as BM
import net_isolate_model as IM
import net_model as NM
from test_net_multi_model import encrypt_biases

LOGS = EM.LOGS


# ---- the layers refuse exactly what is planted -------------------------------------------------------------------------------------

def refuses(fn):
    try:
        fn()
    except EM.ShapeError:
        return True
    return False


def test_fc_signed_refuses_the_planted_rows_and_no_other():
    c = IM.FCS_CASE
    x, bias = IM.fcs_case_logs()
    keys = IM.case_keys(c["P"])
    row = lambda p: TM.fc_signed(LOGS, [x[p * c["K"]:(p + 1) * c["K"]]], c["K"], c["W"], c["N"], [bias[p * c["N"]:(p + 1) * c["N"]]], [keys[p]],
                                 c["prf_bytes"])
    assert [p for p in range(c["P"]) if refuses(lambda: row(p))] == list(c["identity_rows"])
    with pytest.raises(EM.ShapeError, match=r"X\[0\] is the identity"):
        row(1)
    # the unsigned layer on the magnitudes: the same rows
    W = [[abs(v) for v in r] for r in c["W"]]
    row_u = lambda p: FM.fc(LOGS, [x[p * c["K"]:(p + 1) * c["K"]]], c["K"], W, c["N"], [bias[p * c["N"]:(p + 1) * c["N"]]], [keys[p]], c["prf_bytes"])
    assert [p for p in range(c["P"]) if refuses(lambda: row_u(p))] == list(c["identity_rows"])


def test_conv_and_pool_refuse_the_planted_planes_and_no_other():
    c = IM.CONV_CASE
    x, per, keys = IM.conv_case_logs(), c["H"] * c["W"], IM.case_keys(c["P"])
    plane = lambda p: EM.layer(LOGS, [x[p * per:(p + 1) * per]], c["H"], c["W"], c["filt"], c["f"], c["f"], 0, 1, [keys[p]], c["prf_bytes"])
    assert [p for p in range(c["P"]) if refuses(lambda: plane(p))] == list(c["identity_planes"])
    c = IM.POOL_CASE
    x, per = IM.pool_case_logs(), c["H"] * c["W"]
    pooled = lambda p: FM.avgpool(LOGS, [x[p * per:(p + 1) * per]], c["H"], c["W"], c["k"], c["k"], c["scale"])
    assert [p for p in range(c["P"]) if refuses(lambda: pooled(p))] == list(c["first_pixel_identity"])


def test_convmc_refuses_the_planted_group_and_no_other():
    c = IM.CONVMC_CASE
    x, per, keys = IM.convmc_case_logs(), c["C"] * c["H"] * c["W"], IM.case_keys(c["groups"] * c["n_out"])
    group = lambda g: CM.layer(LOGS, [x[g * per:(g + 1) * per]], c["C"], c["n_out"], c["H"], c["W"], c["w"], None, c["f"], c["f"], 0, 1,
                               keys[g * c["n_out"]:(g + 1) * c["n_out"]], c["prf_bytes"])
    assert [g for g in range(c["groups"]) if refuses(lambda: group(g))] == list(c["identity_groups"])


# ---- the driver: a batch that loses an image is the survivors' single runs -------------------------------------------------------------

def slot_clients(d, B, seen, reply_hook=None, leaving=None):
    """the round callback over the live slots: slot b's values go to its own client (its key, its queue).  reply_hook(b, rnd, ans)
    may change what slot b answers; leaving: {round: slots that the callback drops}"""
    fns = [NM.log_client(d["sks"][b], d["client_r"][b], seen[b]) for b in range(B)]

    def client(slots, rnd, relu, bits, reencrypt, c1, c2):
        a1, a2 = [], []
        for at, b in enumerate(slots):
            ans = fns[b](rnd, relu, bits, reencrypt, BM.part(c1, at, len(slots)), BM.part(c2, at, len(slots)))
            if reencrypt:
                ans = reply_hook(b, rnd, ans) if reply_hook else ans
                a1 += ans[0]
                a2 += ans[1]
        return ((a1, a2) if reencrypt else None), [b for b in (leaving or {}).get(rnd, []) if b in slots]

    return client


def single_run(d, b):
    """slot b alone: its image under its client's key, its slot's keys and bias r -> (layers, rounds)"""
    c1, c2 = NM.log_encrypt(d["sks"][b], d["images"][b], d["image_r"][b])
    seen = []
    layers, _ = BM.infer_batch_model(LOGS, d["model"], [c1], [c2], [d["keys"][b]], encrypt_biases(d["model"], [d["sks"][b]], [d["bias_r"][b]]),
                                     NM.log_client(d["sks"][b], d["client_r"][b], seen))
    return layers, seen


def run_isolated(d, B, plant=None, **kw):
    enc = [NM.log_encrypt(d["sks"][b], d["images"][b], d["image_r"][b]) for b in range(B)]
    c1, c2 = [list(e[0]) for e in enc], [list(e[1]) for e in enc]
    if plant:
        plant(c1, c2)
    seen = [[] for _ in range(B)]
    calls, status = IM.infer_isolated_model(LOGS, d["model"], c1, c2, d["keys"][:B], encrypt_biases(d["model"], d["sks"][:B], d["bias_r"][:B]),
                                            slot_clients(d, B, seen, **kw))
    return calls, status, seen


def assert_survivor_is_its_single_run(d, b, calls, seen, upto=None):
    ref, ref_seen = single_run(d, b)
    n = len(calls) if upto is None else upto
    for i in range(n):
        for key in ("out", "mults", "adds", "left"):
            assert IM.image_part(calls[i], b, key) == list(ref[i].get(key, [])), "slot %d layer %d %s" % (b, i, key)
    assert [(list(v), list(a)) for v, a in seen[b][:n]] == [(list(v), list(a)) for v, a in ref_seen[:n]]


def test_an_image_refused_at_the_first_layer_leaves_and_the_others_are_their_single_runs():
    d = IM.two_round_inputs()

    def plant(c1, c2):
        c1[1][3] = 0  # one identity c1 point of slot 1

    calls, status, seen = run_isolated(d, 3, plant)
    assert [c["slots"] for c in calls] == [[0, 2], [0, 2]]
    assert status[0] is None and status[2] is None and status[1][:3] == (IM.ESHAPE, 0, -1) and "X[3] is the identity" in status[1][3]
    assert seen[1] == []
    for b in (0, 2):
        assert_survivor_is_its_single_run(d, b, calls, seen)
        plain = TM.net_plaintext(d["model"], np.array(d["images"][b]).reshape(1, 2, 4))
        assert [list(v) for v, _ in seen[b]] == plain[0]


def test_an_image_refused_at_a_later_layer_was_there_before():
    d = IM.two_round_inputs()

    def hook(b, rnd, ans):
        if b == 1 and rnd == 0:
            return [0] + list(ans[0][1:]), ans[1]  # its reply carries an identity c1
        return ans

    calls, status, seen = run_isolated(d, 3, reply_hook=hook)
    assert [c["slots"] for c in calls] == [[0, 1, 2], [0, 2]]
    assert status[1][:3] == (IM.ESHAPE, 1, -1) and status[0] is None and status[2] is None
    assert_survivor_is_its_single_run(d, 1, calls, seen, upto=1)
    for b in (0, 2):
        assert_survivor_is_its_single_run(d, b, calls, seen)


def test_an_image_dropped_in_a_round_is_not_in_the_next_layer():
    d = IM.two_round_inputs()
    calls, status, seen = run_isolated(d, 3, leaving={0: [0]})
    assert [c["slots"] for c in calls] == [[0, 1, 2], [1, 2]] and status[0][:3] == (IM.ESHAPE, 0, 0)
    for b in (1, 2):
        assert_survivor_is_its_single_run(d, b, calls, seen)
    with pytest.raises(EM.ShapeError, match="no image is left"):
        run_isolated(d, 3, leaving={0: [0, 1, 2]})


def test_nothing_refuses_is_the_batch_drivers_model():
    d = IM.two_round_inputs()
    calls, status, seen = run_isolated(d, 3)
    assert status == [None] * 3
    enc = [NM.log_encrypt(d["sks"][b], d["images"][b], d["image_r"][b]) for b in range(3)]
    ref_seen = [[] for _ in range(3)]
    fns = [NM.log_client(d["sks"][b], d["client_r"][b], ref_seen[b]) for b in range(3)]

    def client(rnd, relu, bits, reencrypt, c1, c2):
        ans = [fns[b](rnd, relu, bits, reencrypt, BM.part(c1, b, 3), BM.part(c2, b, 3)) for b in range(3)]
        return (BM.flat([a[0] for a in ans]), BM.flat([a[1] for a in ans])) if reencrypt else None

    ref, _ = BM.infer_batch_model(LOGS, d["model"], [e[0] for e in enc], [e[1] for e in enc], d["keys"][:3],
                                  encrypt_biases(d["model"], d["sks"], d["bias_r"][:3]), client)
    assert [c["res"] for c in calls] == ref and seen == ref_seen


def test_the_trained_network_loses_the_image_with_an_all_identity_c1():
    d = dict(BM.trained_inputs(3), sks=IM.TWO_ROUND_SKS)

    def plant(c1, c2):
        c1[0] = [0] * len(c1[0])

    calls, status, seen = run_isolated(d, 3, plant)
    assert [c["slots"] for c in calls] == [[1, 2]] * 5 and status[0][:3] == (IM.ESHAPE, 0, -1) and status[1:] == [None, None]
    for b in (1, 2):
        assert_survivor_is_its_single_run(d, b, calls, seen)


# ---- the host side of the interface ------------------------------------------------------------------------------------------------

def test_the_binding_has_the_new_symbols():
    import ctypes as C
    from vpin_amd import capi, net
    L = capi.lib()
    assert L.vpin_abi_version() >= 9
    names = ["vpin_enc_last_refusals", "vpin_net_infer_isolated", "vpin_net_round_images", "vpin_net_round_drop_images",
             "vpin_net_trace_layer_images", "vpin_net_last_isolation", "vpin_net_server_set_isolation", "vpin_net_server_stats_isolation"]
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in names)
    assert callable(net.infer_isolated) and callable(net.round_images) and callable(net.round_drop_images) and net.STAGE_LAYER == -4
    assert C.sizeof(capi.NetImageStatus) == 4 + 4 + 4 + 256
    # what needs no device: outside a round callback the two hooks refuse, and null arguments are VPIN_EINVAL with their rule
    p, n = C.c_void_p(), C.c_size_t()
    assert L.vpin_net_round_images(C.byref(p), C.byref(n)) == -1 and b"no round callback is running" in L.vpin_last_error()
    assert L.vpin_net_round_drop_images(None, 0, -5, b"x") == -1 and b"no round callback is running" in L.vpin_last_error()
    assert L.vpin_enc_last_refusals(None, 0, None) == -1 and b"vpin_enc_last_refusals: null argument" in L.vpin_last_error()
    assert L.vpin_enc_last_refusals(None, 0, C.byref(n)) == 0
    assert L.vpin_net_server_set_isolation(None, 1) == -1 and L.vpin_net_server_stats_isolation(None, None) == -1
    assert L.vpin_net_trace_layer_images(None, 0, None, None) == -1
    b = (C.c_uint8 * 64)()
    assert L.vpin_net_infer_isolated(None, None, 1, b, b, b, b, b, b, None, b, b, 1, b, None, 0, None, 0, None, None, None, None) == -1
    assert b"vpin_net_infer_isolated: null argument" in L.vpin_last_error()
