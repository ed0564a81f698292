"""The reference's LeNet as a layer list, without a GPU (vpin_lenet_as_net, vpin_net_cfg_counts, the fields sum_table, sum_out,
repeat and plane_order of vpin_net_layer; vpin_amd.net.from_lenet): the list consumes exactly what vpin_lenet_cfg_counts says of
the LeNet configuration -- per label, per round and in all -- on the default network, on the 32 x 32 network of
tests/test_gpu_lenet.py and on the tiny one of tests/tiny_lenet.py; a list that sets none of the new fields counts as it always
did; and every new refusal has its text."""
import ctypes as C

import pytest

import lenet_model as LM
import tiny_lenet as TL
from vpin_amd import build as vbuild

FULL = LM.default_config()
SMALL32 = dict(H=32, W=32, n1=2, n2=3, n3=4, connect=[[1, 1], [0, 1], [1, 0]], f=FULL["f"], filter=FULL["filter"], pool_k=2, pool_stride=2,
               pool_scale=1, rounds=[(1, 0), (0, 14), (1, 0), (0, 18), (1, 20), (1, 19), (1, 0)], N1=3, N2=2)


@pytest.fixture(scope="module")
def mods():
    vbuild.build()
    from vpin_amd import lenet, net
    return lenet, net


def lenet_cfgs(VL):
    _, w1, b1, w2, b2 = LM.reference_model()
    return dict(default=(VL.default_config(w1, b1, w2, b2), FULL), small32=(TL.make_cfg(VL, SMALL32), SMALL32), tiny=(TL.make_cfg(VL), TL.CFG))


@pytest.mark.parametrize("which", ["default", "small32", "tiny"])
def test_the_list_consumes_what_the_lenet_configuration_says(mods, which):
    VL, VN = mods
    lcfg, model = lenet_cfgs(VL)[which]
    want, got = lcfg.counts(), VN.from_lenet(lcfg).counts()
    assert want == dict(LM.counts(model), labels=[tuple(l) for l in LM.counts(model)["labels"]])
    assert got["layers"] == want["labels"] and got["per_round"] == want["per_round"] and got["rounds"] == 7
    assert (got["n_mult"], got["n_add"]) == (sum(m for m, _ in want["labels"]), sum(a for _, a in want["labels"]))
    assert (got["decryptions"], got["encryptions"], got["prf_keys"], got["bias_r"]) == (want["decryptions"], want["encryptions"], want["prf_keys"], want["bias_r"])
    assert VN.from_lenet(lcfg).counts(batch=3)["prf_keys"] == 3 * want["prf_keys"]


def test_the_list_is_the_seven_steps_of_lenet_infer(mods):
    VL, VN = mods
    lcfg = TL.make_cfg(VL, giants=[3, 5, 7, 9, 11, 13, 15])
    cfg = VN.from_lenet(lcfg)
    ls = cfg.layers
    assert cfg.dims == (1, 11, 11) and cfg.prf_bytes == lcfg.c.prf_bytes and cfg.max_giants() == [3, 5, 7, 9, 11, 13, 15]
    assert [l.kind for l in ls] == [VN.CONV, VN.POOL, VN.CONV, VN.POOL, VN.CONV, VN.FC, VN.FC]
    assert [l.plane_order for l in ls] == [VN.ORDER_INTERLEAVED] * 5 + [0, 0]
    assert [(l.repeat, l.sum_out, bool(l.sum_table)) for l in ls] == [(2, 0, False), (0, 0, False), (0, 3, True), (0, 0, False), (4, 1, True), (0, 0, False), (0, 0, False)]
    assert ls[2].sum_table == lcfg.c.connect and bytes((C.c_uint8 * 3).from_address(ls[4].sum_table)) == b"\1\1\1"
    assert [(l.has_round, l.relu, l.shift_bits, l.reencrypt) for l in ls] == [(1, r, s, int(i < 6)) for i, (r, s) in enumerate(TL.CFG["rounds"])]
    assert [(ls[i].K, ls[i].N) for i in (5, 6)] == [(4, 3), (3, 2)] and [(l.fh, l.fw, l.pad, l.stride) for l in ls[0:5:2]] == [(2, 2, 0, 1)] * 3
    assert VN.schedule(cfg, batch=2) == [(3, 0, 400), (2, 17, 100), (3, 0, 96), (2, 18, 24), (3, 20, 8), (3, 19, 6), (1, 0, 4)]


def test_a_bad_lenet_configuration_has_the_texts_of_lenet_infer(mods):
    import vpin_amd
    VL, VN = mods
    for change, text in [(lambda b: b.set_pool(2, 1, 1), "vpin_lenet: a window does not fit its plane|vpin_lenet: the third convolution's output is not 1 x 1"),
                         (lambda b: b.connect.__setitem__((1, slice(None)), 0), "vpin_lenet: a row of the connection table selects no plane"),
                         (lambda b: b.w2.__setitem__((1, 1), -1), "vpin_lenet: a weight of the second fully connected layer is negative"),
                         (lambda b: setattr(b.c, "n3", 0), "vpin_lenet: a dimension is zero")]:
        bad = TL.make_cfg(VL)
        change(bad)
        with pytest.raises(vpin_amd.VpinError, match=text) as e:
            VN.from_lenet(bad)
        assert e.value.code == -1
    from vpin_amd import capi
    L = capi.lib()
    assert L.vpin_lenet_as_net(None, None, None, None) == -1 and b"vpin_lenet_as_net: null argument" in L.vpin_last_error()


def old_style(VN):
    """a list of every layer kind that sets none of the new fields"""
    cfg = VN.Config(2, 12, 12, 14)
    cfg.conv([[1, 2, 1], [0, 1, 0], [3, 0, 1]], pad=1).round(relu=True)
    cfg.pool(2, 2, 64).round(shift_bits=20)
    cfg.convmc([[[[1, -2], [3, 1]]] * 2] * 3, connect=[[1, 1], [0, 1], [1, 0]], bias=[1, 2, 3]).round(relu=True)
    cfg.fcs([[1, -1]] * 75, [4, 5]).round(relu=True, reencrypt=False)
    return cfg


def test_a_list_with_the_new_fields_zero_counts_as_before(mods):
    _, VN = mods
    cfg = old_style(VN)
    assert all((l.sum_table, l.sum_out, l.repeat, l.plane_order) == (None, 0, 0, 0) for l in cfg.layers)
    # by hand, from the layers' definitions: conv 2 C fh fw and 2 C (fh fw - 1); pool 2 C oh ow (k k - 1); convmc 2 fh fw pairs, less 2
    # n_out, plus the bias's 2 n_out oh ow; fcs 2 K and 2 (N + K - 1)
    want = [(2 * 2 * 9, 2 * 2 * 8), (0, 2 * 2 * 36 * 3), (2 * 4 * 4, 2 * 4 * 4 - 6 + 2 * 3 * 25), (2 * 75, 2 * (2 + 75 - 1))]
    c = cfg.counts()
    assert c["layers"] == want and c["per_round"] == [2 * 144, 2 * 36, 3 * 25, 2] and c["prf_keys"] == 4 + 6 + 2 and c["bias_r"] == 3 + 2
    assert c["encryptions"] == 2 * 144 + 2 * 144 + 2 * 36 + 3 * 25 and c["decryptions"] == 2 * 144 + 2 * 36 + 3 * 25 + 2
    # the blocked order said by name, and a repeat of 1, are the same list
    for l in cfg.layers:
        l.repeat = 1 if l.kind == VN.CONV else 0
    assert cfg.counts() == c


def test_what_the_new_fields_add_to_the_counts(mods):
    """a convolution behind sums to 3 planes, handed over twice: 6 planes per half go through the filter and come out"""
    _, VN = mods
    cfg = VN.Config(2, 6, 6, 13)
    cfg.conv([[1, 2], [3, 4]], sum_table=[[1, 1], [0, 1], [1, 0]], repeat=2, interleaved=True).round()
    cfg.pool(5, 1, 1, interleaved=True).round(reencrypt=False)
    c = cfg.counts()
    assert c["layers"] == [(2 * 6 * 4, 2 * 6 * 3), (0, 2 * 6 * 1 * 24)] and c["prf_keys"] == 12 and c["per_round"] == [6 * 25, 6]
    assert c["encryptions"] == 2 * 36 + 6 * 25


def test_every_new_refusal_has_its_text(mods):
    import vpin_amd
    _, VN = mods

    def einval(change, text):
        cfg = VN.Config(2, 6, 6, 13)
        cfg.conv([[1, 2], [3, 4]], sum_table=[[1, 1], [0, 1], [1, 0]], repeat=2).round()
        cfg.pool(5, 1, 1).round()
        cfg.fc([[1, 2]] * 6, [0, 0]).round(reencrypt=False)
        change(cfg.layers)
        with pytest.raises(vpin_amd.VpinError) as e:
            cfg.counts()
        assert e.value.code == -1 and text in str(e.value), e.value

    table = lambda ls: ls[0].sum_table
    einval(lambda ls: setattr(ls[1], "sum_table", table(ls)), "vpin_net: only a convolution takes a sum_table or a repeat")
    einval(lambda ls: setattr(ls[2], "sum_table", table(ls)), "vpin_net: only a convolution takes a sum_table or a repeat")
    einval(lambda ls: setattr(ls[1], "repeat", 2), "vpin_net: only a convolution takes a sum_table or a repeat")
    einval(lambda ls: setattr(ls[2], "repeat", 3), "vpin_net: only a convolution takes a sum_table or a repeat")
    einval(lambda ls: setattr(ls[0], "sum_out", 0), "vpin_net: a convolution has a sum_table and sum_out = 0")
    einval(lambda ls: C.memset(table(ls) + 2, 0, 2), "vpin_net: a row of a convolution's sum_table selects no plane")
    einval(lambda ls: setattr(ls[0], "plane_order", 2), "vpin_net: a layer's plane_order is neither 0 nor VPIN_NET_ORDER_INTERLEAVED")
    einval(lambda ls: setattr(ls[1], "plane_order", -1), "vpin_net: a layer's plane_order is neither 0 nor VPIN_NET_ORDER_INTERLEAVED")
    einval(lambda ls: setattr(ls[0], "repeat", 1 << 20), "vpin_net: a dimension is out of range")
    einval(lambda ls: setattr(ls[0], "sum_out", 1 << 20), "vpin_net: a dimension is out of range")


def test_abi_version_and_symbols(mods):
    import vpin_amd
    from vpin_amd import capi
    L = capi.lib()
    assert L.vpin_abi_version() >= 8 and mods[1].ORDER_INTERLEAVED == 1
    for name in ("vpin_e2_plane_sums_batch", "vpin_lenet_as_net", "vpin_net_trace_image_layer"):
        assert name in vpin_amd.exported_symbols()
