"""Tensor references and the addition layer in a layer list, without a GPU (vpin_net_cfg_counts over vpin_net_layer's input_from and
skip_from, VPIN_NET_ADD, vpin_amd.net.Config.add / residual_block): the counts of an ADD layer and of networks whose shapes are only
right if input_from is followed, against tests/residual_model.py; every rejection of the planning walk with its text; ABI 12 and
its symbols; and a list whose new fields are all zero counts as it always did."""
import ctypes as C

import numpy as np
import pytest

import fcs_model as TM
import residual_model as RM
from vpin_amd import build as vbuild

EINVAL = -1


@pytest.fixture(scope="module")
def VN():
    vbuild.build()
    from vpin_amd import net
    return net


def test_abi_version_and_symbols(VN):
    import vpin_amd
    from vpin_amd import capi
    assert capi.lib().vpin_abi_version() >= 12 and (VN.ADD, VN.FROM_INPUT) == (5, 2**64 - 1)
    assert "vpin_enc_add" in vpin_amd.exported_symbols()
    assert [f[0] for f in capi.NetLayer12._fields_] == ["input_from", "skip_from"]
    assert C.sizeof(capi.NetLayer12) == C.sizeof(capi.NetLayer8) + 2 * C.sizeof(C.c_size_t)
    assert capi.NetCfg.layers.size == C.sizeof(C.c_void_p) and capi.NetCfg._fields_[-1][1] == C.POINTER(capi.NetLayer12)


@pytest.mark.parametrize("name", sorted(RM.CONFIGS))
def test_counts_follow_the_references(VN, name):
    model = RM.CONFIGS[name]()
    n_rounds = sum(1 for l in model["layers"] if l.get("round"))
    cfg = RM.device_config(model, [1] * n_rounds)
    want = RM.net_counts(model)
    assert cfg.counts() == dict(want, rounds=n_rounds)
    for l, (m, a), ((c, h, w), _) in zip(model["layers"], cfg.counts()["layers"], RM.net_shapes(model)):
        if l["kind"] == "add":
            assert (m, a) == (0, 2 * c * h * w)
    assert cfg.counts(batch=3)["n_add"] == 3 * want["n_add"]
    sched = VN.schedule(cfg)
    assert [n for _, _, n in sched] == want["per_round"]
    assert VN.proof_expectation(cfg) == [(0, 1, want["n_mult"]), (0, 0, want["n_add"])]
    at = [l["kind"] for l in model["layers"]].index("add")  # per layer an ADD has one record: it multiplies nothing
    assert [e for e in VN.proof_expectation(cfg, per_layer=True) if e[0] == 1 + at] == [(1 + at, 0, want["layers"][at][1])]


def test_the_base_network_by_hand(VN):
    cfg = RM.device_config(RM.base_config(), [1] * 4)
    c = cfg.counts()
    #        CONVMC 1 -> 2 with bias        CONVMC 2 -> 2               ADD           pool 2 / 2               FCS 18 -> 3
    assert c["layers"] == [(2 * 9 * 2, 2 * 9 * 2 - 4 + 2 * 2 * 36), (2 * 9 * 4, 2 * 9 * 4 - 4), (0, 2 * 2 * 36), (0, 2 * 2 * 9 * 3), (36, 2 * (3 + 17))]
    assert c["per_round"] == [72, 72, 72, 3] and c["prf_keys"] == 4 + 4 + 0 + 0 + 2 and c["bias_r"] == 2 + 3
    assert [l.kind for l in cfg.layers] == [VN.CONVMC, VN.CONVMC, VN.ADD, VN.POOL, VN.FCS]
    assert [(l.input_from, l.skip_from) for l in cfg.layers] == [(0, 0), (0, 0), (0, 1), (0, 0), (0, 0)]


def test_the_stride_2_block_is_only_right_if_input_from_is_followed(VN):
    """behind layer 1 (2 x 3 x 3) the 1 x 1 projection of stride 2 would leave 2 x 2; from the input (1 x 6 x 6) it leaves 3 x 3"""
    import vpin_amd
    model = RM.projection_config()
    cfg = RM.device_config(model, [1] * 5)
    assert cfg.layers[2].input_from == VN.FROM_INPUT and cfg.layers[3].skip_from == 2
    c = cfg.counts()
    assert c["layers"][2] == (2 * 1 * 2, 2 * 1 * 2 - 4) and c["layers"][3] == (0, 2 * 2 * 9) and c["per_round"] == [18, 18, 18, 18, 3]
    cfg.layers[2].input_from = 0
    with pytest.raises(vpin_amd.VpinError, match="an addition layer's operands differ in shape: C x H x W = 2 x 2 x 2 and 2 x 3 x 3") as e:
        cfg.counts()
    assert e.value.code == EINVAL


def test_residual_block_appends_the_block(VN):
    w = lambda n_out, c, f: np.ones((n_out, c, f, f), dtype=np.int64)
    r = dict(shift_bits=20, max_giant=7)
    cfg = VN.Config(1, 8, 8, 13)
    cfg.convmc(w(2, 1, 3), pad=1).round(**r)
    cfg.residual_block(w(2, 2, 3), [1, 2], w(2, 2, 3), None, [r, r, dict(max_giant=9)])
    cfg.residual_block(w(4, 2, 3), None, w(4, 4, 3), None, [r, r, dict(r, shift_bits=19), dict(max_giant=9)], stride=2, proj=w(4, 2, 1))
    ls = cfg.layers
    assert [l.kind for l in ls] == [VN.CONVMC, VN.CONVMC, VN.CONVMC, VN.ADD, VN.CONVMC, VN.CONVMC, VN.CONVMC, VN.ADD]
    assert [(l.input_from, l.skip_from) for l in ls] == [(0, 0), (0, 0), (0, 0), (0, 1), (0, 0), (0, 0), (4, 0), (0, 6)]
    assert [(l.fh, l.pad, l.stride) for l in ls if l.kind == VN.CONVMC] == [(3, 1, 1), (3, 1, 1), (3, 1, 1), (3, 1, 2), (3, 1, 1), (1, 0, 2)]
    assert [(l.relu, l.shift_bits) for l in ls] == [(0, 20), (1, 20), (0, 20), (1, 0), (1, 20), (0, 20), (0, 19), (1, 0)]
    assert cfg.max_giants() == [7, 7, 7, 9, 7, 7, 7, 9]
    c = cfg.counts()
    assert c["per_round"] == [2 * 64] * 4 + [4 * 16] * 4 and c["layers"][3] == (0, 2 * 2 * 64) and c["layers"][7] == (0, 2 * 4 * 16)
    first = VN.Config(1, 8, 8, 13).residual_block(w(1, 1, 3), None, w(1, 1, 3), None, [r, r, r])
    assert [(l.input_from, l.skip_from) for l in first.layers] == [(0, 0), (0, 0), (0, VN.FROM_INPUT)]
    assert first.counts()["layers"][2] == (0, 2 * 64)


def base(VN):
    return RM.device_config(RM.base_config(), [1] * 4)


@pytest.mark.parametrize("change, text", [
    (lambda ls, VN: setattr(ls[1], "input_from", 2), "vpin_net: layer 1: input_from = 2 names the layer itself or a later one"),
    (lambda ls, VN: setattr(ls[0], "input_from", 1), "vpin_net: layer 0: input_from = 1 names the layer itself or a later one"),
    (lambda ls, VN: setattr(ls[3], "input_from", 5), "vpin_net: layer 3: input_from = 5 names the layer itself or a later one"),
    (lambda ls, VN: setattr(ls[2], "skip_from", 3), "vpin_net: layer 2: skip_from = 3 names the layer itself or a later one"),
    (lambda ls, VN: setattr(ls[2], "skip_from", 4), "vpin_net: layer 2: skip_from = 4 names the layer itself or a later one"),
    (lambda ls, VN: setattr(ls[1], "skip_from", 1), "vpin_net: layer 1: only an addition layer takes a skip_from"),
    (lambda ls, VN: setattr(ls[3], "skip_from", VN.FROM_INPUT), "vpin_net: layer 3: only an addition layer takes a skip_from"),
    (lambda ls, VN: setattr(ls[2], "skip_from", 0), "vpin_net: layer 2: an addition layer has no skip_from"),
    (lambda ls, VN: setattr(ls[2], "skip_from", 2), "vpin_net: layer 2: an addition layer's two operands are the same tensor (every addition would be a doubling)"),
    (lambda ls, VN: (setattr(ls[2], "input_from", 1), setattr(ls[2], "skip_from", 1)),
     "vpin_net: layer 2: an addition layer's two operands are the same tensor (every addition would be a doubling)"),
    (lambda ls, VN: setattr(ls[2], "skip_from", VN.FROM_INPUT),
     "vpin_net: layer 2: an addition layer's operands differ in shape: C x H x W = 2 x 6 x 6 and 1 x 6 x 6"),
    (lambda ls, VN: setattr(ls[2], "plane_order", VN.ORDER_INTERLEAVED), "vpin_net: layer 2: an addition layer takes no plane_order, sum_table or repeat"),
    (lambda ls, VN: setattr(ls[2], "sum_table", ls[0].w_mc), "vpin_net: layer 2: an addition layer takes no plane_order, sum_table or repeat"),
    (lambda ls, VN: setattr(ls[2], "repeat", 2), "vpin_net: layer 2: an addition layer takes no plane_order, sum_table or repeat"),
])
def test_every_rejection_has_its_text(VN, change, text):
    import vpin_amd
    cfg = base(VN)
    change(cfg.layers, VN)
    with pytest.raises(vpin_amd.VpinError) as e:
        cfg.counts()
    assert e.value.code == EINVAL and text in str(e.value), e.value


def test_a_pooled_tensor_and_its_source_differ_in_h_and_w(VN):
    import vpin_amd
    cfg = VN.Config(2, 4, 4, 13).pool(2, 2, 1).add(VN.FROM_INPUT)
    with pytest.raises(vpin_amd.VpinError, match="operands differ in shape: C x H x W = 2 x 2 x 2 and 2 x 4 x 4"):
        cfg.counts()
    # and layer 0 may add nothing: its only tensor is the input, twice
    with pytest.raises(vpin_amd.VpinError, match="layer 0: an addition layer's two operands are the same tensor"):
        VN.Config(2, 4, 4, 13).add(VN.FROM_INPUT).counts()


def test_an_all_zero_tail_counts_as_before(VN):
    """today's lenet5_config: no layer sets input_from or skip_from, and its counts are fcs_model's formula, unchanged"""
    cfg = TM.lenet5_device_config([1] * 7)
    assert all((l.input_from, l.skip_from) == (0, 0) for l in cfg.layers)
    assert cfg.counts() == dict(TM.net_counts(TM.lenet5_model_config()), rounds=7)
    explicit = TM.lenet5_device_config([1] * 7)
    for i, l in enumerate(explicit.layers):  # naming the previous layer's output is the default, said aloud
        l.input_from = i or VN.FROM_INPUT
    assert explicit.counts() == cfg.counts()
    from vpin_amd import lenet as VL
    import tiny_lenet as TL
    tiny = VN.from_lenet(TL.make_cfg(VL))
    assert all((l.input_from, l.skip_from) == (0, 0) for l in tiny.layers)
