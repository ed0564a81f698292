"""Max pooling inside the client's round in a layer list, without a GPU (vpin_net_cfg_counts over vpin_net_layer's round_pool_k and
round_pool_stride, vpin_amd.net.Config.round(maxpool=), schedule and pool_schedule): ABI 13 and its symbols; every new rejection
of the planning walk with its text; the counts of a network whose later layers are only right if the pooled shape is followed,
against tests/maxpool_model.py; and a list whose new fields are all zero counts as it always did."""
import ctypes as C

import pytest

import fcs_model as TM
import maxpool_model as MM
from vpin_amd import build as vbuild

EINVAL = -1


@pytest.fixture(scope="module")
def VN():
    vbuild.build()
    from vpin_amd import net
    return net


def small(VN):
    return MM.device_config(MM.small_config(), [1] * 4)


def test_abi_version_and_symbols(VN):
    import vpin_amd
    from vpin_amd import capi, inference
    assert capi.lib().vpin_abi_version() >= 13 and VN.MAXPOOL == 4 == inference.MAXPOOL
    syms = vpin_amd.exported_symbols()
    for name in ("vpin_e2_client_round_pool", "vpin_net_round_pool", "vpin_net_client_set_pools", "vpin_net_client_act_count"):
        assert name in syms
    assert [f[0] for f in capi.NetLayer13._fields_] == ["round_pool_k", "round_pool_stride"]
    assert C.sizeof(capi.NetLayer13) == C.sizeof(capi.NetLayer12) + 2 * C.sizeof(C.c_size_t)
    assert C.sizeof(capi.NetRoundPoolSpec) == 4 * C.sizeof(C.c_size_t)
    # outside a callback the accessor says so, as vpin_net_round_images does
    with pytest.raises(vpin_amd.VpinError, match="vpin_net_round_pool: no round callback is running on this thread") as e:
        VN.round_pool()
    assert e.value.code == EINVAL
    # an array of the whole struct is what the configuration points to
    cfg = small(VN)
    assert isinstance(cfg.layers[0], capi.NetLayer13) and (cfg.layers[0].round_pool_k, cfg.layers[0].round_pool_stride) == (2, 2)


@pytest.mark.parametrize("change, text", [
    (lambda ls: (setattr(ls[0], "has_round", 0), setattr(ls[3], "K", 128), setattr(ls[2], "skip_from", 1)),
     "vpin_net: layer 0: round_pool_k or round_pool_stride on a layer without a round"),
    (lambda ls: setattr(ls[0], "round_pool_stride", 0), "vpin_net: layer 0: round_pool_k = 2 beside round_pool_stride = 0: one of the two is zero"),
    (lambda ls: setattr(ls[0], "round_pool_k", 0), "vpin_net: layer 0: round_pool_k = 0 beside round_pool_stride = 2: one of the two is zero"),
    (lambda ls: setattr(ls[1], "round_pool_stride", 3), "vpin_net: layer 1: round_pool_k = 0 beside round_pool_stride = 3: one of the two is zero"),
    (lambda ls: setattr(ls[0], "round_pool_k", 9), "vpin_net: layer 0: the round's pooling window 9 does not fit the layer's 8 x 8 output"),
    (lambda ls: (setattr(ls[1], "round_pool_k", 5), setattr(ls[1], "round_pool_stride", 1)),
     "vpin_net: layer 1: the round's pooling window 5 does not fit the layer's 4 x 4 output"),
    (lambda ls: (setattr(ls[3], "round_pool_k", 2), setattr(ls[3], "round_pool_stride", 1)),
     "vpin_net: layer 3: the round's pooling window 2 does not fit the layer's 1 x 3 output"),
])
def test_every_rejection_has_its_text(VN, change, text):
    import vpin_amd
    cfg = small(VN)
    change(cfg.layers)
    with pytest.raises(vpin_amd.VpinError) as e:
        cfg.counts()
    assert e.value.code == EINVAL and text in str(e.value), e.value


def test_counts_follow_the_pooled_shape(VN):
    import vpin_amd
    model = MM.small_config()
    cfg = small(VN)
    want = MM.net_counts(model)
    c = cfg.counts()
    assert c == dict(want, rounds=4)
    #        CONVMC 1 -> 2 over 8 x 8, biased              CONVMC 2 -> 2 over the POOLED 4 x 4   ADD over 2 x 4 x 4   FCS 32 -> 3
    assert c["layers"] == [(2 * 9 * 2, 2 * 9 * 2 - 4 + 2 * 2 * 64), (2 * 9 * 4, 2 * 9 * 4 - 4), (0, 2 * 2 * 16), (2 * 32, 2 * (3 + 31))]
    assert c["per_round"] == [128, 32, 32, 3], "out[10 + 3 i] stays the C H W the round decrypts"
    assert c["encryptions"] == 64 + 32 + 32 + 32, "out[5] counts the C Ho Wo the round encrypts"
    assert cfg.counts(batch=3)["encryptions"] == 3 * c["encryptions"]
    assert VN.shapes(cfg) == MM.net_shapes(model)
    assert VN.schedule(cfg) == [(1 | 2 | 4, 20, 128), (2, 20, 32), (1 | 2, 0, 32), (0, 0, 3)]
    assert VN.schedule(cfg, batch=2)[0] == (7, 20, 256)
    assert VN.pool_schedule(cfg) == MM.pool_schedule(model) == [(8, 8, 2, 2), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    # without the pooling the same list is refused: the FC's K, and before it nothing (the ADD's operands are both 2 x 8 x 8)
    cfg.layers[0].round_pool_k = cfg.layers[0].round_pool_stride = 0
    with pytest.raises(vpin_amd.VpinError, match="a fully connected layer's K is not the C \\* H \\* W that reaches it"):
        cfg.counts()
    # a reference to the input next to the pooled tensor: the ADD's comparison sees the pooled shape
    cfg = small(VN)
    cfg.layers[2].skip_from = VN.FROM_INPUT
    with pytest.raises(vpin_amd.VpinError, match="operands differ in shape: C x H x W = 2 x 4 x 4 and 1 x 8 x 8"):
        cfg.counts()
    # remainders are dropped, and a stride above the window leaves gaps: 8 x 8 by (3, 2) -> 3 x 3, by (2, 3) -> 3 x 3
    for k, stride, side in ((3, 2, 3), (2, 3, 3), (8, 1, 1), (1, 1, 8)):
        one = VN.Config(1, 8, 8, 13).convmc([[[[1] * 3] * 3]], pad=1).round(maxpool=(k, stride))
        assert one.counts()["encryptions"] == 64 + side * side and VN.shapes(one)[0][2] == (1, side, side)


def test_the_lenet5_shape_with_max_pooling(VN):
    model = MM.lenet5max_model_config()
    cfg = MM.device_config(model, [1] * 5)
    c = cfg.counts()
    assert c == dict(MM.net_counts(model), rounds=5)
    assert c["per_round"] == [6 * 28 * 28, 16 * 10 * 10, 120, 84, 10]
    assert c["encryptions"] == 1024 + 6 * 14 * 14 + 16 * 5 * 5 + 120 + 84
    assert VN.pool_schedule(cfg) == [(28, 28, 2, 2), (10, 10, 2, 2)] + [(0, 0, 0, 0)] * 3


def test_an_all_zero_tail_counts_as_before(VN):
    """today's lenet5_config: no round pools, and its counts are fcs_model's formula, unchanged; the reference's LeNet as a layer list
    has the new fields zeroed"""
    cfg = TM.lenet5_device_config([1] * 7)
    assert all((l.round_pool_k, l.round_pool_stride) == (0, 0) for l in cfg.layers)
    assert cfg.counts() == dict(TM.net_counts(TM.lenet5_model_config()), rounds=7)
    assert VN.pool_schedule(cfg) == [(0, 0, 0, 0)] * 7 and all(not f & VN.MAXPOOL for f, _, _ in VN.schedule(cfg))
    from vpin_amd import lenet as VL
    import tiny_lenet as TL
    tiny = VN.from_lenet(TL.make_cfg(VL))
    assert len(tiny.layers) == 7 and all((l.round_pool_k, l.round_pool_stride) == (0, 0) for l in tiny.layers)
    assert tiny.counts()["rounds"] == 7
