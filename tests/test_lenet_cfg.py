"""The LeNet configuration behind the C ABI without a GPU (vpin_lenet_cfg_default, vpin_lenet_cfg_counts through
vpin_amd.lenet): the default configuration around the reference's weights consumes what the reference's run consumes, its label
counts are the LENET table's, and a configuration the architecture does not allow is rejected."""
import pytest

import lenet_model as LM
from vpin_amd import build as vbuild
from vpin_amd import gadgets as VG


@pytest.fixture(scope="module")
def VL():
    vbuild.build()
    from vpin_amd import lenet
    return lenet


@pytest.fixture(scope="module")
def cfg(VL):
    _, w1, b1, w2, b2 = LM.reference_model()
    return VL.default_config(w1, b1, w2, b2)


def test_default_counts(cfg):
    c = cfg.counts()
    assert (c["encryptions"], c["decryptions"], c["prf_keys"], c["bias_r"]) == (9108, 8094, 288, 94)
    assert c["labels"] == [(VG.CONFIGS[l]["n_mult"], VG.CONFIGS[l]["n_add"]) for l in VG.LENET]
    model = LM.counts(LM.default_config())
    assert c == dict(model, labels=[tuple(l) for l in model["labels"]])


def test_default_schedule_and_ranges(cfg):
    c = cfg.c
    assert (c.H, c.W, c.n1, c.n2, c.n3, c.f, c.pool_k, c.pool_stride, c.prf_bytes, c.N1, c.N2) == (32, 32, 6, 16, 120, 5, 2, 2, 13, 84, 10)
    model = LM.default_config()
    assert [(c.relu[r], c.shift_bits[r]) for r in range(7)] == model["rounds"]
    assert int.from_bytes(bytes(c.pool_scale_le16), "little") == model["pool_scale"]
    # with the default table of 2^24 baby steps R6 and R7 reach at least 2^39, the others the 2^35 of vpin_amd.elgamal
    assert all(c.max_giant[r] << 24 >= 2**39 for r in (5, 6)) and all(c.max_giant[r] << 24 >= 2**35 for r in range(5))


def test_preprocess_is_the_models(VL):
    import numpy as np
    import os
    img = np.load(os.path.join(LM.GOLDEN, "image_mnist_32_32.npy"))
    assert np.array_equal(VL.preprocess(img), LM.preprocess(img))


def test_rejected_configurations(VL, cfg):
    import vpin_amd

    def einval(change, match):
        _, w1, b1, w2, b2 = LM.reference_model()
        bad = VL.default_config(w1, b1, w2, b2)
        change(bad)
        with pytest.raises(vpin_amd.VpinError, match=match) as e:
            bad.counts()
        assert e.value.code == -1

    einval(lambda b: setattr(b.c, "H", 36) or setattr(b.c, "W", 36), "1 x 1")       # conv3 would give 2 x 2
    einval(lambda b: setattr(b.c, "H", 16) or setattr(b.c, "W", 16), "does not fit")  # 16 -> 12 -> 6 -> 2 -> pool 1: no 5 x 5 window
    einval(lambda b: setattr(b.c, "n3", 0), "zero")
    einval(lambda b: b.connect.__setitem__((3, slice(None)), 0), "selects no plane")
    einval(lambda b: setattr(b.c, "prf_bytes", 17), "prf_bytes")
