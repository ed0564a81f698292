"""GPU test of a batch of images between two endpoints over a byte stream (vpin_net_serve_batch against vpin_net_client_run, which
needs nothing new): the small trained network with B = 2 as two threads over a socketpair and two contexts, the server allowing
up to 4 images and reading B off the INPUT frame, against vpin_net_infer_batch in process on the same inputs -- every layer, the
label and every round byte for byte, the bytes on the wire exactly the formula of the single run at the batch's counts.  Then the
refusals on the one-layer network of test_gpu_net_wire.py: each ends both sides with an error return, and the same contexts run a
good batch again.  vpin_net_serve itself still takes one image and says so in its own words."""
import re

import numpy as np
import pytest

import elgamal_model as EL
import fcs_model as TM
import net_batch_model as BM
from test_gpu_net_batch import assert_views_are, views
from test_gpu_net_wire import Pair, assert_traffic, both, ints, small_model

pytestmark = pytest.mark.gpu

NB = 1 << 16
GIANTS = [1 << 14] * 5
SK = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER


@pytest.fixture(scope="module")
def ctxs():
    """the server's context and the client's"""
    import vpin_amd
    a, b = vpin_amd.Context(0), vpin_amd.Context(0)
    yield a, b
    b.close()
    a.close()


@pytest.mark.timeout(240)
def test_a_batch_of_two_over_a_socketpair_is_the_batch_in_process(ctxs):
    from vpin_amd import net as VN
    d = BM.trained_inputs(4)  # the server holds the keys and bias r of max_batch = 4 images; two arrive
    cfg = TM.device_config(d["model"], GIANTS)
    queue = BM.client_queue(d["model"], d["client_r"][:2])
    client = VN.Client(ctxs[0], SK, NB, GIANTS, queue)
    ref_scores, ref_rounds, ref = VN.infer_batch(ctxs[0], cfg, client, d["images"][:2], d["image_r"][:2], d["keys"][:2], d["bias_r"][:2])
    client.free()
    sched = VN.schedule(cfg, batch=2)
    assert sched == [(3, 28, 256), (2, 17, 64), (3, 20, 54), (3, 21, 8), (0, 0, 6)]
    client = VN.Client(ctxs[1], SK, NB, GIANTS, queue)
    pair = Pair()
    trace, res = both(lambda: VN.serve(ctxs[0], cfg, pair.server, BM.flat(d["keys"]), BM.flat(d["bias_r"]), max_batch=4),
                      lambda: client.run(pair.client, BM.flat(d["images"][:2]), BM.flat(d["image_r"][:2]), sched))
    assert not isinstance(trace, BaseException), trace
    assert not isinstance(res, BaseException), res
    scores, rounds = res
    assert ints(rounds) == ints(ref_rounds) and len(rounds) == 5
    for b in range(2):
        acts = TM.net_plaintext(d["model"], np.array(d["images"][b]).reshape(1, 10, 10))[1]
        assert [int(a) for a in scores.reshape(2, -1)[b]] == acts[-1] == [int(a) for a in ref_scores[b]]
    assert trace.images == ref.images == 2 and trace.n_layers == ref.n_layers == 5
    for i in range(5):
        assert_views_are(views(trace.layer(i)), [views(ref.layer(i))], "layer %d" % i)
    assert_views_are(views(trace.label(), left=False), [views(ref.label(), left=False)], "the label")
    for b in range(2):
        assert_views_are(views(trace.image_label(b), left=False), [views(ref.image_label(b), left=False)], "the label of image %d" % b)
    assert_traffic(200, sched, pair.client.stats(), pair.server.stats())
    trace.free()
    ref.free()
    client.free()
    pair.close()


# ---- refusals, on the one-layer network of two ciphertexts per image ---------------------------------------------------------------
IMAGES = [[3, -50, 7, 9, 11, 13, 15, -17], [-4, 8, 21, -6, 10, 2, -30, 5], [1, 2, 3, 4, 5, 6, 7, 8]]
IMAGE_R = [EL.splitmix_scalars(0x7C1 + b, 8) for b in range(3)]


@pytest.fixture(scope="module")
def small(ctxs):
    from vpin_amd import net as VN
    cfg = TM.device_config(small_model(), [4])
    client = VN.Client(ctxs[1], SK, NB, [4], EL.splitmix_scalars(0x7C9, 64))
    yield dict(cfg=cfg, client=client)
    client.free()


def good_batch(ctxs, small):
    """two images over the same contexts and client: the plaintext model's values of both, image-major"""
    from vpin_amd import net as VN
    pair = Pair()
    sched = VN.schedule(small["cfg"], batch=2)
    assert sched == [(3, 0, 4)]
    trace, res = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], [], max_batch=2),
                      lambda: small["client"].run(pair.client, BM.flat(IMAGES[:2]), BM.flat(IMAGE_R[:2]), sched))
    assert not isinstance(trace, BaseException), trace
    assert not isinstance(res, BaseException), res
    plain = [TM.net_plaintext(small_model(), np.array(im).reshape(1, 2, 4)) for im in IMAGES[:2]]
    assert ints(res[1]) == [(plain[0][0][0] + plain[1][0][0], plain[0][1][0] + plain[1][1][0])] and ints(res[1])[0][1] == [0, 14, 16, 0]
    assert trace.images == 2 and trace.layer(0).P == 4
    assert_traffic(16, sched, pair.client.stats(), pair.server.stats())
    trace.free()
    pair.close()


@pytest.mark.timeout(60)
def test_the_small_batch_runs(ctxs, small):
    good_batch(ctxs, small)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("n_input, text", [(3 * 8, "cnt 24"), (8 + 1, "cnt 9")], ids=["three images against max_batch 2", "not a multiple of C H W"])
def test_an_input_that_is_no_batch_the_server_takes_is_eshape_on_both_sides(ctxs, small, n_input, text):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    image = (BM.flat(IMAGES) + [1])[:n_input]
    server, client = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], [], max_batch=2),
                          lambda: small["client"].run(pair.client, image, EL.splitmix_scalars(0x7CA, n_input), VN.schedule(small["cfg"], batch=3)))
    want = "vpin_net_serve_batch: expected INPUT of 1 .. 2 images of 8 ciphertexts, the peer sent " + text
    assert isinstance(server, vpin_amd.VpinError) and server.code == -5 and want in str(server), server  # VPIN_ESHAPE
    assert isinstance(client, vpin_amd.VpinError) and client.code == -7, client                           # VPIN_ECOMM: the ERROR frame
    assert "the peer reported an error (-5)" in str(client) and want in str(client), client
    pair.close()
    good_batch(ctxs, small)


@pytest.mark.timeout(60)
def test_a_schedule_for_one_image_against_an_input_of_two_is_refused_by_the_client(ctxs, small):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    server, client = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], [], max_batch=2),
                          lambda: small["client"].run(pair.client, BM.flat(IMAGES[:2]), BM.flat(IMAGE_R[:2]), VN.schedule(small["cfg"])))
    text = "round 0: the server sends 4 ciphertexts, the schedule says 2"
    assert isinstance(client, vpin_amd.VpinError) and client.code == -5 and re.search(text, str(client)), client
    assert isinstance(server, vpin_amd.VpinError) and server.code == -7, server
    assert "the peer reported an error (-5)" in str(server) and re.search(text, str(server)), server
    pair.close()
    good_batch(ctxs, small)


@pytest.mark.timeout(60)
def test_the_single_endpoint_still_takes_one_image_in_its_own_words(ctxs, small):
    import vpin_amd
    from vpin_amd import net as VN
    pair = Pair()
    server, client = both(lambda: VN.serve(ctxs[0], small["cfg"], pair.server, [], []),
                          lambda: small["client"].run(pair.client, BM.flat(IMAGES[:2]), BM.flat(IMAGE_R[:2]), VN.schedule(small["cfg"], batch=2)))
    want = "vpin_net_serve: expected INPUT of 8 ciphertexts, the peer sent type 2 with cnt 16"
    assert isinstance(server, vpin_amd.VpinError) and server.code == -5 and want in str(server), server
    assert isinstance(client, vpin_amd.VpinError) and client.code == -7 and want in str(client), client
    pair.close()
    good_batch(ctxs, small)
