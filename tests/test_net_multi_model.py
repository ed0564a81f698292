"""Several clients in one batched inference on the models, without a GPU (vpin_net_infer_multi, vpin_net_serve_multi): the images
of three clients with three secret keys laid out in the image slots of ONE batch in wire order, every client's bias encrypted
under its own H (what vpin_e2_encrypt_keyed does: element i under key key_of[i]), every round one callback over the whole batch
that hands each client the values of its own slots.  On elgamal_model and net_batch_model (the batch driver's model on discrete
logarithms): every client decrypts the plaintext model's scores of its own images, its slots of every layer are what it gets when
it is served alone with the same slots' keys and bias r, and a bias under another client's key is not the bias.  Also the
host side of the interface: the new symbols and the ABI version."""
import numpy as np

import elgamal_model as EL
import enc_conv_model as EM
import fcs_model as TM
import net_batch_model as BM
import net_model as NM

SKS = [0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % EL.ORDER, 1, EL.ORDER - 1]
IMAGES_OF = [1, 2, 1]  # B_i per client, in wire order: slots 0, 1 .. 2, 3


def slots():
    """per client (first_image, n_images): the slots after those of the clients before it"""
    out, first = [], 0
    for n in IMAGES_OF:
        out.append((first, n))
        first += n
    return out


def encrypt_biases(model, sk_of_image, bias_r):
    """per image, per layer with a bias, its (c1, c2) under the key of the image's own client"""
    out = []
    for b, sk in enumerate(sk_of_image):
        one, pos = [], 0
        for l in model["layers"]:
            if l.get("bias") is not None:
                one.append(NM.log_encrypt(sk, l["bias"], bias_r[b][pos:pos + len(l["bias"])]))
                pos += len(l["bias"])
        assert pos == len(bias_r[b])
        out.append(one)
    return out


def roster_client(clients):
    """the round callback over the whole batch: client i is given the values of its slots and answers for them alone.
    clients: per client (first, n, its own callback)"""
    B = sum(n for _, n, _ in clients)

    def client(rnd, relu, bits, reencrypt, c1, c2):
        per = len(c1) // B
        a1, a2 = [], []
        for first, n, fn in clients:
            ans = fn(rnd, relu, bits, reencrypt, c1[first * per:(first + n) * per], c2[first * per:(first + n) * per])
            if reencrypt:
                a1 += ans[0]
                a2 += ans[1]
        return (a1, a2) if reencrypt else None

    return client


def run(d, sk_of_client):
    """the batch of all clients, every bias under the key of its image's client -> (layers, per client its rounds)"""
    sk_image = [sk for sk, n in zip(sk_of_client, IMAGES_OF) for _ in range(n)]
    enc = [NM.log_encrypt(sk, d["images"][b], d["image_r"][b]) for b, sk in enumerate(sk_image)]
    seen = [[] for _ in IMAGES_OF]
    clients = [(first, n, NM.log_client(sk, BM.client_queue(d["model"], d["client_r"][first:first + n]), seen[i]))
               for i, ((first, n), sk) in enumerate(zip(slots(), sk_of_client))]
    layers, _ = BM.infer_batch_model(EM.LOGS, d["model"], [c[0] for c in enc], [c[1] for c in enc], d["keys"],
                                     encrypt_biases(d["model"], sk_image, d["bias_r"]), roster_client(clients))
    assert all(not fn.left for _, _, fn in clients), "every client consumes exactly its own queue"
    return layers, seen


def test_three_clients_with_three_keys_each_decrypt_the_plaintext_models_scores():
    d = BM.trained_inputs(4)
    layers, seen = run(d, SKS)
    for i, (first, n) in enumerate(slots()):
        plain = [TM.net_plaintext(d["model"], np.array(d["images"][b]).reshape(1, 10, 10)) for b in range(first, first + n)]
        assert len(seen[i]) == 5
        for r, (v, act) in enumerate(seen[i]):
            assert list(v) == [x for vs, _ in plain for x in vs[r]], "client %d round %d" % (i, r)
            assert list(act) == [x for _, acts in plain for x in acts[r]], "client %d round %d" % (i, r)


def test_a_clients_slots_are_what_it_gets_served_alone_with_the_same_slots_keys():
    d = BM.trained_inputs(4)
    layers, seen = run(d, SKS)
    for i, ((first, n), sk) in enumerate(zip(slots(), SKS)):
        enc = [NM.log_encrypt(sk, d["images"][b], d["image_r"][b]) for b in range(first, first + n)]
        alone = []
        client = NM.log_client(sk, BM.client_queue(d["model"], d["client_r"][first:first + n]), alone)
        ref, _ = BM.infer_batch_model(EM.LOGS, d["model"], [c[0] for c in enc], [c[1] for c in enc], d["keys"][first:first + n],
                                      encrypt_biases(d["model"], [sk] * n, d["bias_r"][first:first + n]), client)
        assert [(list(v), list(a)) for v, a in alone] == [(list(v), list(a)) for v, a in seen[i]]
        for k, (got, exp) in enumerate(zip(layers, ref)):
            for key in ("out", "mults", "adds", "left"):
                whole = list(got.get(key, []))
                per = len(whole) // 4
                assert whole[first * per:(first + n) * per] == list(exp.get(key, [])), "client %d layer %d %s" % (i, k, key)


def test_a_bias_under_another_clients_key_is_not_the_bias():
    """why the key is per image: what client 1 decrypts of a bias encrypted under client 0's key is off by r * (sk_0 - sk_1)"""
    d = BM.trained_inputs(2)
    bias = next(l["bias"] for l in d["model"]["layers"] if l.get("bias") is not None)
    c1, c2 = NM.log_encrypt(SKS[0], bias, d["bias_r"][1][:len(bias)])
    dec = lambda sk: [(b - sk * a) % EL.ORDER for a, b in zip(c1, c2)]
    assert dec(SKS[0]) == [v % EL.ORDER for v in bias] and all(u != v % EL.ORDER for u, v in zip(dec(SKS[1]), bias))


def test_the_keyed_encryption_on_the_curve_is_the_logarithms_rule():
    """c2 = msg * G + r * H[key_of] on E2 (elgamal_model) is the model's m + r * sk[key_of] on discrete logarithms"""
    pubs = [EL.keygen(sk) for sk in SKS]
    for i, (msg, r) in enumerate([(5, 7), (-3, EL.ORDER - 1), (0, 1), (2**62 - 1, 0x1234567)]):
        k = i % 3
        c1, c2 = EL.encrypt(pubs[k], msg, r)
        l1, l2 = NM.log_encrypt(SKS[k], [msg], [r])
        assert c1 == EL.mul(l1[0]) and c2 == EL.mul(l2[0])
    # sk = 1: H = G, so msg = -r gives the identity as c2
    assert EL.encrypt(pubs[1], -9, 9)[1] is None


def test_the_binding_has_the_new_symbols():
    from vpin_amd import capi, elgamal, net
    L = capi.lib()
    assert L.vpin_abi_version() >= 7
    names = ["vpin_e2_encrypt_keyed", "vpin_net_infer_multi", "vpin_net_server_create", "vpin_net_server_free", "vpin_net_server_stats",
             "vpin_net_serve_multi"]
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in names)
    assert callable(elgamal.encrypt_keyed) and callable(net.infer_multi) and callable(net.Server)
    assert (net.STAGE_DONE, net.STAGE_ADMISSION, net.STAGE_SERVER) == (-1, -2, -3)
    import ctypes as C
    assert C.sizeof(capi.NetPeerStatus) == 4 + 4 + 4 + 4 + 256
    # the checks that need no device: every null argument is VPIN_EINVAL with its rule
    b = (C.c_uint8 * 64)()
    assert L.vpin_e2_encrypt_keyed(None, b, b, b, 1, b, b, b, 1, b, b, b, b, b, b) == -1
    assert b"vpin_e2_encrypt_keyed: null argument" in L.vpin_last_error()
    assert L.vpin_net_serve_multi(None, None, 1, None, 0, None, 0, None, None) == -1
    assert b"vpin_net_serve_multi: null argument" in L.vpin_last_error()
    assert L.vpin_net_server_create(None, None, 1, None) == -1 and L.vpin_net_server_stats(None, None) == -1
