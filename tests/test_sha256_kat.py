"""Known answers for the library's SHA-256 (vpin_sha256: the digest vpin_snark_verify_batch binds its weights to every item
with).  FIPS 180-4 / NIST example vectors, and every length around the block and padding boundaries against hashlib.  CPU only:
the function touches no device."""
import hashlib

import vpin_amd

VECTORS = [
    (b"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"),
    (b"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"),
    (b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu",
     "cf5b16a778af8380036ce59e7b0492370b249b11e8f07a51afac45037afee9d1"),
    (b"a" * 1000000, "cdc76e5c9914fb9281a1c7e284d73e67f1809a48a497200e046d39ccc7112cd0"),
]


def test_fips_180_4_vectors():
    for msg, want in VECTORS:
        assert hashlib.sha256(msg).hexdigest() == want  # the vectors themselves
        assert vpin_amd.sha256(msg).hex() == want, len(msg)


def test_every_length_around_the_block_boundaries():
    data = bytes((37 * i + 11) % 256 for i in range(300))
    for n in range(0, 300):
        assert vpin_amd.sha256(data[:n]) == hashlib.sha256(data[:n]).digest(), n
