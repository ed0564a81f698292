"""What tests/test_gpu_pool_poison.py shares: the poison words, contexts whose pool fills every block it hands out
(vpin_ctx_set_pool_poison), and the bracket that shows the fill happened.

The words.  A block that comes fresh from the driver is zeroed, and a block that a test recycles by repeating a call holds the right
bytes of the identical previous call; under either a kernel that reads before it writes, reads past its length into the tail of
the size class, or lacks a zero-fill still computes the right answer.  0x00000001 and 0x00000100 are both valid small indices,
counts and field elements, so a stale read gives wrong bytes and never a wild address; between them they set byte 0 and byte 1 of
every word, so a byte-flag array (inf, bad, found, par) reads "set" under one of them wherever its alignment puts the flag."""
import contextlib

WORDS = (0x00000001, 0x00000100)


def poisoned_context(word, device=0, **kw):
    """a Context whose pool poisons from its first block on"""
    import vpin_amd
    c = vpin_amd.Context(device, **kw)
    c.set_pool_poison(word)
    return c


@contextlib.contextmanager
def filled(*ctxs):
    """the scenario inside ran on recycled-or-fresh blocks that were all filled: every context's counters moved, and by whole size
    classes (a class is at least 256 bytes)"""
    before = [c.pool_poison_stats() for c in ctxs]
    yield
    for c, (b0, n0) in zip(ctxs, before):
        b1, n1 = c.pool_poison_stats()
        assert b1 > b0, "no block was poisoned: the scenario ran without the pool, or the switch is off"
        assert n1 - n0 >= 256 * (b1 - b0) and (n1 - n0) % 256 == 0, (b1 - b0, n1 - n0)


class Ranks:
    """makes the contexts of a several-rank proof poisoned ones and keeps their counters past their close"""

    def __init__(self, word):
        self.word, self.stats = word, []

    def __call__(self, device):
        c = poisoned_context(self.word, device)
        close = c.close

        def closing():
            self.stats.append(c.pool_poison_stats())
            close()

        c.close = closing
        return c


CHILD = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
import vpin_amd
from vpin_amd import gadgets as G
word = %(word)d
c = vpin_amd.Context(0)
c.set_pool_poison(word)
for label, kind in %(cases)r:
    inp = G.synthetic_mult_inputs(label) if kind == 'mult' else G.synthetic_add_inputs(label)
    before = c.pool_poison_stats()
    d = c.gadget_point_mult_dev(*inp) if kind == 'mult' else c.gadget_point_add_dev(*inp)
    r = d.snark_prove(bytes(range(64)), bytes((7 * i + 3) %% 256 for i in range(64)))
    d.free()
    assert c.pool_poison_stats()[0] > before[0]
    print(hashlib.sha256(r['proof']).hexdigest())
c.close()
"""
