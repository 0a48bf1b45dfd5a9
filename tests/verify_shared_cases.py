"""The case list of the shared-message verify calls (blsgpu_verify_shared_batch, blsgpu_verify_shared_indexed_batch), shared by
tests/test_verify_shared_cases.py (CPU: the expected statuses are the oracle's, one verification per item with its group's
message) and tests/test_gpu_verify_shared.py (GPU: the calls return them).

Every item is built from public scalars: a key k g, a signature s H(prefix || signed message).  Its expected status follows from
how it was made -- the signature is valid iff s = k, the signed message is the group's and (MessageAugmentation) the prefix is
the item's own key -- and tests/test_verify_shared_cases.py holds that against the oracle for every item."""
import functools

import util
from util import c, ref

OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
R = c.R
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}
COMBOS = [(sg, scheme) for sg in (1, 2) for scheme in (ref.BASIC, ref.AUG, ref.POP)]
COMBO_IDS = ['g%d-%s' % (sg, {ref.BASIC: 'basic', ref.AUG: 'aug', ref.POP: 'pop'}[scheme]) for sg, scheme in COMBOS]


class Item:
    """key: the key's scalar (0: the identity); signer: the signature's scalar (0: the identity signature); signed: the message
    that was signed (None: the group's); prefix: the scalar of the key whose bytes prefix the message under MessageAugmentation
    (None: the signer's own, what sign() does)."""

    def __init__(self, name, key, signer, signed=None, prefix=None):
        self.name, self.key, self.signer, self.signed, self.prefix = name, key % R, signer % R, signed, prefix

    def points(self, sg, scheme, msg):
        C = IMPLS[sg]
        pk = C.pk_curve.mul(C.pk_gen, self.key) if self.key else None
        if not self.signer:
            return pk, None
        m = msg if self.signed is None else self.signed
        if scheme == ref.AUG:
            pre = self.signer if self.prefix is None else self.prefix
            m = C.pk_to_bytes(C.pk_curve.mul(C.pk_gen, pre)) + m
        return pk, C.sig_curve.mul(_hash(sg, scheme, m), self.signer)

    def expect(self, scheme, msg):
        if not self.signer:
            return SIG_IDENTITY
        if not self.key:
            return PK_IDENTITY
        same_msg = self.signed is None or self.signed == msg
        same_prefix = scheme != ref.AUG or self.prefix is None and self.signer == self.key or self.prefix == self.key
        return OK if self.signer == self.key and same_msg and same_prefix else INVALID_SIGNATURE


@functools.lru_cache(maxsize=None)
def _hash(sg, scheme, m):
    C = IMPLS[sg]
    return C.hash_to_point(m, C.DST[scheme])


def valid(k, name='valid'):
    return Item(name, k, k)


def groups_of(scheme):
    """[(message, [Item])]: empty groups first, in the middle and last; a group of one; two groups with the same message; an empty
    message; identity signature and identity key in one item (the signature wins); an identity key alone; a tampered signature; a
    signature valid under the NEXT group's message at a group's last position and one valid under the PREVIOUS group's message at
    the next group's first position (an off-by-one group lookup makes either of them pass); under MessageAugmentation two items
    over the same hashed bytes, of which only the one whose own key is the prefix verifies."""
    g = [
        (b'first group is empty', []),
        (b'one', [valid(11, 'a group of one')]),
        (b'an empty group in the middle', []),
        (b'same', [valid(12), Item('tampered: signed by another key', 13, 14), Item('identity signature and identity key', 0, 0),
                   Item('identity key alone', 0, 15), valid(13)]),
        (b'same', [valid(14, 'the same message again')]),
        (b'', [valid(15, 'an empty message'), Item('identity signature alone', 16, 0)]),
        (b'alpha', [valid(16), Item('valid under the next group\'s message', 17, 17, signed=b'beta')]),
        (b'beta', [Item('valid under the previous group\'s message', 18, 18, signed=b'alpha'), valid(19)]),
    ]
    if scheme == ref.AUG:
        g.append((b'prefixed', [Item('own scalar, another key\'s prefix', 21, 21, prefix=22), Item('the prefix is the item\'s key', 22, 22, prefix=22)]))
    g.append((b'last group is empty', []))
    return g


@functools.lru_cache(maxsize=None)
def batches(sg, scheme):
    """[(name, [(message, [(pk point, sig point)]), ...], [expected status per item])]"""
    out = [('no groups', [], []), ('only empty groups', [(b'x', []), (b'', []), (b'y', [])], [])]
    gs = groups_of(scheme)
    out.append(('mixed', [(m, [it.points(sg, scheme, m) for it in items]) for m, items in gs],
                [it.expect(scheme, m) for m, items in gs for it in items]))
    return out


def names(scheme):
    return [it.name for _, items in groups_of(scheme) for it in items]


def raw_groups(sg, groups, rng=None):
    """the groups as api.verify_shared_batch takes them: (message, [RAW_PROJ keys], [RAW_PROJ signatures])"""
    pkraw, sigraw = (util.g2_raw, util.g1_raw) if sg == 1 else (util.g1_raw, util.g2_raw)
    return [(m, [pkraw(pk, rng) if pk is not None else pkraw(None) for pk, _ in items],
             [sigraw(sig, rng) if sig is not None else sigraw(None) for _, sig in items]) for m, items in groups]


def oracle_statuses(bo, sg, scheme, groups):
    """one verification per item with its group's message, by the C oracle (util.load_c_oracle): [status per item]"""
    out = []
    for m, pks, sigs in groups:
        for pk, sig in zip(pks, sigs):
            out.append(bo.bo_verify(sg, scheme, pk, sig, m, len(m)))
    return out
