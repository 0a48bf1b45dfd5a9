"""The case list of the registered message sets (blsgpu_msgset_*, blsgpu_verify_msgset_batch, blsgpu_verify_msgset_indexed_batch),
shared by tests/test_msgset_cases.py (CPU: the expected statuses are the oracle's, one verification per item under the message its
group's entry holds) and tests/test_gpu_msgset.py (GPU: the calls return them).

A set is a list of messages (ENTRIES); a group names one by position.  Items are those of tests/verify_shared_cases.py: a key k g,
a signature s H(signed message), built from public scalars.  An item's expected status is BLSGPU_E_ARG when its group's index lies
outside the set, whatever else is wrong with it; otherwise what its making says under the ENTRY's message."""
import functools

import verify_shared_cases as vc
from util import ref
from verify_shared_cases import Item, valid

OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY = vc.OK, vc.INVALID_SIGNATURE, vc.SIG_IDENTITY, vc.PK_IDENTITY
E_ARG = -3
ENTRIES = [b'first entry', b'', b'alpha', b'beta', b'an entry no group names']
PAST_END = len(ENTRIES)
OUTSIDE_MSG = b'signed for a group whose entry does not exist'
COMBOS = [(sg, scheme) for sg in (1, 2) for scheme in (ref.BASIC, ref.POP)]
COMBO_IDS = ['g%d-%s' % (sg, {ref.BASIC: 'basic', ref.POP: 'pop'}[scheme]) for sg, scheme in COMBOS]


def groups_of():
    """[(entry index, [Item])]: empty groups first, in the middle and last; a group of one; two groups on one entry; the empty
    message; a tampered signature; an identity signature (with an identity key: the signature wins; and alone); an identity key; a
    signature valid under ANOTHER entry's message, both ways round between two entries that neighbouring groups name; and two groups
    whose index lies outside the set (the first index past the end, and 2^32 - 1), with items that would be OK, SIG_IDENTITY and
    PK_IDENTITY anywhere else."""
    return [
        (0, []),
        (0, [valid(11, 'a group of one')]),
        (4, []),
        (2, [valid(12), Item('tampered: signed by another key', 13, 14), Item('identity signature and identity key', 0, 0),
             Item('identity key alone', 0, 15), valid(13)]),
        (2, [valid(14, 'a second group on the same entry'), Item('valid under another entry\'s message', 17, 17, signed=b'beta')]),
        (1, [valid(15, 'an empty message'), Item('identity signature alone', 16, 0)]),
        (3, [Item('valid under the previous group\'s entry', 18, 18, signed=b'alpha'), valid(19)]),
        (PAST_END, [valid(20, 'entry index past the end'), Item('past the end, identity signature', 21, 0), Item('past the end, identity key', 0, 22)]),
        (2 ** 32 - 1, [valid(23, 'the largest index')]),
        (3, []),
    ]


def message_of(idx):
    """what an item of a group with this index is signed under when it does not say otherwise"""
    return ENTRIES[idx] if idx < len(ENTRIES) else OUTSIDE_MSG


@functools.lru_cache(maxsize=None)
def batch(sg, scheme):
    """(ENTRIES, [(entry index, [(pk point, sig point)])], [expected status per item])"""
    gs = groups_of()
    groups = [(idx, [it.points(sg, scheme, message_of(idx)) for it in items]) for idx, items in gs]
    expect = [E_ARG if idx >= len(ENTRIES) else it.expect(scheme, ENTRIES[idx]) for idx, items in gs for it in items]
    return ENTRIES, groups, expect


def names():
    return [it.name for _, items in groups_of() for it in items]


def raw_groups(sg, groups, rng=None):
    """the groups as api.verify_msgset_batch takes them: (entry index, [RAW_PROJ keys], [RAW_PROJ signatures])"""
    return [(idx, pks, sigs) for idx, (_, pks, sigs) in zip([g[0] for g in groups], vc.raw_groups(sg, [(b'', items) for _, items in groups], rng))]
