"""The model of tests/msgset_cases.py against the oracle: every item of the case list, for both orientations under Basic and
ProofOfPossession, verified on its own under the message its group's ENTRY holds (the C oracle's Signature::verify, pinned by the
reference's known-answer vectors in tests/test_oracle_c.py).  An item whose group names no entry is BLSGPU_E_ARG by the calls' rule;
the oracle says what it would have been under the message it was signed for, so that only the index can explain the E_ARG.  The
list holds every kind of item and group the calls distinguish."""
import random

import pytest

import msgset_cases as mc
import util


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


@pytest.mark.parametrize('sg,scheme', mc.COMBOS, ids=mc.COMBO_IDS)
def test_expected_statuses_are_the_oracles(bo, sg, scheme):
    entries, groups, expect = mc.batch(sg, scheme)
    raw = mc.raw_groups(sg, groups, random.Random(10 * sg + scheme))
    got, elsewhere = [], []
    for idx, pks, sigs in raw:
        for pk, sig in zip(pks, sigs):
            if idx < len(entries):
                got.append(bo.bo_verify(sg, scheme, pk, sig, entries[idx], len(entries[idx])))
            else:
                got.append(mc.E_ARG)
                elsewhere.append(bo.bo_verify(sg, scheme, pk, sig, mc.OUTSIDE_MSG, len(mc.OUTSIDE_MSG)))
    assert got == expect and len(expect) == sum(len(items) for _, items in groups)
    assert elsewhere == [mc.OK, mc.SIG_IDENTITY, mc.PK_IDENTITY, mc.OK]


@pytest.mark.parametrize('sg,scheme', mc.COMBOS, ids=mc.COMBO_IDS)
def test_cross_entry_items_pass_under_the_other_entry(bo, sg, scheme):
    """what makes the two items a test of the entry lookup: each verifies under the entry its group does NOT name"""
    entries, groups, expect = mc.batch(sg, scheme)
    raw = mc.raw_groups(sg, groups)
    nm = mc.names()
    flat = [(idx, pk, sig) for idx, pks, sigs in raw for pk, sig in zip(pks, sigs)]
    for name, other in (('valid under another entry\'s message', 3), ('valid under the previous group\'s entry', 2)):
        i = nm.index(name)
        idx, pk, sig = flat[i]
        assert idx != other and expect[i] == mc.INVALID_SIGNATURE
        assert bo.bo_verify(sg, scheme, pk, sig, entries[other], len(entries[other])) == mc.OK


def test_kinds_present():
    gs = mc.groups_of()
    sizes = [len(items) for _, items in gs]
    idxs = [idx for idx, _ in gs]
    assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and 1 in sizes                     # empty groups, a group of one
    assert sum(1 for idx, items in gs if idx == 2 and items) == 2                                  # two groups on one entry
    assert mc.ENTRIES[1] == b'' and any(idx == 1 and items for idx, items in gs)                    # the empty message
    assert mc.PAST_END in idxs and 2 ** 32 - 1 in idxs and max(i for i in idxs if i < mc.PAST_END) < len(mc.ENTRIES)
    assert 4 not in [idx for idx, items in gs if items]                                            # an entry no item uses
    for sg, scheme in mc.COMBOS:
        expect = mc.batch(sg, scheme)[2]
        nm = mc.names()
        assert set(expect) == {mc.OK, mc.INVALID_SIGNATURE, mc.SIG_IDENTITY, mc.PK_IDENTITY, mc.E_ARG}
        assert expect[nm.index('tampered: signed by another key')] == mc.INVALID_SIGNATURE
        assert expect[nm.index('valid under another entry\'s message')] == mc.INVALID_SIGNATURE
        assert expect[nm.index('identity signature and identity key')] == mc.SIG_IDENTITY           # the signature wins
        assert expect[nm.index('identity signature alone')] == mc.SIG_IDENTITY
        assert expect[nm.index('identity key alone')] == mc.PK_IDENTITY
        assert expect[nm.index('an empty message')] == mc.OK
        assert [expect[nm.index(n)] for n in ('entry index past the end', 'past the end, identity signature', 'past the end, identity key',
                                              'the largest index')] == [mc.E_ARG] * 4
