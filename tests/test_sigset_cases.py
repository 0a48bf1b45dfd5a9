"""What tests/sigset_cases.py claims for itself, checked on the CPU: every group's signature is an entry, every item names the entry
of its group, no two neighbours share an entry, the two extra items name n and 0xffffffff, every status class is present, and the two
precedence pairs are pinned -- a bad u under a bad entry gives u's status, a wrong tag under an identity entry gives INVALID_SCHEME.
The expectations themselves are the by-value list's (tests/test_timecrypt_cases.py checks those against the oracle)."""
import pytest

import sigset_cases as sc
import timecrypt_cases as tc

CASES = [(sg, fmt) for sg in (1, 2) for fmt in tc.FMTS]


@pytest.mark.parametrize('sg,fmt', CASES, ids=['sg%d-%s' % (sg, tc.FMT_IDS[fmt]) for sg, fmt in CASES])
def test_the_list_is_the_by_value_list_by_index(sg, fmt):
    wire = fmt in (tc.COMPRESSED, tc.LEGACY)
    entries, est, items, msgs, sts, names = sc.render(sg, fmt)
    groups = [g for g in tc.timelock_groups(sg) if wire or not g['sig_bad']]
    n = len(entries)
    assert n == len(groups) == len(est) and [t for _, t in entries] == [g['scheme'] for g in groups]
    assert all(len(b) == sg * {tc.RAW_PROJ: 144, tc.RAW_AFFINE: 96, tc.COMPRESSED: 48, tc.LEGACY: 48}[fmt] for b, _ in entries)
    # the entries of the empty groups, the identity and (on the wire) the undecodable signature are there
    assert sum(1 for g in groups if not g['items']) >= 3 and any(g['sig'] is None for g in groups)
    assert [s != tc.OK for s in est] == [bool(g['sig_bad']) for g in groups] and (any(est) == wire)
    # every item of the by-value list once, under its own group's entry, with that list's expectation
    _, want_msgs, want_sts = tc.render_groups(sg, tc.timelock_groups(sg), fmt)
    inside = [i for i, it in enumerate(items) if it[0] < n]
    assert len(inside) == len(want_sts) == len(items) - 2
    by_name = {}
    for k, g in enumerate(groups):
        for it in g['items']:
            if wire or not it['u_bad']:
                by_name[it['name']] = (k, tc.expected_item(sg, g, it, fmt), it)
    assert len(by_name) == len(inside)
    for i in inside:
        k, (st, m), it = by_name[names[i]]
        assert items[i][0] == k and (sts[i], msgs[i]) == (st, m) and items[i][2:] == (it['v'], it['w'], it['scheme']), names[i]
    assert sorted(sts[i] for i in inside) == sorted(want_sts) and sorted(m or b'' for m in msgs) == sorted(m or b'' for m in want_msgs + [None, None])
    # no two neighbours share an entry; the two extra items
    assert all(a[0] != b[0] for a, b in zip(items, items[1:]))
    outside = [i for i, it in enumerate(items) if it[0] >= n]
    assert [items[i][0] for i in outside] == [n, sc.NO_ENTRY] and outside[1] == len(items) - 1 and 0 < outside[0] < len(items) - 2
    assert all(sts[i] == sc.E_ARG and msgs[i] is None for i in outside)
    assert all((m is not None) == (s == tc.OK) for m, s in zip(msgs, sts))
    # every status class
    classes = {tc.OK, tc.INVALID_SIGNATURE, tc.SIG_IDENTITY, tc.PK_IDENTITY, tc.INVALID_SCHEME, tc.BAD_FRAME, sc.E_ARG}
    assert set(sts) - {tc.BAD_ENCODING, tc.LEGACY_FORMAT} == classes
    assert bool(set(sts) & {tc.BAD_ENCODING, tc.LEGACY_FORMAT}) == wire
    # the precedence pairs
    at = {nm: i for i, nm in enumerate(names)}
    assert sts[at['identity signature and scheme mismatch']] == tc.INVALID_SCHEME and sts[at['identity signature']] == tc.SIG_IDENTITY
    assert groups[items[at['identity signature and scheme mismatch']][0]]['sig'] is None
    if wire:
        i = at['undecodable signature and u']
        u_st, e_st = tc.decode_status(3 - sg, items[i][1], fmt), est[items[i][0]]
        assert u_st != tc.OK and e_st != tc.OK and sts[i] == u_st
        assert sts[at['undecodable signature']] == e_st and sts[at['undecodable signature and scheme mismatch']] == e_st


def test_a_bad_u_under_a_bad_entry_is_told_apart_on_one_format():
    """the pair pins the order only where the two decode statuses differ: under LEGACY the entry's stray header bit is LEGACY_FORMAT
    and the u out of range is BAD_ENCODING"""
    seen = set()
    for sg in (1, 2):
        entries, est, items, _, sts, names = sc.render(sg, tc.LEGACY)
        i = names.index('undecodable signature and u')
        seen.add((sts[i], est[items[i][0]]))
    assert any(a != b for a, b in seen), seen


@pytest.mark.parametrize('sg', [1, 2])
def test_the_tiled_list(sg):
    """4,097 items over about ten entries that all have usable rows"""
    entries, items, msgs, sts = sc.tiled(sg, tc.RAW_AFFINE, 4097)
    assert 8 <= len(entries) <= 12 and len(items) == len(msgs) == len(sts) == 4097
    assert {k for k, *_ in items} == set(range(len(entries))) and all(b != bytes(len(b)) for b, _ in entries)
    assert {tc.OK, tc.INVALID_SIGNATURE, tc.PK_IDENTITY, tc.INVALID_SCHEME, tc.BAD_FRAME} <= set(sts)
