"""Every expected entry of tests/agg_batch_cases.py is what the oracle's AggregateSignature::verify (oracle/py/blsful_ref.py
aggregate_verify, reference src/aggregate_signature.rs:230-239) raises for that set alone, error strings and indices included --
for both impls and the three schemes.  Sets above a few pairs (the sizes 63, 64, 65) are valid by construction; the GPU tests
compare them with the single call."""
import pytest

import agg_batch_cases as abc
import util
from util import ref

STRINGS = {
    abc.OK: lambda aux: None,
    abc.INVALID_SIGNATURE: lambda aux: ref.BlsError('InvalidSignature'),
    abc.SIG_IDENTITY: lambda aux: ref.BlsError('InvalidInputs', 'signature is the identity point'),
    abc.PK_IDENTITY: lambda aux: ref.BlsError('InvalidInputs', 'public key at %d is the identity point' % aux[0]),
    abc.DUPLICATE_MESSAGE: lambda aux: ref.BlsError('InvalidInputs', 'duplicate messages detected at %d and %d' % aux),
}


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('scheme', [ref.BASIC, ref.AUG, ref.POP])
def test_expected_entries_are_the_oracles(sg, scheme):
    C = abc.IMPLS[sg]
    checked = pairs_checked = 0
    for name, pairs, sig, (st, aux) in abc.cases(sg, scheme, big=False):
        assert len(pairs) <= abc.ORACLE_MAX_PAIRS
        try:
            ref.aggregate_verify(C, scheme, pairs, sig)
            got = None
        except ref.BlsError as e:
            got = e
        assert got == STRINGS[st](aux), (name, got)
        if st not in (abc.PK_IDENTITY, abc.DUPLICATE_MESSAGE):
            assert aux == (0, 0), name
        checked += 1
        pairs_checked += len(pairs)
    assert checked >= 19 and pairs_checked <= 64


def test_kinds_present():
    """The list holds every kind of set the batched call has to tell apart, under Basic with the duplicate rule and without it otherwise."""
    for scheme in (ref.BASIC, ref.AUG, ref.POP):
        cl = abc.cases(2, scheme, big=scheme == ref.BASIC)
        sts = [e[0] for _, _, _, e in cl]
        assert {abc.OK, abc.INVALID_SIGNATURE, abc.SIG_IDENTITY, abc.PK_IDENTITY} <= set(sts)
        assert (abc.DUPLICATE_MESSAGE in sts) == (scheme == ref.BASIC)
        if scheme == ref.BASIC:
            assert sorted(len(p) for n, p, _, _ in cl if n.startswith('size ') and ',' not in n) == [1, 2, 3, 63, 64, 65]
            assert all(e[0] in (abc.OK, abc.INVALID_SIGNATURE) and e[1] == (0, 0) for _, p, _, e in cl if len(p) > abc.ORACLE_MAX_PAIRS)
        assert any(len(p) == 0 and s is None for _, p, s, _ in cl) and any(len(p) == 0 and s is not None for _, p, s, _ in cl)
    # the message both neighbouring sets hold is a duplicate only inside one set
    by_name = {n: (p, e) for n, p, _, e in abc.cases(1, ref.BASIC, big=False)}
    a, b = by_name['same message as the next set'], by_name['same message as the set before']
    assert {m for _, m in a[0]} & {m for _, m in b[0]} == {b'shared'} and a[1][0] == b[1][0] == abc.OK


def test_raw_sets_shapes():
    for sg, pk_len, sig_len in ((1, 288, 144), (2, 144, 288)):
        cl = abc.cases(sg, ref.POP, big=False)
        for (pks, msgs, sig), (_, pairs, _, _) in zip(abc.raw_sets(sg, cl), cl):
            assert len(pks) == len(msgs) == len(pairs) and all(len(p) == pk_len for p in pks) and len(sig) == sig_len
