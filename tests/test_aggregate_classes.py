"""The error cases of MultiSignature.from_signatures, AggregateSignature.from_signatures and
AggregateSignature.from_signatures_secure that the reference decides before any curve arithmetic (src/multi_signature.rs:80-107,
src/aggregate_signature.rs:123-148,191-227), and the same cases through the *_many helpers.  None of them reaches the library,
so this runs on a machine with no device: a call that did reach it would raise BlsGpuRuntimeError here, not BlsError."""
import pytest


@pytest.fixture(scope='module')
def m(pkg):
    return pkg


def sig(m, scheme, impl=None):
    return m.Signature(impl or m.Bls12381G1Impl, scheme, b'\0' * 144)


def key(m, impl=None):
    return m.PublicKey(impl or m.Bls12381G1Impl, b'\0' * 288)


def kind(m, fn, *a):
    with pytest.raises(m.BlsError) as e:
        fn(*a)
    return e.value


def test_multi_signature_from_signatures_errors(m):
    f = m.MultiSignature.from_signatures
    B, A, P = m.BASIC, m.AUG, m.POP
    assert kind(m, f, []) == m.BlsError('InvalidSignature')
    assert kind(m, f, [sig(m, B)]) == m.BlsError('InvalidSignature')
    assert kind(m, f, [sig(m, B), sig(m, P)]) == m.BlsError('InvalidSignatureScheme')
    assert kind(m, f, [sig(m, P), sig(m, P), sig(m, B)]) == m.BlsError('InvalidSignatureScheme')
    # a MessageAugmentation signature at any position after the first (reference :92-97), the all-Aug list included
    assert kind(m, f, [sig(m, A), sig(m, A)]) == m.BlsError('InvalidSignatureScheme')
    assert kind(m, f, [sig(m, A), sig(m, A), sig(m, A)]) == m.BlsError('InvalidSignatureScheme')
    assert kind(m, f, [sig(m, B), sig(m, A)]) == m.BlsError('InvalidSignatureScheme')
    # one signature is too few whatever its scheme: the length check comes first
    assert kind(m, f, [sig(m, A)]) == m.BlsError('InvalidSignature')


def test_aggregate_signature_from_signatures_errors(m):
    f = m.AggregateSignature.from_signatures
    B, A, P = m.BASIC, m.AUG, m.POP
    assert kind(m, f, []) == m.BlsError('InvalidSignature')
    assert kind(m, f, [sig(m, A)]) == m.BlsError('InvalidSignature')
    assert kind(m, f, [sig(m, B), sig(m, A)]) == m.BlsError('InvalidSignatureScheme')
    assert kind(m, f, [sig(m, A), sig(m, A), sig(m, P)]) == m.BlsError('InvalidSignatureScheme')
    assert kind(m, f, (sig(m, P, m.Bls12381G2Impl), sig(m, B, m.Bls12381G2Impl))) == m.BlsError('InvalidSignatureScheme')


def test_from_signatures_secure_errors(m):
    f = m.AggregateSignature.from_signatures_secure
    B, A = m.BASIC, m.AUG
    assert kind(m, f, [sig(m, B)], []) == m.BlsError('InvalidInputs', 'Mismatched array lengths')
    assert kind(m, f, [], [key(m)]) == m.BlsError('InvalidInputs', 'Mismatched array lengths')
    assert kind(m, f, [], []) == m.BlsError('InvalidInputs', 'Empty signatures array')
    assert kind(m, f, [sig(m, B), sig(m, A)], [key(m), key(m)]) == m.BlsError('InvalidSignatureScheme')
    # the reference's order: lengths, then emptiness, then schemes
    assert kind(m, f, [sig(m, B), sig(m, A)], [key(m)]) == m.BlsError('InvalidInputs', 'Mismatched array lengths')


def test_many_helpers_decide_errors_on_the_host(m):
    B, A, P = m.BASIC, m.AUG, m.POP
    g2 = m.Bls12381G2Impl
    assert m.multi_signatures_many([]) == [] and m.aggregate_signatures_many([]) == [] and m.aggregate_secure_many([]) == []
    lists = [[sig(m, B)], [sig(m, A), sig(m, A)], [sig(m, P, g2), sig(m, B, g2)], []]
    assert m.multi_signatures_many(lists) == [m.BlsError('InvalidSignature'), m.BlsError('InvalidSignatureScheme'),
                                              m.BlsError('InvalidSignatureScheme'), m.BlsError('InvalidSignature')]
    assert m.aggregate_signatures_many(lists[::2]) == [m.BlsError('InvalidSignature'), m.BlsError('InvalidSignatureScheme')]
    got = m.aggregate_secure_many([([sig(m, B)], []), ([], []), ([sig(m, B, g2), sig(m, P, g2)], [key(m, g2), key(m, g2)], m.LEGACY)])
    assert got == [m.BlsError('InvalidInputs', 'Mismatched array lengths'), m.BlsError('InvalidInputs', 'Empty signatures array'),
                   m.BlsError('InvalidSignatureScheme')]


def test_flat_call_refuses_unequal_lists_before_the_library(m):
    with pytest.raises(ValueError):
        m.api.aggregate_secure_batch(1, [([b'\0' * 288], [])])


def test_exports_name_the_new_entry_points(m):
    assert 'blsgpu_aggregate_secure_batch' in m.api.EXPORTS and 'blsgpu_sum_batch' in m.api.EXPORTS
