"""The CPU restatement of the ElGamal checks (tests/merlin_ref.py, tests/elgamal_cases.py): the pins of the transcript, the
model's own verdict on every case of the list, and that the list covers every status."""
import random

import pytest

import elgamal_cases as ec
import merlin_ref
from util import c

R = c.R


def test_keccak_f_of_zero():
    assert merlin_ref.keccak_f1600([0] * 25)[0] == 0xF1258F7940E1DDE7


def test_merlin_published_vector():
    t = merlin_ref.Transcript(b'test protocol')
    t.append_message(b'some label', b'some data')
    assert t.challenge_bytes(b'challenge', 32).hex() == 'd5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615'


def test_scalar_from_bytes_wide():
    assert ec.scalar_from_bytes_wide(bytes([1]) + bytes(63)) == 1
    assert ec.scalar_from_bytes_wide(bytes(32) + bytes([1]) + bytes(31)) == 2 ** 256 % R
    assert ec.scalar_from_bytes_wide(b'\xff' * 64) == (2 ** 512 - 1) % R


EXPECT = {
    'honest': ec.OK, 'custom generator': ec.OK, 'default generator given explicitly': ec.OK, 'r = 0': ec.OK, 'r = 0, custom generator': ec.OK,
    'honest with pk = G': ec.OK, 'honest with pk = H': ec.OK, 'honest with generator = G': ec.OK, 'honest with m = 0': ec.OK,
    'b = 0': ec.IDENTITY, 'all identity': ec.IDENTITY, 'mp = r with c1 identity (deserialisation first)': ec.BAD_ENCODING,
}


@pytest.mark.parametrize('sg', [1, 2])
def test_model_verdicts(sg):
    cl = ec.cases(sg)
    assert len({cs.name for cs in cl}) == len(cl)
    for cs in cl:
        if cs.name in EXPECT:
            want = EXPECT[cs.name]
        elif cs.name.endswith(('= r', '= 2^256 - 1')):
            want = ec.BAD_ENCODING
        elif 'identity' in cs.name:
            want = ec.IDENTITY               # alone and together with a zero scalar: the identity check comes first
        elif cs.name.endswith(' zero'):
            want = ec.ZERO_PROOF
        else:
            want = ec.CHALLENGE_MISMATCH     # tampered, wrong key or generator, hand-made related bases
        assert cs.expect == want, cs.name
    assert {cs.expect for cs in cl} == {ec.OK, ec.BAD_ENCODING, ec.IDENTITY, ec.ZERO_PROOF, ec.CHALLENGE_MISMATCH}
    for name in EXPECT:
        assert any(cs.name == name for cs in cl), name


@pytest.mark.parametrize('sg', [1, 2])
def test_related_bases_reach_the_exceptional_sums(sg):
    """The hand-made cases do produce r1 = identity (P - P) and equal summands (P + P): the joint ladder has to get them right."""
    g = ec.kg(sg)
    by = {cs.name: cs for cs in ec.cases(sg)}
    for name in ('c1 = G, ch = bp', 'c1 = -G, -ch = bp'):
        cs = by[name]
        assert g.add(g.mul(cs.c1, -cs.ch), g.mul(g.gen, cs.bp)) is None
    cs = by['c1 = G, -ch = bp']
    assert g.mul(cs.c1, -cs.ch) == g.mul(g.gen, cs.bp)
    cs = by['r = 0']
    assert g.add(g.mul(cs.c1, -cs.ch), g.mul(g.gen, cs.bp)) is None


@pytest.mark.parametrize('sg', [1, 2])
def test_from_shares_and_decrypt(sg):
    """elgamal_ciphertext_works of the reference: the sum of three ciphertexts, opened from threshold shares of the key."""
    g = ec.kg(sg)
    rng = random.Random(5 + sg)
    sk, a1 = rng.randrange(1, R), rng.randrange(1, R)
    pk = g.mul(g.gen, sk)
    H = g.message_generator()
    ms = [rng.randrange(1, 1000) for _ in range(3)]
    cts = [ec.seal_scalar(g, pk, m, H, rng.randrange(1, R)) for m in ms]
    c1 = c2 = None
    for a, b in cts:
        c1, c2 = g.add(c1, a), g.add(c2, b)
    shares = [(x, g.mul(c1, (sk + a1 * x) % R)) for x in (1, 2, 3)]
    st, key = ec.from_shares(g, shares[:2])
    assert st == ec.OK and key == g.mul(c1, sk)
    assert ec.decrypt(g, key, c2) == g.mul(H, sum(ms))
    assert ec.from_shares(g, shares[:1])[0] == ec.VSSS_ERROR
    assert ec.from_shares(g, [shares[0], shares[0]])[0] == ec.VSSS_ERROR
    assert ec.from_shares(g, [(0, shares[0][1]), shares[1]])[0] == ec.VSSS_ERROR
    assert ec.from_shares(g, [(R, shares[0][1]), shares[1]])[0] == ec.BAD_ENCODING
