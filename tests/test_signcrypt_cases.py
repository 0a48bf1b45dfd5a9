"""The model of tests/signcrypt_cases.py against the oracle (oracle/py/blsful_ref.py signcrypt_valid, signcrypt_verify_share;
reference src/traits/sign_crypt.rs:69-77,192-207): the validity verdict of EVERY distinct ciphertext of the list, and the share
verdicts of one share of every kind (honest, of another index, identity share, identity key share, under an identity w, under a
tampered v, and an honest share of an Aug ciphertext under the Basic and the Aug DST).  The oracle's pairing work is bounded: at
most 40 pairing products in all, counted and asserted -- which is why the share verdicts are a selection: the list holds more
honest shares than that budget.  Every opened plaintext of an honest case equals the message."""
import pytest

import signcrypt_cases as sc
from util import ref

MAX_PRODUCTS = 40


class Counter:
    def __init__(self):
        self.n = 0
        self.saved = {}

    def __enter__(self):
        for C in sc.IMPLS.values():
            self.saved[C] = C.__dict__['pairing_is_identity']
            inner = C.pairing_is_identity

            def counted(pairs, inner=inner):
                self.n += 1
                return inner(pairs)
            C.pairing_is_identity = staticmethod(counted)
        return self

    def __exit__(self, *a):
        for C, f in self.saved.items():
            C.pairing_is_identity = f


def test_verdicts_are_the_oracles():
    with Counter() as cnt:
        seen = set()
        for sg in (1, 2):
            C = sc.IMPLS[sg]
            for cs in sc.cases(sg):
                key = (sg, cs.scheme, id(cs.u) if cs.u is not None else None, cs.v, id(cs.w) if cs.w is not None else None)
                if key in seen:
                    continue
                seen.add(key)
                got = ref.signcrypt_valid(C, cs.u, cs.v, cs.w, C.DST[cs.scheme])
                assert got == (cs.valid_status() == sc.OK), cs.name
                assert (cs.valid_status() == sc.SIG_IDENTITY) == (cs.w is None), cs.name
                assert (cs.valid_status() == sc.PK_IDENTITY) == (cs.w is not None and cs.u is None), cs.name
        assert len(seen) >= 30
        picked = 0
        for sg in (1, 2):
            C = sc.IMPLS[sg]
            by = {cs.name: cs for cs in sc.cases(sg)}
            mixed, base = by['identity share, identity key share, other index'], by['basic, 3 of 2-of-3']
            sel = [(mixed, sh, None) for sh in mixed.shares] + [(by['identity w'], base.shares[0], None), (by['tampered v'], base.shares[0], None)]
            if sg == 2:
                aug = by['aug, 2 of 2-of-3']
                sel += [(aug, aug.shares[0], ref.BASIC), (aug, aug.shares[0], ref.AUG)]
            for cs, (_, a, b), scheme in sel:
                dst = C.DST[cs.scheme if scheme is None else scheme]
                got = ref.signcrypt_verify_share(C, sc.pk_point(sg, a), sc.pk_point(sg, b), cs.u, cs.v, cs.w, dst)
                assert got == (cs.share_status(a, b, scheme) == sc.OK), (cs.name, scheme)
                picked += 1
        assert picked >= 14
    assert 0 < cnt.n <= MAX_PRODUCTS, cnt.n


def test_honest_cases_open_to_their_message():
    n = 0
    for sg in (1, 2):
        for cs in sc.cases(sg):
            if cs.message is None:
                continue
            assert cs.open_with_shares() == (sc.OK, cs.message), cs.name
            assert cs.open_with_key() == (sc.OK, cs.message), cs.name
            assert all(st == sc.OK for st in cs.share_statuses()), cs.name
            n += 1
    assert n >= 2 * 5 + len(sc.LENGTHS)


def test_kinds_present():
    """Every status of the two calls occurs in the list, for each impl; both message-length and crafted cases are all there."""
    names = set()
    for sg in (1, 2):
        cl = sc.cases(sg)
        opened = {cs.open_with_shares()[0] for cs in cl} | {cs.open_with_key()[0] for cs in cl}
        assert {sc.OK, sc.VSSS_ERROR, sc.INVALID_SIGNATURE, sc.SIG_IDENTITY, sc.PK_IDENTITY} <= opened, sg
        shares = {st for cs in cl for st in cs.share_statuses()}
        assert shares == {sc.OK, sc.INVALID_DECRYPTION_SHARE}
        assert {cs.scheme for cs in cl} == {ref.BASIC, ref.AUG, ref.POP}
        assert {len(cs.shares) for cs in cl} >= {0, 1, 2, 3, 17}
        names |= {cs.name for cs in cl}
    both = sc.cases(1) + sc.cases(2)
    assert sc.BAD_FRAME in {cs.open_with_shares()[0] for cs in both} and sc.BAD_FRAME in {cs.open_with_key()[0] for cs in both}
    assert all('message of %d bytes' % n in names for n in sc.LENGTHS)
    assert all('crafted frame: ' + n in names for n, _ in sc.crafted_frames())
    # rejected identifier sets run on as the identity key, and a wrong key may still parse: the model decides, never an error
    for sg in (1, 2):
        by = {cs.name: cs for cs in sc.cases(sg)}
        for n in ('duplicate identifier', 'zero identifier', 'identifier >= r', 'identifier 2^256 - 1'):
            assert sc.combined_scalar([(i, a) for i, a, _ in by[n].shares]) == 0
            assert by[n].open_with_shares()[0] in (sc.OK, sc.BAD_FRAME)
    # the two-byte varint starts at 128
    assert len(sc.varint(127)) == 1 and len(sc.varint(128)) == 2 and sc.parse_frame(sc.frame_of(bytes(128))) == (2, 128)
    assert len(sc.frame_of(b'')) == 32 and len(sc.frame_of(bytes(31))) == 32 and len(sc.frame_of(bytes(32))) == 33
