"""The case list of blsgpu_signcrypt_share_verify_indexed_batch: the ciphertexts and shares of tests/signcrypt_cases.py with every
public-key share named by its POSITION in a committee table of eight entries, shared by tests/test_signcrypt_indexed_cases.py (CPU:
the classes are all there, a handful of the expected statuses are the oracle's pairings) and tests/test_gpu_signcrypt_indexed.py (GPU:
the call returns them).

The table is created from wire bytes (FMT_COMPRESSED), so that one entry can fail decoding:
    0, 1, 2   the key shares of the 2-of-3 polynomial at the identifiers 1, 2, 3
    3, 4      the key shares of another polynomial at 1, 2
    5         the identity (a valid entry)
    6         x >= p: deserialization fails, the entry's creation status is BAD_ENCODING
    7         the key share of the 9-of-17 polynomial at its first identifier
The expected status of a share (position, a) of a ciphertext, the first that applies: E_ARG for a position outside the table; the
entry's creation status for the invalid entry; otherwise Case.share_status(a, b) with b the entry's scalar, under the DST of the CALL's
scheme -- what the by-value call gives with the gathered key."""
import functools

import signcrypt_cases as sc
from util import ref

OK, INVALID_DECRYPTION_SHARE = sc.OK, sc.INVALID_DECRYPTION_SHARE
E_ARG, BAD_ENCODING = -3, 7
R = sc.R
N = 8
P23_1, P23_2, P23_3, OTHER_1, OTHER_2, IDENT, BAD, P917_0 = range(N)
CLASSES = ('valid', 'tampered share', 'wrong member', 'identity share', 'identity entry', 'invalid entry', 'past the end', 'identity w',
           'wrong-scheme DST', '0 shares', 'repeated position', 'empty v')


@functools.lru_cache(maxsize=None)
def table(sg):
    """dict(ks, blobs, status): ks[i] is entry i's scalar (0: the identity, None: the invalid entry), blobs the compressed bytes the
    set is created from, status the creation statuses the library must report"""
    C = sc.IMPLS[sg]
    p23 = [sc._scalar(b'p23', sg), sc._scalar(b'p23b', sg)]
    other = [sc._scalar(b'other', sg), sc._scalar(b'otherb', sg)]
    p917 = [sc._scalar(b'p917', k + 100 * sg) for k in range(9)]
    ks = [sc.poly_eval(p23, 1), sc.poly_eval(p23, 2), sc.poly_eval(p23, 3), sc.poly_eval(other, 1), sc.poly_eval(other, 2), 0, None,
          sc.poly_eval(p917, sc._scalar(b'id17', 0))]
    blobs = [C.pk_to_bytes(sc.pk_point(sg, k)) if k is not None else None for k in ks]
    w = len(blobs[0])
    blobs[BAD] = bytes([blobs[0][0] & 0x9f | 0x1f]) + b'\xff' * (w - 1)          # x >= p
    assert blobs[IDENT] == b'\xc0' + bytes(w - 1)
    return dict(ks=ks, blobs=blobs, status=[BAD_ENCODING if k is None else OK for k in ks])


class ICase:
    """One ciphertext of the indexed call: cs (a signcrypt_cases.Case), the scheme the CALL passes, shares [(position, a)] and the
    classes the case stands for"""

    def __init__(self, cs, shares, classes, call_scheme=None, name=None):
        self.cs, self.shares, self.classes = cs, list(shares), tuple(classes)
        self.call_scheme = cs.scheme if call_scheme is None else call_scheme
        self.name = name or cs.name

    def expected(self):
        t = table(self.cs.sg)
        return [share_expected(self.cs, t, pos, a, self.call_scheme) for pos, a in self.shares]


def share_expected(cs, t, pos, a, scheme):
    if pos >= len(t['ks']):
        return E_ARG
    if t['status'][pos] != OK:
        return t['status'][pos]
    return cs.share_status(a, t['ks'][pos], scheme)


def by_position(cs, t):
    """the case's (identifier, a, b) shares as (position, a), or None when some b is not in the table"""
    out = []
    for _, a, b in cs.shares:
        if b % R not in [k for k in t['ks'] if k is not None]:
            return None
        out.append((t['ks'].index(b % R), a))
    return out


@functools.lru_cache(maxsize=None)
def cases(sg):
    t = table(sg)
    by = {cs.name: cs for cs in sc.cases(sg)}
    out = []
    tags = {'basic, 3 of 2-of-3': ('valid',), '0 shares': ('0 shares',), 'identity w': ('identity w',),
            'identity share, identity key share, other index': ('identity share', 'identity entry', 'wrong member'),
            'crafted frame: empty v': ('empty v', 'valid')}
    for cs in sc.cases(sg):                                   # every case of the list whose key shares are committee members
        pos = by_position(cs, t)
        if pos is not None:
            out.append(ICase(cs, pos, tags.get(cs.name, ())))
    base = by['basic, 3 of 2-of-3']
    s = by_position(base, t)
    big = by['17 of 9-of-17']
    out.append(ICase(big, [(P917_0, big.shares[0][1])], ('valid',), name='17 of 9-of-17: its first member'))
    out.append(ICase(base, [s[0], (s[1][0], (s[1][1] + 1) % R), s[2]], ('tampered share',), name='tampered share'))
    out.append(ICase(base, [(s[1][0], s[0][1]), (s[0][0], s[1][1]), s[2]], ('wrong member',), name='right shares, two positions swapped'))
    out.append(ICase(base, [(IDENT, s[0][1]), s[1]], ('identity entry',), name='a share under the identity entry'))
    out.append(ICase(base, [s[0], (BAD, s[1][1]), (BAD, 0)], ('invalid entry',), name='shares under the invalid entry'))
    out.append(ICase(base, [(N, s[0][1]), s[1], (2 ** 32 - 1, s[2][1]), (N, 0)], ('past the end',), name='positions past the end'))
    out.append(ICase(base, [s[0], s[0], s[1], s[0]], ('repeated position',), name='a repeated position'))
    aug = by['aug, 2 of 2-of-3']
    out.append(ICase(aug, by_position(aug, t), ('wrong-scheme DST',), call_scheme=ref.BASIC, name='an Aug ciphertext under the Basic DST'))
    out.append(ICase(base, s, ('wrong-scheme DST',), call_scheme=ref.POP, name='a Basic ciphertext under the PoP DST'))
    if 'crafted frame: empty v' not in by:                    # the list alternates its crafted frames between the impls
        p23 = [sc._scalar(b'p23', sg), sc._scalar(b'p23b', sg)]
        ev = sc.sealed(sg, 'indexed: empty v', ref.BASIC, b'', p23, [2, 1], frame=b'')
        out.append(ICase(ev, by_position(ev, t), ('empty v', 'valid')))
    iw = by['identity w']
    out.append(ICase(iw, [(BAD, iw.shares[0][1]), (N, iw.shares[1][1]), by_position(iw, t)[2]], ('identity w', 'invalid entry', 'past the end'),
                     name='identity w under bad positions'))
    return out


def by_call_scheme(sg):
    out = {}
    for ic in cases(sg):
        out.setdefault(ic.call_scheme, []).append(ic)
    return out


# ------------------------------------------------------------------ raw inputs of the library calls
def raw_shares(ic, rng=None):
    return [(pos, sc.raw_pk(ic.cs.sg, sc.pk_point(ic.cs.sg, a), rng)) for pos, a in ic.shares]


def gathered(ic, rng=None):
    """the by-value call's (share, key share) pairs for the shares whose position names a valid entry (else None)"""
    t = table(ic.cs.sg)
    return [(sc.raw_pk(ic.cs.sg, sc.pk_point(ic.cs.sg, a), rng), sc.raw_pk(ic.cs.sg, sc.pk_point(ic.cs.sg, t['ks'][pos]), rng))
            if pos < N and t['ks'][pos] is not None else None for pos, a in ic.shares]
