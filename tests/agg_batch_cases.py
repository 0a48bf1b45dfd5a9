"""The case list of the batched aggregate verify (blsgpu_aggregate_verify_batch), shared by tests/test_agg_batch_cases.py (CPU:
every expected entry is what the oracle's aggregate_verify raises) and tests/test_gpu_agg_batch.py / tests/agg_batch_worker.py
(GPU: the batched call returns them).  Points are oracle points (None = identity); signatures are made here from the secret
keys, sum_i sk_i H(m_i), not by the library."""
import functools

import util
from util import ref

OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY, DUPLICATE_MESSAGE = 0, 1, 2, 3, 4
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}
N_KEYS = 5
ORACLE_MAX_PAIRS = 8              # larger sets are expected-by-construction only: the pure-Python pairing is left out of the CPU suite

_keys = {}


def keys(C):
    if C.name not in _keys:
        sks = [ref.keygen_from_hash(bytes([0x40 + j]) * 32) for j in range(N_KEYS)]
        _keys[C.name] = (sks, [ref.public_key(C, sk) for sk in sks])
    return _keys[C.name]


def aggregate(C, scheme, pairs):
    """The aggregate signature over pairs = [(key index, msg)]: sum_j sk_j (sum of H(m) over the key's messages)."""
    sks, pks = keys(C)
    by_key = {}
    for j, m in pairs:
        full = C.pk_to_bytes(pks[j]) + m if scheme == ref.AUG else m
        by_key[j] = C.sig_curve.add(by_key.get(j), C.hash_to_point(full, C.DST[scheme]))
    sig = None
    for j, h in by_key.items():
        sig = C.sig_curve.add(sig, C.sig_curve.mul(h, sks[j]))
    return sig


@functools.lru_cache(maxsize=None)
def cases(sg, scheme, big=True):
    """[(name, [(pk, msg)], sig, (status, (aux0, aux1)))] for one impl and scheme.  big=False leaves out the sets above
    ORACLE_MAX_PAIRS pairs (making their signatures takes the pure-Python oracle seconds)."""
    C = IMPLS[sg]
    _, pks = keys(C)
    basic = scheme == ref.BASIC
    out = []

    def add(name, signed, shown=None, sig='signed', expect=(OK, (0, 0))):
        """signed: the (key index, msg) pairs the signature covers; shown: what the verifier gets ((None, msg): an identity key)."""
        shown = signed if shown is None else shown
        s = aggregate(C, scheme, signed) if sig == 'signed' else sig
        out.append((name, [(pks[j] if j is not None else None, m) for j, m in shown], s, expect))

    bad = (INVALID_SIGNATURE, (0, 0))
    abc = [(0, b'case a'), (1, b'case b'), (2, b'case c')]
    add('valid', abc)
    add('wrong message', abc, [(0, b'case a'), (1, b'case B'), (2, b'case c')], expect=bad)
    add('a pair missing', abc + [(3, b'case d')], abc, expect=bad)
    add('a key swapped', abc, [(0, b'case a'), (4, b'case b'), (2, b'case c')], expect=bad)
    add('pairs permuted together', abc, [abc[2], abc[0], abc[1]])
    dup = [(0, b'x'), (1, b'same'), (2, b'y'), (3, b'same')]
    add('duplicate message in one set', dup, expect=(DUPLICATE_MESSAGE, (1, 3)) if basic else (OK, (0, 0)))
    add('same message as the next set', [(0, b'shared'), (1, b'p')])
    add('same message as the set before', [(2, b'q'), (3, b'shared')])
    add('empty set, non-identity signature', abc, [], expect=bad)
    add('empty set, identity signature', [], expect=(SIG_IDENTITY, (0, 0)))
    add('identity signature, pairs present', abc, sig=None, expect=(SIG_IDENTITY, (0, 0)))
    add('identity keys at two positions', [(0, b'i0'), (2, b'i2')], [(0, b'i0'), (None, b'i1'), (2, b'i2'), (None, b'i3')], expect=(PK_IDENTITY, (2, 0)))
    add('duplicate, identity key and identity signature', [], [(0, b'd'), (None, b'e'), (1, b'd')], sig=None,
        expect=(DUPLICATE_MESSAGE, (0, 2)) if basic else (SIG_IDENTITY, (0, 0)))
    add('a zero-length message', [(0, b'z'), (1, b''), (2, b'zz')])
    add('two zero-length messages', [(0, b''), (1, b'nz'), (2, b'')], expect=(DUPLICATE_MESSAGE, (0, 2)) if basic else (OK, (0, 0)))
    add('one message a prefix of another', [(0, b'abc'), (1, b'abcd'), (2, b'ab'), (3, b'\x00'), (4, b'\x00\x00')])
    for n in (1, 2, 3) + ((63, 64, 65) if big else ()):
        add('size %d' % n, [(i % N_KEYS, b'size %d item %d' % (n, i)) for i in range(n)])
    if big:
        add('size 64, last message changed', [(i % N_KEYS, b'size 64t item %d' % i) for i in range(64)],
            [(i % N_KEYS, b'size 64t item %d' % i if i < 63 else b'size 64t item 63!') for i in range(64)], expect=bad)
    return out


def raw_sets(sg, case_list, rng=None):
    """[(pks, msgs, sig)] as RAW_PROJ byte strings (random Z when rng is given), the input of api.aggregate_verify_batch."""
    pk_raw, sig_raw = (util.g2_raw, util.g1_raw) if sg == 1 else (util.g1_raw, util.g2_raw)
    return [([pk_raw(pk, rng) if pk is not None else pk_raw(None) for pk, _ in pairs], [m for _, m in pairs], sig_raw(sig, rng) if sig is not None else sig_raw(None))
            for _, pairs, sig, _ in case_list]
