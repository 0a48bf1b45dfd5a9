"""ElGamal over the public-key group, restated over the oracle (util.c, util.ref) from the reference crate:

    BlsElGamal::message_generator / seal_scalar_with_proof / verify_proof     src/traits/elgamal.rs:20-23,79-136,177-226
    ElGamalDecryptionKey::from_shares / decrypt                                src/elgamal_decryption_share.rs:76-90
    ElGamalCiphertext + ElGamalCiphertext                                      src/elgamal_ciphertext.rs:74-83

and the case list per impl that the CPU test (tests/test_elgamal_cases.py) and the GPU test (tests/test_gpu_elgamal.py) share.
The transcript is tests/merlin_ref.py.  `scalar_from_bytes_wide` is Scalar::from_bytes_wide of the back-end crates: the 64 bytes
as ONE little-endian integer, reduced modulo r.  That is their documented behaviour; their sources are not available here, and a
proof this module makes verifies under either byte order, so the byte order is taken from the documentation alone.

seal_scalar_with_proof here takes the blinder b and the nonce r as arguments and has no debug assertions: it only builds inputs
(the r = 0 and b = 0 proofs among them)."""
import random

import merlin_ref
import util
from util import c, ref

R = c.R
SALT = b'ELGAMAL_BLS12381_XOF:HKDF-SHA2-256_'
# the tag names the OTHER group than the one it hashes into (src/impls/g1.rs:129, g2.rs:127); kept as the reference has it
ENC_DST = {1: b'BLS_ELGAMAL_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_', 2: b'BLS_ELGAMAL_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_'}

OK, BAD_ENCODING, VSSS_ERROR, IDENTITY, ZERO_PROOF, CHALLENGE_MISMATCH = 0, 7, 13, 16, 17, 18
DEFAULT = 'default generator'      # Case.generator: the trait's None (a point, or None for the identity, is Some(point))
ERRORS = {IDENTITY: 'Parameters or ciphertext values are identity point', ZERO_PROOF: 'Proof values are zero',
          CHALLENGE_MISMATCH: 'Challenge values do not match'}


class KeyGroup:
    """The public-key group of an impl (sig_group 1: G2, 2: G1)."""

    def __init__(self, sg):
        self.sg, self.group = sg, 3 - sg
        self.C = ref.G1Impl if sg == 1 else ref.G2Impl
        self.E, self.gen, self.to_bytes = self.C.pk_curve, self.C.pk_gen, self.C.pk_to_bytes
        self.hash = c.hash_to_g2 if sg == 1 else c.hash_to_g1
        self.raw = util.g2_raw if sg == 1 else util.g1_raw
        self.aff_raw = util.g2_aff_raw if sg == 1 else util.g1_aff_raw
        self.K = 96 if sg == 1 else 48
        self._h = None

    def message_generator(self):
        if self._h is None:
            self._h = self.hash(self.to_bytes(self.gen), ENC_DST[self.sg])
        return self._h

    def mul(self, p, k):
        return self.E.mul(p, k % R)

    def add(self, a, b):
        return self.E.add(a, b)

    def sub(self, a, b):
        return self.E.add(a, self.E.neg(b))


_KG = {}


def kg(sg):
    if sg not in _KG:
        _KG[sg] = KeyGroup(sg)
    return _KG[sg]


def scalar_from_bytes_wide(b):
    assert len(b) == 64
    return int.from_bytes(b, 'little') % R


def challenge(g, pk, generator, c1, c2, r1, r2):
    t = merlin_ref.Transcript(b'ElGamalProof')
    t.append_message(b'dst', SALT)
    t.append_message(b'base point', g.to_bytes(g.gen))
    for label, p in ((b'pk', pk), (b'generator', generator), (b'c1', c1), (b'c2', c2), (b'r1', r1), (b'r2', r2)):
        t.append_message(label, g.to_bytes(p))
    return scalar_from_bytes_wide(t.challenge_bytes(b'challenge', 64))


def seal_scalar(g, pk, message, generator, blinder):
    return g.mul(g.gen, blinder), g.add(g.mul(pk, blinder), g.mul(generator, message))


def seal_scalar_with_proof(g, pk, message, generator, b, r):
    generator = g.message_generator() if generator is DEFAULT else generator
    c1, c2 = seal_scalar(g, pk, message, generator, b)
    r1, r2 = seal_scalar(g, pk, b, generator, r)
    ch = challenge(g, pk, generator, c1, c2, r1, r2)
    return c1, c2, (b + ch * message) % R, (r + ch * b) % R, ch


def verify_proof(g, pk, generator, c1, c2, mp, bp, ch):
    """The status of BlsElGamal::verify_proof.  A scalar >= r cannot be a reference Scalar: deserialisation fails first."""
    if mp >= R or bp >= R or ch >= R:
        return BAD_ENCODING
    generator = g.message_generator() if generator is DEFAULT else generator
    if pk is None or generator is None or c1 is None or c2 is None:
        return IDENTITY
    if mp == 0 or bp == 0 or ch == 0:
        return ZERO_PROOF
    neg = -ch % R
    r1 = g.add(g.mul(c1, neg), g.mul(g.gen, bp))
    r2 = g.add(g.add(g.mul(c2, neg), g.mul(generator, mp)), g.mul(pk, bp))
    return OK if challenge(g, pk, generator, c1, c2, r1, r2) == ch else CHALLENGE_MISMATCH


def lagrange0(xs):
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num, den = num * xj % R, den * (xj - xi) % R
        out.append(num * pow(den, R - 2, R) % R)
    return out


def from_shares(g, shares):
    """ElGamalDecryptionKey::from_shares over (identifier, point): (status, key point)."""
    xs = [i for i, _ in shares]
    if any(x >= R for x in xs):
        return BAD_ENCODING, None
    if len(xs) < 2 or 0 in xs or len(set(xs)) != len(xs):
        return VSSS_ERROR, None
    key = None
    for lam, (_, p) in zip(lagrange0(xs), shares):
        key = g.add(key, g.mul(p, lam))
    return OK, key


def decrypt(g, key, c2):
    return g.sub(c2, key)


class Case:
    def __init__(self, name, pk, generator, c1, c2, mp, bp, ch):
        self.name, self.pk, self.generator, self.c1, self.c2, self.mp, self.bp, self.ch = name, pk, generator, c1, c2, mp, bp, ch
        self.expect = None       # set by cases(): the model's verdict, computed once

    def with_(self, name, **kw):
        d = dict(pk=self.pk, generator=self.generator, c1=self.c1, c2=self.c2, mp=self.mp, bp=self.bp, ch=self.ch)
        d.update(kw)
        return Case(name, **d)


_CASES = {}


def cases(sg):
    """The case list of one impl: Case objects with .expect filled in by verify_proof (computed once per process)."""
    if sg in _CASES:
        return _CASES[sg]
    g = kg(sg)
    rng = random.Random(100 + sg)
    G, H = g.gen, g.message_generator()
    sk = rng.randrange(1, R)
    pk = g.mul(G, sk)
    m, b, r = rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, R)
    honest = Case('honest', pk, DEFAULT, *seal_scalar_with_proof(g, pk, m, DEFAULT, b, r))
    out = [honest]
    # tampering
    for f in ('mp', 'bp', 'ch'):
        out.append(honest.with_('tampered ' + f, **{f: (getattr(honest, f) + 1) % R}))
    other = g.mul(G, rng.randrange(1, R))
    for f in ('c1', 'c2'):
        out.append(honest.with_('tampered ' + f, **{f: g.add(getattr(honest, f), G)}))
    out.append(honest.with_('wrong pk', pk=other))
    out.append(honest.with_('wrong generator', generator=other))
    # a custom generator
    gen2 = g.mul(G, rng.randrange(1, R))
    custom = Case('custom generator', pk, gen2, *seal_scalar_with_proof(g, pk, m, gen2, b, r))
    out.append(custom)
    out.append(custom.with_('custom generator, default given', generator=DEFAULT))
    out.append(honest.with_('default generator given explicitly', generator=H))
    # identities, alone and with a zero scalar (the identity check comes first)
    for f in ('pk', 'generator', 'c1', 'c2'):
        out.append(honest.with_(f + ' identity', **{f: None}))
        out.append(honest.with_(f + ' identity, zero mp', **{f: None, 'mp': 0}))
        out.append(honest.with_(f + ' identity, zero ch', **{f: None, 'ch': 0}))
    out.append(Case('all identity', None, None, None, None, honest.mp, honest.bp, honest.ch))
    # zero scalars, scalars that are no Scalar
    for f in ('mp', 'bp', 'ch'):
        out.append(honest.with_(f + ' zero', **{f: 0}))
        out.append(honest.with_(f + ' = r', **{f: R}))
        out.append(honest.with_(f + ' = 2^256 - 1', **{f: 2 ** 256 - 1}))
    out.append(honest.with_('mp = r with c1 identity (deserialisation first)', mp=R, c1=None))
    # extreme challenges and unit proofs: the verdict is a mismatch, r1 and r2 must still be computed right
    out.append(honest.with_('ch = 1', ch=1))
    out.append(honest.with_('ch = r - 1', ch=R - 1))
    out.append(honest.with_('bp = mp = 1', bp=1, mp=1))
    out.append(honest.with_('bp = mp = ch = 1', bp=1, mp=1, ch=1))
    # related bases: the accumulator of the joint ladder meets P + P, P - P and the identity
    k = rng.randrange(1, R)
    out.append(honest.with_('c1 = G, -ch = bp', c1=G, ch=k, bp=-k % R))
    out.append(honest.with_('c1 = G, ch = bp', c1=G, ch=k, bp=k))                 # r1 = identity
    out.append(honest.with_('c1 = -G', c1=g.E.neg(G)))
    out.append(honest.with_('c1 = -G, ch = bp', c1=g.E.neg(G), ch=k, bp=k))
    out.append(honest.with_('c1 = -G, -ch = bp', c1=g.E.neg(G), ch=k, bp=-k % R))    # r1 = identity
    out.append(honest.with_('pk = H', pk=H))
    out.append(honest.with_('pk = H, mp = -bp', pk=H, mp=-honest.bp % R))
    out.append(honest.with_('pk = H, mp = bp', pk=H, mp=honest.bp))
    out.append(honest.with_('c2 = H', c2=H))
    out.append(honest.with_('c2 = H, mp = ch', c2=H, mp=honest.ch))
    out.append(honest.with_('c2 = H, mp = -ch', c2=H, mp=-honest.ch % R))
    out.append(honest.with_('pk = G', pk=G))
    out.append(honest.with_('pk = G = c2 = c1, bp = ch', pk=G, c1=G, c2=G, bp=honest.ch))
    out.append(Case('honest with pk = G', G, DEFAULT, *seal_scalar_with_proof(g, G, m, DEFAULT, b, r)))
    out.append(Case('honest with pk = H', H, DEFAULT, *seal_scalar_with_proof(g, H, m, DEFAULT, b, r)))
    out.append(Case('honest with generator = G', pk, G, *seal_scalar_with_proof(g, pk, m, G, b, r)))
    out.append(Case('honest with m = 0', pk, DEFAULT, *seal_scalar_with_proof(g, pk, 0, DEFAULT, b, r)))
    # r = 0: valid, r1 = r2 = identity; b = 0: c1 = identity
    out.append(Case('r = 0', pk, DEFAULT, *seal_scalar_with_proof(g, pk, m, DEFAULT, b, 0)))
    out.append(Case('r = 0, custom generator', pk, gen2, *seal_scalar_with_proof(g, pk, m, gen2, b, 0)))
    out.append(Case('b = 0', pk, DEFAULT, *seal_scalar_with_proof(g, pk, m, DEFAULT, 0, r)))
    for cs in out:
        cs.expect = verify_proof(g, cs.pk, cs.generator, cs.c1, cs.c2, cs.mp, cs.bp, cs.ch)
    _CASES[sg] = out
    return out


def arrays(sg, cl, rng=None, explicit_generators=True, shared_pk=None):
    """The flat arguments of the proof check for a list of cases: (pks, generators or None, c1s, c2s, mps, bps, chs) as lists of
    raw points (random Z with rng) and ints.  explicit_generators=False needs every case to use the default generator."""
    g = kg(sg)
    pks = [g.raw(cs.pk, rng) for cs in cl] if shared_pk is None else [g.raw(shared_pk, rng)]
    gens = None
    if explicit_generators:
        H = g.message_generator()
        gens = [g.raw(H if cs.generator is DEFAULT else cs.generator, rng) for cs in cl]
    else:
        assert all(cs.generator is DEFAULT for cs in cl)
    return (pks, gens, [g.raw(cs.c1, rng) for cs in cl], [g.raw(cs.c2, rng) for cs in cl], [cs.mp for cs in cl], [cs.bp for cs in cl],
            [cs.ch for cs in cl])
