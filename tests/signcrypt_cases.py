"""The case list of the threshold signcryption calls (blsgpu_signcrypt_share_verify_batch, blsgpu_signcrypt_open_batch), shared by
tests/test_signcrypt_cases.py (CPU: the expected verdicts are the oracle's), tests/test_hostsim_signcrypt.py (the frame parser) and
tests/test_gpu_signcrypt.py (GPU: the batched calls return them).

Everything is built from public scalars: u = r g, a key share sk_i g, a decryption share (sk_i r) g, w = rho H(U || V).  The model
below restates include/blsgpu.h -- the share rule, Lagrange at zero over the share SCALARS (a rejected identifier set gives the
identity), SHAKE128(G.to_bytes()) xor v, the varint prefix -- and decides validity and share verdicts algebraically (w = rho H(m) is
valid for u = r g iff m is the hashed message and rho = r), without a pairing; tests/test_signcrypt_cases.py holds that against the
oracle's pairings."""
import functools
import hashlib

from util import c, ref

OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
VSSS_ERROR, INVALID_DECRYPTION_SHARE, BAD_FRAME = 13, 14, 15
R = c.R
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}
VARINT_MAX = 19


# ------------------------------------------------------------------ the model
def varint(n):
    """uint-zigzag's unsigned encoding: seven bits per byte, least significant group first, top bit on every byte but the last."""
    out = bytearray()
    while True:
        b = n & 0x7f
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def parse_frame(frame):
    """(overhead, len) of varint(len) || message || padding, or None (reference src/traits/sign_crypt.rs:122-136)."""
    value = 0
    for i in range(VARINT_MAX):
        if i >= len(frame):
            return None
        value |= (frame[i] & 0x7f) << (7 * i)
        if not frame[i] & 0x80:
            value %= 2 ** 64
            return (i + 1, value) if value <= len(frame) - (i + 1) else None
    return None


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def keystream(C, G, n):
    return hashlib.shake_128(C.pk_to_bytes(G)).digest(n) if n else b''


@functools.lru_cache(maxsize=None)
def pk_point(sg, k):
    """k g in the public-key group of the impl (None for k = 0 mod r)."""
    C = IMPLS[sg]
    return C.pk_curve.mul(C.pk_gen, k % R) if k % R else None


def combined_scalar(shares):
    """sum lambda_i a_i mod r over (identifier, a_i); 0 -- the identity -- for a set the recovery rejects (a zero or duplicate
    identifier, an identifier >= r): combine().unwrap_or_default()."""
    ids = [i for i, _ in shares]
    if any(i == 0 or i >= R for i in ids) or len(set(ids)) != len(ids):
        return 0
    tot = 0
    for i, (xi, a) in enumerate(shares):
        num = den = 1
        for j, (xj, _) in enumerate(shares):
            if j != i:
                num = num * xj % R
                den = den * (xj - xi) % R
        tot = (tot + a * num * pow(den, R - 2, R)) % R
    return tot


class Case:
    """One ciphertext and what is done with it.  u = r g (None: the identity); w = rho H_scheme(w_msg) (None: the identity);
    shares: [(identifier, a, b)], decryption share a g and public-key share b g; key: G = key g for the decrypt form."""

    def __init__(self, sg, name, scheme, r, v, rho, w_msg, shares, key, message=None, u_identity=False, w_identity=False):
        C = IMPLS[sg]
        self.sg, self.name, self.scheme, self.r, self.v, self.rho, self.w_msg = sg, name, scheme, r, bytes(v), rho, w_msg
        self.shares, self.key, self.message = list(shares), key, message
        self.u = None if u_identity else pk_point(sg, r)
        self.w = None if w_identity else C.sig_curve.mul(C.hash_to_point(w_msg, C.DST[scheme]), rho % R)

    @property
    def C(self):
        return IMPLS[self.sg]

    def hashed(self):
        return self.C.pk_to_bytes(self.u) + self.v

    def valid_status(self):
        if self.w is None:
            return SIG_IDENTITY
        if self.u is None:
            return PK_IDENTITY
        return OK if self.w_msg == self.hashed() and self.rho % R == self.r % R else INVALID_SIGNATURE

    def share_status(self, a, b, scheme=None):
        """BlsSignCrypt::verify_share under the DST of `scheme` (default: the ciphertext's own)."""
        scheme = self.scheme if scheme is None else scheme
        ok = a % R and b % R and self.w is not None and scheme == self.scheme and self.w_msg == self.hashed() and (a - self.rho * b) % R == 0
        return OK if ok else INVALID_DECRYPTION_SHARE

    def share_statuses(self):
        return [self.share_status(a, b) for _, a, b in self.shares]

    def _open(self, G):
        frame = xor(keystream(self.C, G, len(self.v)), self.v)
        st = self.valid_status()
        if st != OK:
            return st, None
        p = parse_frame(frame)
        if p is None:
            return BAD_FRAME, None
        return OK, frame[p[0]:p[0] + p[1]]

    def open_with_shares(self):
        if len(self.shares) < 2:
            return VSSS_ERROR, None
        return self._open(pk_point(self.sg, combined_scalar([(i, a) for i, a, _ in self.shares])))

    def open_with_key(self):
        return self._open(pk_point(self.sg, self.key))


def frame_of(msg):
    f = varint(len(msg)) + msg
    return f + bytes(max(0, 32 - len(f)))


def poly_eval(coeffs, x):
    v = 0
    for a in reversed(coeffs):
        v = (v * x + a) % R
    return v


def _scalar(tag, n=0):
    return int.from_bytes(hashlib.sha256(b'signcrypt case %s %d' % (tag, n)).digest() * 2, 'big') % (R - 1) + 1


def sealed(sg, name, scheme, msg, coeffs, ids, frame=None, **kw):
    """seal (reference src/traits/sign_crypt.rs:34-61) under the key coeffs[0] g with r derived from the name, and the shares of
    the identifiers `ids` of the polynomial `coeffs`.  frame: the bytes encrypted in place of varint || msg || padding."""
    C = IMPLS[sg]
    r = _scalar(name.encode(), sg)
    sk = coeffs[0]
    frame = frame_of(msg) if frame is None else frame
    v = xor(keystream(C, pk_point(sg, sk * r), len(frame)), frame)
    w_msg = C.pk_to_bytes(pk_point(sg, r)) + v
    shares = [(i, poly_eval(coeffs, i) * r % R, poly_eval(coeffs, i)) for i in ids]
    return Case(sg, name, scheme, r, v, r, w_msg, shares, sk * r % R, message=msg if frame == frame_of(msg) else None, **kw)


def variant(cs, name, **kw):
    """The same ciphertext (same u, v, w objects unless changed) with other shares / key / fields."""
    n = Case.__new__(Case)
    n.__dict__.update(cs.__dict__)
    n.name = name
    n.message = kw.pop('message', None)
    n.__dict__.update(kw)
    return n


LENGTHS = [0, 1, 30, 31, 32, 126, 127, 128, 165, 166, 167, 168, 334, 335, 336]


@functools.lru_cache(maxsize=None)
def cases(sg):
    """The list for one impl.  The message-length and crafted-frame cases alternate between the impls (the keystream and the parser
    do not depend on the group beyond the 48 / 96 key bytes), which keeps the oracle's pairing work of the CPU test bounded."""
    out = []
    p23 = [_scalar(b'p23', sg), _scalar(b'p23b', sg)]                       # 2-of-3
    other = [_scalar(b'other', sg), _scalar(b'otherb', sg)]
    p917 = [_scalar(b'p917', k + 100 * sg) for k in range(9)]               # 9-of-17
    ids17 = [_scalar(b'id17', k) for k in range(17)]
    msg = b'thirty bytes of plaintext....!'
    base = sealed(sg, 'basic, 3 of 2-of-3', ref.BASIC, msg, p23, [1, 2, 3])
    out.append(base)
    out.append(sealed(sg, 'aug, 2 of 2-of-3', ref.AUG, msg + b' aug', p23, [3, 1]))
    out.append(sealed(sg, 'pop, 2 of 2-of-3', ref.POP, msg + b' pop', p23, [2, 3]))
    out.append(variant(base, '0 shares', shares=[]))
    out.append(variant(base, '1 share', shares=base.shares[:1]))
    out.append(variant(base, '2 shares', shares=base.shares[1:], message=msg))
    out.append(sealed(sg, '17 of 9-of-17', ref.BASIC, msg * 3, p917, ids17))
    s = base.shares
    out.append(variant(base, 'duplicate identifier', shares=[s[0], (s[0][0], s[1][1], s[1][2]), s[2]]))
    out.append(variant(base, 'zero identifier', shares=[s[0], (0, s[1][1], s[1][2])]))
    out.append(variant(base, 'identifier >= r', shares=[s[0], (R + 2, s[1][1], s[1][2])]))
    out.append(variant(base, 'identifier 2^256 - 1', shares=[(2 ** 256 - 1, s[0][1], s[0][2]), s[1]]))
    out.append(variant(base, 'shares of another key', shares=[(i, poly_eval(other, i) * base.r % R, poly_eval(other, i)) for i in (1, 2)],
                       key=other[0] * base.r % R))
    out.append(variant(base, 'one good share and one of another key', shares=[s[0], (2, poly_eval(other, 2) * base.r % R, poly_eval(other, 2))]))
    tv = bytearray(base.v)
    tv[5] ^= 0x40
    out.append(variant(base, 'tampered v', v=bytes(tv)))
    out.append(variant(base, 'identity u', u=None))
    out.append(variant(base, 'identity w', w=None))
    out.append(variant(base, 'identity share, identity key share, other index',
                       shares=[(1, 0, s[0][2]), (2, s[1][1], 0), (3, s[0][1], s[2][2]), s[2]]))
    for k, n in enumerate(LENGTHS):
        if k % 2 == sg % 2:
            m = bytes((7 * j + n) & 0xff for j in range(n))
            out.append(sealed(sg, 'message of %d bytes' % n, ref.BASIC, m, p23, [1, 3]))
    for k, (name, frame) in enumerate(crafted_frames()):
        if k % 2 == sg % 2:
            out.append(sealed(sg, 'crafted frame: ' + name, ref.BASIC, b'', p23, [2, 1], frame=frame))
    return out


def crafted_frames():
    return [('empty v', b''),
            ('10 continuation bytes', bytes([0x80, 0xff, 0x81, 0x80, 0x92, 0xa5, 0x80, 0x80, 0xc0, 0xfe])),
            ('declared length one more than remains', varint(40) + bytes(range(39))),
            ('declared length exactly what remains', varint(40) + bytes(range(40))),
            ('two-byte prefix, exactly what remains', varint(200) + bytes(200)),
            ('nine-byte prefix', varint(2 ** 63 - 1) + bytes(30))]


# ------------------------------------------------------------------ raw inputs of the library calls
def raw_pk(sg, pt, rng=None):
    import util
    return (util.g2_raw if sg == 1 else util.g1_raw)(pt, rng) if pt is not None else (util.g2_raw if sg == 1 else util.g1_raw)(None)


def raw_sig(sg, pt, rng=None):
    import util
    return (util.g1_raw if sg == 1 else util.g2_raw)(pt, rng) if pt is not None else (util.g1_raw if sg == 1 else util.g2_raw)(None)


def raw_ct(cs, rng=None):
    return raw_pk(cs.sg, cs.u, rng), cs.v, raw_sig(cs.sg, cs.w, rng)
