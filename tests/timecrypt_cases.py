"""The case lists of the pairing-value call (blsgpu_pairing_batch) and of time-lock decryption (blsgpu_timecrypt_open_batch, second
half of this file), shared by tests/test_timecrypt_cases.py (CPU: what the lists claim for themselves),
tests/test_hostsim_timecrypt.py (the engine and tail functions on the host) and tests/test_gpu_pairing_value.py /
tests/test_gpu_timecrypt.py (the calls).  Every expected byte and status comes from tests/timecrypt_ref.py and the oracle.

A pair is (P in G1, Q in G2), built from public scalars: P = a g1, Q = b g2, so that e(P, Q) = e(g1, g2)^(a b) can be checked against
the list's own base value.  An item is a pair with its two rendered members, its expected 576 bytes and its expected status."""
import functools
import random

import util
from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref
import timecrypt_ref as tr

RAW_PROJ, RAW_AFFINE, COMPRESSED, LEGACY = 0, 1, 2, 3       # include/blsgpu.h
FMTS = (RAW_PROJ, RAW_AFFINE, COMPRESSED, LEGACY)
FMT_IDS = {RAW_PROJ: 'proj', RAW_AFFINE: 'affine', COMPRESSED: 'compressed', LEGACY: 'legacy'}
OK, BAD_ENCODING, LEGACY_FORMAT = 0, 7, 8
ZERO_GT = bytes(tr.GT_BYTES)

# the scalars (a, b) of the dozen distinct pairs: the generators, small and large multiples, r - 1 (the negated generators)
_rng = random.Random(20250)
SCALARS = [(1, 1), (5, 7), (c.R - 1, 1), (1, c.R - 1), (2, c.R - 2), (3, 3)] + \
          [(_rng.randrange(1, c.R), _rng.randrange(1, c.R)) for _ in range(6)]


@functools.lru_cache(maxsize=None)
def g1_mul(a):
    return c.E1.mul(c.G1_GEN, a % c.R) if a % c.R else None


@functools.lru_cache(maxsize=None)
def g2_mul(b):
    return c.E2.mul(c.G2_GEN, b % c.R) if b % c.R else None


@functools.lru_cache(maxsize=None)
def value(a, b):
    """the oracle's pairing value of (a g1, b g2)"""
    return tr.pairing_value(g1_mul(a), g2_mul(b))


def expected(a, b):
    return tr.gt_bytes(value(a, b))


def render_point(group, pt, fmt, rng):
    """one occurrence of a point in a caller format (RAW_PROJ: a fresh Jacobian Z; the identity: Z = 0 / all zero / the 0xc0 header)"""
    if fmt == RAW_PROJ:
        return util.g1_raw(pt, rng) if group == 1 else util.g2_raw(pt, rng)
    if fmt == RAW_AFFINE:
        if pt is None:
            return bytes(96 * group)
        return util.g1_aff_raw(pt) if group == 1 else util.g2_aff_raw(pt)
    b = c.g1_compress(pt) if group == 1 else c.g2_compress(pt)
    return ref.modern_to_legacy(b) if fmt == LEGACY else b


def decode_status(group, b, fmt):
    """the status of one wire point: OK, BAD_ENCODING (DeserializationError) or LEGACY_FORMAT (LegacyFormatError)"""
    try:
        if fmt == LEGACY:
            b = ref.legacy_to_modern(b)
        else:
            ref.validate_modern(b[0], 'G%d' % group)
        (c.g1_decompress if group == 1 else c.g2_decompress)(b)
        return OK
    except ref.BlsError as e:
        return {'LegacyFormatError': LEGACY_FORMAT, 'DeserializationError': BAD_ENCODING}[e.kind]
    except c.DecodeError:
        return BAD_ENCODING


def bad_wire(group, kind, fmt):
    """wire bytes that do not decode: 'flag' (no compression flag; under LEGACY a stray header bit), 'range' (x >= p), 'curve' (an x
    with no point)"""
    n = 48 * group
    if kind == 'flag':
        return bytes([0x60 if fmt == LEGACY else 0x00]) + bytes(n - 1)
    if kind == 'range':
        b = bytes([0x9f]) + bytes([0xff]) * (n - 1)
    else:
        x = 1
        while True:                                        # the first small x whose right-hand side is no square
            rhs = c.E1.rhs(x) if group == 1 else c.E2.rhs((x, 0))
            if (c.fp_sqrt(rhs) if group == 1 else c.f2_sqrt(rhs)) is None:
                break
            x += 1
        b = bytearray(n)
        b[n - 1] = x
        b[0] |= 0x80
        b = bytes(b)
    return ref.modern_to_legacy(b) if fmt == LEGACY else b


def items(fmt, n, seed=0):
    """n items in format fmt: the distinct pairs in turn, freshly rendered -> (g1s, g2s, want bytes, want statuses)"""
    rng = random.Random(1000 * fmt + seed)
    g1s, g2s, want = [], [], []
    for i in range(n):
        a, b = SCALARS[(i + seed) % len(SCALARS)]
        g1s.append(render_point(1, g1_mul(a), fmt, rng))
        g2s.append(render_point(2, g2_mul(b), fmt, rng))
        want.append(expected(a, b))
    return g1s, g2s, want, [OK] * n


def special_items(fmt):
    """an identity on either side and on both, between ordinary pairs; P and -P with one Q; on the wire formats the pairs that do not
    decode (either member, both: the G1 member's status comes first) -> (names, g1s, g2s, want bytes, want statuses)"""
    rng = random.Random(77 + fmt)
    a, b = SCALARS[1]
    rows = [('plain', g1_mul(a), g2_mul(b), expected(a, b)),
            ('identity G1', None, g2_mul(b), tr.GT_ONE),
            ('identity G2', g1_mul(a), None, tr.GT_ONE),
            ('identity both', None, None, tr.GT_ONE),
            ('P', g1_mul(a), g2_mul(b), expected(a, b)),
            ('-P', g1_mul(c.R - a), g2_mul(b), expected(c.R - a, b)),
            ('plain again', g1_mul(3), g2_mul(3), expected(3, 3))]
    names = [r[0] for r in rows]
    g1s = [render_point(1, r[1], fmt, rng) for r in rows]
    g2s = [render_point(2, r[2], fmt, rng) for r in rows]
    want = [r[3] for r in rows]
    st = [OK] * len(rows)
    if fmt in (COMPRESSED, LEGACY):
        good1, good2 = render_point(1, g1_mul(a), fmt, rng), render_point(2, g2_mul(b), fmt, rng)
        for kind in ('flag', 'range', 'curve'):
            for which in ('G1', 'G2', 'both'):
                x1 = bad_wire(1, kind, fmt) if which != 'G2' else good1
                x2 = bad_wire(2, kind, fmt) if which != 'G1' else good2
                s1, s2 = decode_status(1, x1, fmt), decode_status(2, x2, fmt)
                names.append('undecodable %s, %s' % (which, kind))
                g1s.append(x1)
                g2s.append(x2)
                want.append(ZERO_GT)
                st.append(s1 if s1 != OK else s2)
                assert st[-1] != OK
        names.append('plain last')
        g1s.append(good1)
        g2s.append(good2)
        want.append(expected(a, b))
        st.append(OK)
    return names, g1s, g2s, want, st


def pair_limbs(a, b):
    """the six reduced limb vectors (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1) of the pair, as the engine's workspace holds them"""
    p, q = g1_mul(a), g2_mul(b)
    return [util.limbs_of_elem(x) for x in (p[0], p[1], q[0][0], q[0][1], q[1][0], q[1][1])]


# ------------------------------------------------------------------ time-lock ciphertexts (blsgpu_timecrypt_open_batch)
# A group is {'sig': point or None, 'sig_bad': None or a bad_wire kind, 'scheme': tag, 'items': [...]}; an item is {'name', 'u': point
# or None, 'u_bad': None or a bad_wire kind, 'v', 'w', 'scheme', 'want': (status, message or None)}.  'want' is tr.unseal's answer under
# the group's signature; the *_bad members exist on the wire formats only, where they replace the point's bytes and the decode status
# comes first (expected_item).
INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY, INVALID_SCHEME, BAD_FRAME = 1, 2, 3, 12, 15
MESSAGE_LENGTHS = (0, 1, 30, 31, 32,               # the sealer's pad-to-32 rule
                   55, 56, 63, 64, 119, 120,       # SHA-256 padding of the message hash
                   126, 127, 128,                  # the varint grows to two bytes
                   165, 166, 167, 334, 335)        # frames of 167, 168, 169, 336, 337 bytes: the SHAKE128 rate
ROUND = {s: b'round %d' % (1000 + s) for s in (ref.BASIC, ref.AUG, ref.POP)}


def _sk(sg):
    return ref.keygen_from_hash(bytes([0x50 + sg]) * 32)


@functools.lru_cache(maxsize=None)
def round_sig(sg, scheme, ident, tweak=0):
    """the signature over an identifier as such, under the key (sk xor tweak)"""
    C = tr.IMPLS[sg]
    return C.sig_curve.mul(C.hash_to_point(ident, C.DST[scheme]), _sk(sg) ^ tweak)


def _message(n, salt):
    return bytes((salt + 31 * i) & 0xff for i in range(n))


def _alpha(k):
    return bytes((k * 17 + 3 * i + 1) & 0xff for i in range(32))


@functools.lru_cache(maxsize=None)
def timelock_groups(sg):
    """every case of one impl as the groups of ONE call: sizes 0, 1, 2, 5 first, empty groups between and at the end"""
    C = tr.IMPLS[sg]
    pk = ref.public_key(C, _sk(sg))

    def item(name, ct, sig, sig_scheme, u_bad=None):
        return {'name': name, 'u': ct[0], 'u_bad': u_bad, 'v': ct[1], 'w': ct[2], 'scheme': ct[3], 'want': tr.unseal(C, ct, sig, sig_scheme)}

    def group(scheme, items, sig='own', sig_bad=None):
        return {'sig': round_sig(sg, scheme, ROUND[scheme]) if sig == 'own' else sig, 'sig_bad': sig_bad, 'scheme': scheme, 'items': items}

    # ---- round trips at every length, scheme by scheme
    plain = []
    for k, n in enumerate(MESSAGE_LENGTHS):
        scheme = k % 3
        msg = _message(n, k + sg)
        ct = tr.seal(C, pk, msg, ROUND[scheme], scheme, _alpha(k))
        plain.append((scheme, item('message of %d bytes' % n, ct, round_sig(sg, scheme, ROUND[scheme]), scheme)))
        assert plain[-1][1]['want'] == (OK, msg) and len(ct[2]) == max(32, n + (1 if n < 128 else 2))
    by_scheme = {s: [it for sc, it in plain if sc == s] for s in (0, 1, 2)}
    groups = [group(0, []), group(0, by_scheme[0][:1]), group(1, by_scheme[1][:2]), group(2, by_scheme[2][:5]), group(1, []),
              group(0, by_scheme[0][1:]), group(1, by_scheme[1][2:]), group(2, by_scheme[2][5:])]

    # ---- crafted frames and failures, under the Basic round's signature
    S = ref.BASIC
    sig = round_sig(sg, S, ROUND[S])
    alpha = _alpha(99)
    body = _message(31, 7)
    long_msg = _message(200, 11)

    def raw(frame, message=b'', r=None, a=alpha):
        return tr.seal_raw_frame(C, pk, ROUND[S], S, a, frame, message=message, r=r)

    def first_invalid(name, variants):
        """the first variant the oracle answers with INVALID_SIGNATURE (a garbled alpha opens a pseudo-random frame, which the length
        rule may refuse first)"""
        for ct, sg_pt in variants:
            it = item(name, ct, sg_pt, S)
            if it['want'] == (INVALID_SIGNATURE, None):
                return it
        raise AssertionError(name)

    good = raw(tr.frame_of(long_msg), message=long_msg)
    r_good = tr.scalar_r(alpha, long_msg)
    flip = lambda b, bit: bytes(x ^ (1 << (bit & 7)) if i == bit >> 3 else x for i, x in enumerate(b))  # noqa: E731
    crafted = [
        item('w empty', raw(b''), sig, S),
        item('unterminated varint, 32 bytes 0x80', raw(b'\x80' * 32), sig, S),
        item('length one beyond the frame', raw(bytes([32]) + body, message=body), sig, S),
        item('length exactly filling the frame', raw(bytes([31]) + body, message=body), sig, S),
        item('good, 200 bytes', good, sig, S),
        first_invalid('one bit flipped in u', (((C.pk_curve.mul(C.pk_gen, r_good ^ (1 << b)), good[1], good[2], S), sig) for b in range(16))),
        first_invalid('one bit flipped in v', (((good[0], flip(good[1], b), good[2], S), sig) for b in range(64))),
        item('one bit flipped in w', (good[0], good[1], flip(good[2], 8 * 40 + 3), S), sig, S),
        first_invalid('one bit flipped in the signature', ((good, round_sig(sg, S, ROUND[S], 1 << b)) for b in range(16))),
        item('scheme mismatch', (good[0], good[1], good[2], ref.POP), sig, S),
        item('identity u', (None, good[1], good[2], S), sig, S),
        item('identity u and a length beyond the frame', (None,) + raw(bytes([32]) + body, message=body)[1:], sig, S),
        item('a length beyond the frame and a wrong u', (C.pk_curve.mul(C.pk_gen, 5),) + raw(bytes([32]) + body, message=body)[1:], sig, S),
        item('undecodable u', good, sig, S, u_bad='range'),
        item('undecodable u and scheme mismatch', (good[0], good[1], good[2], ref.AUG), sig, S, u_bad='flag'),
        item('good again', good, sig, S),
    ]
    names = [it['name'] for it in crafted]
    for nm, st in (('w empty', OK), ('unterminated varint, 32 bytes 0x80', OK), ('length one beyond the frame', BAD_FRAME),
                   ('length exactly filling the frame', OK), ('one bit flipped in w', INVALID_SIGNATURE), ('scheme mismatch', INVALID_SCHEME),
                   ('identity u', PK_IDENTITY), ('identity u and a length beyond the frame', PK_IDENTITY),
                   ('a length beyond the frame and a wrong u', BAD_FRAME), ('good again', OK)):
        assert crafted[names.index(nm)]['want'][0] == st, nm
    assert crafted[1]['want'] == (OK, b'') and crafted[0]['want'] == (OK, b'') and crafted[3]['want'] == (OK, body)
    # the one signature that matters per group: the flipped one needs a group of its own
    flipped = crafted.pop(names.index('one bit flipped in the signature'))
    tweak = next(1 << b for b in range(16) if item('x', good, round_sig(sg, S, ROUND[S], 1 << b), S)['want'] == flipped['want'])
    groups.append(group(S, crafted))
    groups.append(group(S, [flipped], sig=round_sig(sg, S, ROUND[S], tweak)))
    other = round_sig(sg, S, b'round 999')
    groups.append(group(S, [item('a signature of another round', good, other, S), item('... and its w empty', raw(b''), other, S)], sig=other))
    groups.append(group(S, [item('identity signature', good, None, S), item('identity signature and identity u', (None,) + good[1:], None, S),
                            item('identity signature and scheme mismatch', good[:3] + (ref.AUG,), None, S)], sig=None))
    groups.append(group(S, [item('undecodable signature', good, sig, S), item('undecodable signature and u', good, sig, S, u_bad='range'),
                            item('undecodable signature and scheme mismatch', good[:3] + (ref.POP,), sig, S)], sig_bad='flag'))
    groups.append(group(2, []))
    want = {it['name']: it['want'][0] for g in groups for it in g['items']}
    assert want['identity signature'] == want['identity signature and identity u'] == SIG_IDENTITY and want['identity signature and scheme mismatch'] == INVALID_SCHEME
    return groups


def expected_item(sg, grp, it, fmt):
    """(status, message or None) of one item under a format: on the wire formats a member that does not decode comes first, u before sig"""
    if fmt in (COMPRESSED, LEGACY):
        if it['u_bad']:
            return decode_status(3 - sg, bad_wire(3 - sg, it['u_bad'], fmt), fmt), None
        if grp['sig_bad']:
            return decode_status(sg, bad_wire(sg, grp['sig_bad'], fmt), fmt), None
    return it['want']


def render_groups(sg, groups, fmt, seed=0):
    """the groups as api.timecrypt_open_batch takes them, and what it must return: (api groups, [message or None], [status]).  On the
    raw formats the members that exist as wire bytes only are left out (the items, and the groups of such a signature)."""
    rng = random.Random(31 * fmt + seed)
    wire = fmt in (COMPRESSED, LEGACY)
    out, msgs, sts = [], [], []
    for g in groups:
        if g['sig_bad'] and not wire:
            continue
        sig = bad_wire(sg, g['sig_bad'], fmt) if g['sig_bad'] else render_point(sg, g['sig'], fmt, rng)
        cts = []
        for it in g['items']:
            if it['u_bad'] and not wire:
                continue
            u = bad_wire(3 - sg, it['u_bad'], fmt) if it['u_bad'] else render_point(3 - sg, it['u'], fmt, rng)
            cts.append((u, it['v'], it['w'], it['scheme']))
            st, m = expected_item(sg, g, it, fmt)
            sts.append(st)
            msgs.append(m)
        out.append((sig, g['scheme'], cts))
    return out, msgs, sts


def tiled_groups(sg, n):
    """n items made by repeating the groups of timelock_groups(sg) that hold no wire-only member, the last one cut"""
    base = [g for g in timelock_groups(sg) if not g['sig_bad'] and g['items'] and not any(it['u_bad'] for it in g['items'])]
    out, left, k = [], n, 0
    while left:
        g = base[k % len(base)]
        items = g['items'][:left]
        out.append(dict(g, items=items))
        left -= len(items)
        k += 1
    return out
