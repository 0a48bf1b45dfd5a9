"""Inputs of tests/test_gpu_keyset.py and tests/keyset_worker.py: a key table of about 320 entries per key group -- keys k_i g made
on the device by sign_batch, as wire bytes -- with the entries a registry really holds: the identity, one key at two positions, one
blob that does not decode and, for the Legacy form (Bls12381G2Impl only), one blob with a bad Legacy header.  Sets are lists of
positions; their closed-form signatures come from the secrets (multi: the sum; secure: tests/secure_coeffs.py)."""
import random

import multi_batch_cases as mb
import secure_batch_cases as sb
from secure_coeffs import R, aggregate_secret

N = 320
GEN, IDENT, DUP_A, DUP_B, BAD, BAD_LEGACY = 0, 5, 7, 200, 11, 13
SIZES = [0, 1, 2, 3, 63, 64, 65, 130, 300]
X_ABS = 0xd201000000010000
LAM = X_ABS * X_ABS % R            # phi(P) = [-z^2] P on G1; psi(P) = [-z] P on G2
SPECIAL_SCALARS = [0, 1, 2, R - 1, R, R + 1, 2 ** 128 - 1, 2 ** 128, 2 ** 255, 2 ** 256 - 1, LAM, LAM - 1, LAM + 1, R - LAM, X_ABS, X_ABS - 1, X_ABS + 1]

_cache = {}


def table(api, sg, legacy=False):
    """dict(ks, blobs, fmt, status, valid): ks[i] is entry i's secret (0: the identity, None: an invalid entry), blobs the wire
    bytes the table is created from, status what blsgpu_deserialize says about each, valid the positions of the finite keys."""
    key = (sg, legacy)
    if key in _cache:
        return _cache[key]
    rng = random.Random(1000 + 10 * sg + legacy)
    g = 3 - sg
    ks = [rng.randrange(1, R) for _ in range(N)]
    ks[GEN] = 1
    ks[DUP_B] = ks[DUP_A]
    blobs = api.serialize(g, mb.key_points(api, sg, ks), legacy=legacy)
    w = len(blobs[0])
    ks[IDENT] = 0
    blobs[IDENT] = b'\xc0' + bytes(w - 1)
    ks[BAD] = None
    blobs[BAD] = bytes([blobs[BAD][0] & 0x9f | 0x1f]) + b'\xff' * (w - 1)      # x >= p
    if legacy:
        ks[BAD_LEGACY] = None
        blobs[BAD_LEGACY] = bytes([blobs[BAD_LEGACY][0] | 0x40]) + blobs[BAD_LEGACY][1:]
    pts, status = api.deserialize(g, blobs, legacy=legacy)
    t = dict(ks=ks, blobs=blobs, fmt=api.FMT_LEGACY if legacy else api.FMT_COMPRESSED, status=status, points=pts,
             valid=[i for i, k in enumerate(ks) if k])
    assert status[BAD] == api.BAD_ENCODING and (not legacy or status[BAD_LEGACY] == api.LEGACY_FORMAT)
    assert [i for i, s in enumerate(status) if s] == [BAD] + ([BAD_LEGACY] if legacy else [])
    _cache[key] = t
    return t


def draw(t, sizes, rng):
    """index lists of the given sizes over the finite keys, with repetition (every set of two or more names one key twice)"""
    out = []
    for n in sizes:
        idx = [rng.choice(t['valid']) for _ in range(n)]
        if n >= 2:
            idx[-1] = idx[0]
        out.append(idx)
    return out


def multi_sets(api, sg, scheme, t, rng, sizes=SIZES, idxs=None):
    """[(idx, sig, msg)], every non-empty set valid for MultiSignature::verify: the signature is (sum of the secrets) H(msg).
    idxs: the index lists themselves, in place of a draw."""
    idxs = idxs or draw(t, sizes, rng)
    msgs = [b'keyset multi %d' % s for s in range(len(idxs))]
    sigs = mb.signatures(api, sg, scheme, [sum(t['ks'][i] for i in idx) for idx in idxs], msgs)
    return list(zip(idxs, sigs, msgs))


def secure_sets(api, sg, scheme, t, rng, legacy=False, sizes=SIZES, idxs=None):
    """[(idx, sig, msg)], every non-empty set valid for verify_secure over the keys' Modern or Legacy bytes (idxs: as multi_sets)"""
    g = 3 - sg
    out = []
    for s, idx in enumerate(idxs or draw(t, sizes, rng)):
        msg = b'keyset secure %d' % s
        kb = api.serialize(g, [t['points'][i] for i in idx], legacy=legacy) if idx else []
        out.append((idx, sb.sign(api, sg, scheme, aggregate_secret(kb, [t['ks'][i] for i in idx]) if idx else 0, msg), msg))
    return out


def tampered(api, sg, sets):
    """from valid sets (sizes SIZES): wrong message, identity signature, no keys under a real signature, a key missing, the identity
    entry and the repeated key added without signing for them -- at least four distinct statuses"""
    big = sets[-1]
    return [sets[4], (sets[5][0], sets[5][1], sets[5][2] + b'!'), (sets[6][0], mb.identity(sg), sets[6][2]), ([], sets[3][1], sets[3][2]),
            (sets[7][0][:-1], sets[7][1], sets[7][2]), (big[0] + [IDENT], big[1], big[2]), (sets[2][0] + [DUP_B], sets[2][1], sets[2][2]),
            ([IDENT], sets[1][1], sets[1][2]), sets[0]]


def gathered(api, ks, sets):
    """the sets with their keys by value, as KeySet.get hands them out"""
    return [(ks.get(idx)[0], sig, msg) for idx, sig, msg in sets]
