"""Inputs of tests/test_gpu_multi_batch.py and tests/multi_batch_worker.py: sets of keys k_i g made on the device, and the
signature MultiSignature::verify accepts for them in closed form: (sum k_i mod r) H(msg), made by sign_batch for that secret (under
MessageAugmentation sign_batch prefixes that secret's own key, which is the sum of the set's keys)."""
import random

import util
from util import P, c

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def identity(group):
    return util.g1_raw(None) if group == 1 else util.g2_raw(None)


def key_points(api, sg, ks):
    """k g in the key group of sig_group sg (RAW_PROJ), one sign_batch call for all of them."""
    return api.sign_batch(sg, api.BASIC, ks, [b''] * len(ks))[0] if ks else []


def signatures(api, sg, scheme, sks, msgs):
    """sk_i H(msg_i) under the scheme (one sign_batch call); the identity for sk = 0."""
    live = [i for i, sk in enumerate(sks) if sk % R]
    sigs = api.sign_batch(sg, scheme, [sks[i] % R for i in live], [msgs[i] for i in live])[1] if live else []
    out = [identity(sg)] * len(sks)
    for i, s in zip(live, sigs):
        out[i] = s
    return out


def _coords(group, raw):
    """RAW_PROJ bytes -> Jacobian (X, Y, Z), the point being (X / Z^2, Y / Z^3); Fp2 coordinates as pairs."""
    if group == 1:
        return [util.fp_from_raw(raw[48 * k:48 * k + 48]) for k in range(3)]
    return [(util.fp_from_raw(raw[96 * k:96 * k + 48]), util.fp_from_raw(raw[96 * k + 48:96 * k + 96])) for k in range(3)]


def z_is_one(group, raw):
    return _coords(group, raw)[2] == (1 if group == 1 else (1, 0))


def rescale(group, raw, rng):
    """The same point with another Z: (X l^2, Y l^3, Z l) for a random l != 0, 1 (oracle field arithmetic)."""
    x, y, z = _coords(group, raw)
    if group == 1:
        l = rng.randrange(2, P)
        return util.fp_raw(x * l * l) + util.fp_raw(y * l * l * l) + util.fp_raw(z * l)
    l = (rng.randrange(2, P), rng.randrange(1, P))
    l2 = c.f2_sqr(l)
    return util.fp2_raw(c.f2_mul(x, l2)) + util.fp2_raw(c.f2_mul(y, c.f2_mul(l2, l))) + util.fp2_raw(c.f2_mul(z, l))


def negate(group, raw):
    x, y, z = _coords(group, raw)
    if group == 1:
        return util.fp_raw(x) + util.fp_raw(-y) + util.fp_raw(z)
    return util.fp2_raw(x) + util.fp2_raw(((-y[0]) % P, (-y[1]) % P)) + util.fp2_raw(z)


def z_one(api, group, raws):
    """The same points as deserialisation leaves them: Z = 1."""
    pts, sts = api.deserialize(group, api.serialize(group, raws))
    assert all(s == 0 for s in sts) and all(z_is_one(group, p) for p in pts)
    return pts


def valid_sets(api, sg, scheme, sizes, rng, tag=b''):
    """[(pks, sig, msg, ks)] for the given set sizes: the signature of set s is (sum ks) H(msg), so every non-empty set verifies;
    an empty set gets the identity signature."""
    ks_all = [rng.randrange(1, R) for _ in range(sum(sizes))]
    pts = key_points(api, sg, ks_all)
    msgs = [b'multi batch %d %s' % (s, tag) for s in range(len(sizes))]
    sets, at = [], 0
    for t in sizes:
        sets.append((pts[at:at + t], ks_all[at:at + t]))
        at += t
    sigs = signatures(api, sg, scheme, [sum(ks) for _, ks in sets], msgs)
    return [(pks, sig, msg, ks) for (pks, ks), sig, msg in zip(sets, sigs, msgs)]


# positions of mixed_sets and the status each must have (api.OK = 0, INVALID_SIGNATURE = 1, SIG_IDENTITY = 2, PK_IDENTITY = 3)
MIXED_EXPECT = [0, 1, 2, 2, 3, 3, 0, 0, 0, 0, 1]


def mixed_sets(api, sg, scheme, seed, sizes=()):
    """Every kind of set blsgpu_multi_verify distinguishes (test 2 of tests/test_gpu_multi_batch.py), then one valid set per entry
    of `sizes`."""
    rng = random.Random(seed)
    g = 3 - sg
    v = valid_sets(api, sg, scheme, [5, 7, 4, 3, 6, 9] + list(sizes), rng, tag=b'mixed')
    k1, k2 = rng.randrange(1, R), rng.randrange(1, R)
    p1, p2 = z_one(api, g, key_points(api, sg, [k1, k2]))
    s_pp, s_qq = signatures(api, sg, scheme, [2 * k1, 2 * k2], [b'P + P', b'Q + Q'])
    sets = []
    sets.append(v[0][:3])                                                          # 0 valid
    sets.append((v[1][0], v[1][1], v[1][2] + b'!'))                                # 1 wrong message
    sets.append((v[2][0], identity(sg), v[2][2]))                                  # 2 identity signature, keys present
    sets.append(([], identity(sg), b'empty, identity signature'))                  # 3
    sets.append(([], v[3][1], b'empty, other signature'))                          # 4
    sets.append(([p1, negate(g, p1)], v[3][1], v[3][2]))                           # 5 keys that cancel
    sets.append(([p1, p1], s_pp, b'P + P'))                                        # 6 doubling, both Z = 1 (the mixed addition's, or the fold's)
    sets.append(([rescale(g, p2, rng), rescale(g, p2, rng)], s_qq, b'Q + Q'))      # 7 doubling, one point under two different Z
    pks = v[4][0]
    sets.append((pks[:2] + [identity(g)] + pks[2:] + [identity(g)] * 2, v[4][1], v[4][2]))     # 8 identity keys among valid ones
    pks = z_one(api, g, v[5][0][:4]) + [rescale(g, p, rng) for p in v[5][0][4:]]
    rng.shuffle(pks)
    assert sum(z_is_one(g, p) for p in pks) == 4 and len(pks) == 9
    sets.append((pks, v[5][1], v[5][2]))                                           # 9 Z = 1 and Z != 1 keys mixed
    sets.append((v[0][0][:-1], v[0][1], v[0][2]))                                  # 10 a key missing
    return sets + [s[:3] for s in v[6:]]
