"""Inputs of tests/test_gpu_secure_batch.py and tests/secure_batch_worker.py: sets of keys k_i g made on the device, and the
signature that verify_secure accepts for them, derived in Python (tests/secure_coeffs.py), not by the library's aggregate_secure."""
import random

import util
from secure_coeffs import R, aggregate_secret

AUG_DST = {1: b'BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_AUG_', 2: b'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_AUG_'}


def identity(group):
    return util.g1_raw(None) if group == 1 else util.g2_raw(None)


def key_points(api, sg, ks):
    """k g in the key group of sig_group sg (RAW_PROJ), one sign_batch call for all of them."""
    return api.sign_batch(sg, api.BASIC, ks, [b''] * len(ks))[0] if ks else []


def sign(api, sg, scheme, sk, msg):
    """sk H(msg) under the scheme's DST.  MessageAugmentation without the key prefix: verify_secure never prefixes (reference
    src/secure_aggregation.rs:236-246), so this is sk times the message hashed under the Aug DST (one-point MSM)."""
    if sk % R == 0:
        return identity(sg)
    if scheme == api.AUG:
        h = api.hash_to_point(sg, [msg], AUG_DST[sg])[0]
        return api.point_sum(sg, [h], [sk % R])
    return api.sign_batch(sg, scheme, [sk % R], [msg])[1][0]


def valid_sets(api, sg, scheme, sizes, rng, legacy=False, tag=b''):
    """[(pks, sig, msg, ks)] for the given set sizes, every one valid."""
    ks_all = [rng.randrange(1, R) for _ in range(sum(sizes))]
    pts = key_points(api, sg, ks_all)
    kb_all = api.serialize(3 - sg, pts, legacy=legacy) if pts else []
    out, at = [], 0
    for s, t in enumerate(sizes):
        ks, pks, kb = ks_all[at:at + t], pts[at:at + t], kb_all[at:at + t]
        at += t
        msg = b'secure batch %d %s' % (s, tag)
        out.append((pks, sign(api, sg, scheme, aggregate_secret(kb, ks), msg), msg, ks))
    return out


def mixed_sets(api, sg, scheme, seed, big=0):
    """Valid and invalid sets of every kind the single call distinguishes (test 2 of tests/test_gpu_secure_batch.py)."""
    rng = random.Random(seed)
    sizes = [5, 40, 7, 9, 12, 6, 3, 4] + ([big] if big else [])
    v = valid_sets(api, sg, scheme, sizes, rng)
    pk_group = 3 - sg
    extra = key_points(api, sg, [rng.randrange(1, R) for _ in range(2)])
    sets = []
    sets.append(v[0][:3])                                                          # valid
    sets.append((v[1][0], v[1][1], v[1][2] + b'!'))                                # wrong message
    sets.append((v[2][0][:-1], v[2][1], v[2][2]))                                  # a key missing
    sets.append((v[3][0][:4] + [extra[0]] + v[3][0][5:], v[3][1], v[3][2]))        # a key swapped for another
    perm = list(range(12))
    rng.shuffle(perm)
    sets.append(([v[4][0][i] for i in perm], v[4][1], v[4][2]))                    # permuted order: still valid
    # duplicate keys: signed over the list with its duplicates (valid), and a duplicate added after signing (invalid)
    ks = v[5][3] + v[5][3][:3]
    pks = v[5][0] + v[5][0][:3]
    kb = api.serialize(pk_group, pks)
    msg = b'duplicates'
    sets.append((pks, sign(api, sg, scheme, aggregate_secret(kb, ks), msg), msg))
    sets.append((v[6][0] + v[6][0][:1], v[6][1], v[6][2]))
    sets.append(([], identity(sg), b'empty, identity signature'))
    sets.append(([], v[7][1], b'empty, other signature'))
    sets.append((v[7][0], identity(sg), v[7][2]))                                  # identity signature, keys present
    sets.append(([identity(pk_group)] * 3, v[0][1], b'identity keys'))
    sets.append((v[0][0] + [extra[1]], v[0][1], v[0][2]))                          # an extra key
    if big:
        sets.append(v[8][:3])                                                      # a set above the default plan split
        sets.append((v[8][0], v[8][1], v[8][2] + b'?'))
    return sets
