"""Inputs of tests/test_gpu_aggregate_batch.py and tests/aggregate_batch_worker.py: ragged sets of keys k_i g with signatures
k_i H(m) made on the device by sign_batch, duplicates whose signature carries another secret, and the aggregate
aggregate_secure must return for them in closed form: (sum_i t_i k_first(i)) H(m) with t from tests/secure_coeffs.py."""
import random

import util
from secure_coeffs import R, secure_coefficients

MSG = b'one message for every signer'
CLOSED_SIZES = [0, 1, 2, 3, 57, 64, 65, 130]
# (set size, position, the earlier position whose key it repeats): inside one tile, and two tiles later
CLOSED_DUPLICATES = {57: (40, 10), 130: (129, 3)}


def identity(group):
    return util.g1_raw(None) if group == 1 else util.g2_raw(None)


def signed(api, sg, ks, msg=MSG):
    """(keys k g, signatures k H(msg)) as RAW_PROJ lists, one sign_batch call"""
    return api.sign_batch(sg, api.BASIC, ks, [msg] * len(ks)) if ks else ([], [])


def closed_form_sets(api, sg, sizes, rng, duplicates=CLOSED_DUPLICATES):
    """[(pks, sigs, ks, first)]: ks[i] is the secret behind sigs[i]; pks[i] = pks[first[i]].  A duplicated key keeps a signature
    under a secret of its own, which the first-match rule must ignore."""
    ks_all = [rng.randrange(1, R) for _ in range(sum(sizes))]
    pks_all, sigs_all = signed(api, sg, ks_all)
    out, at = [], 0
    for t in sizes:
        pks, sigs, ks = pks_all[at:at + t], sigs_all[at:at + t], ks_all[at:at + t]
        at += t
        first = list(range(t))
        if t in duplicates:
            pos, src = duplicates[t]
            pks[pos], first[pos] = pks[src], src
        out.append((pks, sigs, ks, first))
    return out


def expected_secret(key_bytes, ks, first):
    """sum_i t_i k_first(i) mod r, t_i the coefficient of INPUT key i (its sorted position's, duplicates in input order)"""
    _, _, ts = secure_coefficients(key_bytes)
    return sum(t * ks[f] for t, f in zip(ts, first)) % R


def expected_aggregates(api, sg, sets, legacy=False):
    """the serialised aggregate of every set of closed_form_sets"""
    es = []
    for pks, _, ks, first in sets:
        kb = api.serialize(3 - sg, pks, legacy=legacy) if pks else []
        es.append(expected_secret(kb, ks, first))
    live = [i for i, e in enumerate(es) if e]
    pts = signed(api, sg, [es[i] for i in live])[1]
    out = [api.serialize(sg, [identity(sg)])[0]] * len(sets)
    for i, p in zip(live, api.serialize(sg, pts) if pts else []):
        out[i] = p
    return out


def mixed_sets(api, sg, seed, big=0):
    """[(pks, sigs)] with identity keys, identity signatures, duplicates, a repeated set, an empty set; `big`: one more set of
    that many keys with a duplicate at its end."""
    rng = random.Random(seed)
    v = [s[:2] for s in closed_form_sets(api, sg, [5, 1, 9, 0, 12, 3, 66], rng, duplicates={9: (7, 2), 66: (65, 1)})]
    g = 3 - sg
    sets = [v[0], v[1], v[2], v[3]]
    sets.append((v[4][0][:3] + [identity(g)] + v[4][0][4:], v[4][1]))                       # an identity key
    sets.append((v[4][0], v[4][1][:5] + [identity(sg)] * 2 + v[4][1][7:]))                  # identity signatures
    sets.append(([identity(g)] * 3, v[5][1]))                                               # identity keys only: all equal
    sets.append(v[0])                                                                       # a repeated set
    sets.append(v[6])
    sets.append((v[5][0], [identity(sg)] * 3))                                              # sums to the identity
    if big:
        pks, sigs, _, _ = closed_form_sets(api, sg, [big], rng, duplicates={big: (big - 1, 0)})[0]
        sets.append((pks, sigs))
    return sets
