"""The MSM (blsgpu_msm_g1/g2, verify_secure's and aggregate_secure's key / signature sums) at the inputs that reach its exceptional
branches on the DEVICE, under every kind of window plan the tuning and A/B knobs allow.

Random scalars put ~50 entries in each bucket: no bucket accumulator then ever meets its next point or its negative, no merge
operand or chunk running sum collides, no bucket is empty.  The cases below are crafted from the sub-scalars of the
second-generation decomposition (csrc/msm2.cuh: G1 k = a0 + a1 z^2, G2 k = a0 + a1 z + a2 z^2 + a3 z^3): sub-scalar values 1 .. 8
are a digit of window 0 under every plan (every window is at least 4 bits wide), so a case hits the same buckets whatever the knobs,
and the padding (identity points or zero scalars) leaves the crafted entries alone in their buckets.

Every expected value is ONE oracle scalar multiplication: the points are sk_i * g (made on the device by blsgpu_sign_batch), so
sum t_i P_i = (sum t_i sk_i mod r) * g, compared as compressed bytes; verify_secure's expected verdicts come from
ref.secure_coefficients and a signature of the known total scalar, aggregate_secure's value from ref.aggregate_secure.
The knobs are read once at library init, so each plan runs in a child process (tests/msm_worker.py), one at a time."""
import json
import os
import random
import subprocess
import sys

import pytest

import util
from util import c, ref

pytestmark = pytest.mark.gpu

R = c.R
Z = 0xd201000000010000          # |x| of the curve: the base of the endomorphism split
THRESHOLD = 1024                # from here on the bucket method runs (below: one double-and-add lane per item)
E_OF = {1: 2, 2: 4}             # sub-scalars per scalar
GEN = {1: (c.E1, c.G1_GEN, c.g1_compress), 2: (c.E2, c.G2_GEN, c.g2_compress)}


def k_of(group, subs):
    """The scalar whose decomposition is `subs` (G1: [a0, a1] with k = a0 + a1 z^2; G2: base-z digits)."""
    if group == 1:
        a0, a1 = (list(subs) + [0, 0])[:2]
        assert a0 < Z * Z
        k = a0 + a1 * Z * Z
    else:
        assert all(a < Z for a in subs)
        k = sum(a * Z ** j for j, a in enumerate(subs))
    assert 0 <= k < R, hex(k)
    return k


def sub(group, j, v):
    """Scalar with sub-scalar j = v and the others 0."""
    s = [0] * E_OF[group]
    s[j] = v
    return k_of(group, s)


def pad(entries, n, mode):
    """Pad a list of (sk or None, t) to n entries: identity points (mode 'inf') or a filler point with scalar 0 ('zero')."""
    filler = (None, 12345) if mode == 'inf' else (0x5eed, 0)
    return list(entries) + [filler] * (n - len(entries))


def crafted(group):
    """name -> [(sk, t)]: the exceptional additions of the bucket, merge, chunk, fold and normalize stages."""
    E = E_OF[group]
    rng = random.Random(1000 + group)
    P = 0x1234567 + group               # the secret keys of the points
    Q = 0x7654321 + 3 * group
    cases = {}
    # bucket doubling: m copies of one point on one digit (one part and across parts, for every Q <= 8)
    for m in (2, 3, 5, 9, 17):
        cases['dbl%d' % m] = [(P, sub(group, m % E, 1 + m % 8))] * m
    # bucket cancellation: P, -P, P on one digit (the fill order is atomic: every order must give the right sum)
    cases['cancel'] = [(P, 3), (R - P, 3), (P, 3)]
    cases['cancel_pair'] = [(P, sub(group, E - 1, 2)), (R - P, sub(group, E - 1, 2)), (Q, 1)]
    # collision across endomorphism images: [z^2]P (G1) / [z^j]P (G2) on digit d of image 0 meets image j of P on digit d
    for j in range(1, E):
        zj = Z ** (2 * j) if group == 1 else Z ** j
        cases['endo%d' % j] = [(P, sub(group, j, 5)), (P * zj % R, 5)]
        cases['endo%d_neg' % j] = [(P, sub(group, j, 5)), ((R - P) * zj % R, 5), (Q, sub(group, j, 6))]
    # chunk running sums: equal neighbours, opposite neighbours (the running sum passes through infinity), empty buckets
    # between full ones, digits above the chunk size so that lo != 0
    cases['run_equal'] = [(P, 1), (P, 2), (P, 3), (P, 4)]
    cases['run_opposite'] = [(P, 1), (R - P, 2), (P, 3), (R - P, 4)]
    cases['run_gaps'] = [(P, 1), (Q, 5), (P, 8)]
    cases['run_high'] = [(P, 6), (R - P, 7), (P * 7 % R, 5), (Q, 8)]
    cases['run_digits'] = [(P + d, sub(group, d % E, 1 + d)) for d in range(8)] + [(Q, rng.randrange(1, 1 << 16))]
    # fold and normalize: equal chunk partials (5P in bucket 1, P in bucket 5), opposite ones, a total that is the identity
    cases['fold_equal'] = [(5 * P, 1), (P, 5)]
    cases['fold_opposite'] = [(R - 5 * P, 1), (P, 5)]
    k = rng.randrange(1, R)
    cases['total_identity'] = [(P, k), (P, R - k), (Q, 3), (R - Q, 3)]
    cases['total_identity_images'] = [(P, sub(group, E - 1, 1)), (P * (Z ** (2 if group == 1 else E - 1)) % R, R - 1)]
    # sub-scalar edges
    top = [Z - 1] * E
    if group == 2:           # z^4 - 1 > r: the largest a3 that keeps k < r
        top[3] = min(Z - 1, (R - 1 - sum((Z - 1) * Z ** j for j in range(3))) // Z ** 3)
    else:
        top[1] = min(Z * Z - 1, (R - 1 - top[0]) // (Z * Z))
    cases['sub_max'] = [(P, k_of(group, top)), (Q, k_of(group, [Z - 1] * E if group == 1 else [Z - 1] * 3))]
    width = 128 if group == 1 else 64
    ones = []
    for b in (width - 1, width - 2, 33, 17, 5):
        v = (1 << b) - 1
        if group == 1 and v >= Z * Z:
            continue
        if group == 2 and v >= Z:
            continue
        ones.append(k_of(group, [v] * E) if group == 1 else k_of(group, [v] * 3))
    cases['ones'] = [(P + i, t) for i, t in enumerate(ones)]
    cases['single_sub'] = [(P + j, sub(group, j, rng.randrange(1, Z))) for j in range(E)]
    cases['z_multiples'] = [(P + j, (j + 2) * Z ** j) for j in range(4)] + [(Q, Z ** 2)]
    cases['edges'] = [(P, 0), (Q, 1), (P + 1, R - 1), (P + 2, R), (P + 3, 2 ** 256 - 1), (P + 4, R + 7)]
    return cases


def build_msm_cases(group, small=True, extra=None):
    """The case list of one child for one group: every crafted case padded to THRESHOLD (alternately with identity points
    and zero scalars); the skew and input-form cases; with `small` the crafted cases again below the threshold."""
    out = []
    cr = crafted(group)
    if extra:
        cr.update(extra)
    for i, (name, ent) in enumerate(sorted(cr.items())):
        out.append((name, pad(ent, THRESHOLD, 'inf' if i % 2 else 'zero')))
    rng = random.Random(2000 + group)
    out.append(('all_zero_scalars', [(0x99 + i, 0) for i in range(THRESHOLD)]))
    out.append(('all_identity', [(None, rng.randrange(R)) for _ in range(THRESHOLD)]))
    out.append(('skew', [(0xabcdef, rng.randrange(1, R))] * 4096))
    mix = [(0x1000 + (i % 37), rng.choice([1, 2, 3, 5, 8, R - 1, rng.randrange(R)])) for i in range(1500)]
    for i in range(0, 1500, 97):
        mix[i] = (None, mix[i][1])
    out.append(('mixed_1500', mix))
    if small:
        names = ('dbl2', 'dbl17', 'cancel', 'endo1', 'run_opposite', 'fold_opposite', 'total_identity', 'edges', 'sub_max')
        for n in (1, 2, 64, 65, 1023):
            for name in names:
                out.append(('%s@%d' % (name, n), pad(cr[name][:n], n, 'zero')))
    return out


def form_cases(group):
    """Points given as bytes: Z != 1 projective points and FMT_RAW_AFFINE, around and below the threshold (oracle points)."""
    rng = random.Random(3000 + group)
    E, gen, _ = GEN[group]
    raw, aff = (util.g1_raw, util.g1_aff_raw) if group == 1 else (util.g2_raw, util.g2_aff_raw)
    sks = [0x777 + 11 * i for i in range(4)]
    pts = [E.mul(gen, s) for s in sks]
    out = []
    for n in (THRESHOLD, 65):
        ent = [(i % 4, rng.choice([1, 2, 5, rng.randrange(R)])) for i in range(n)]
        ent[1] = (0, ent[0][1])              # the same point and digit twice: the bucket doubles
        out.append(('proj_z_%d' % n, [(raw(pts[i], rng).hex(), sks[i], t) for i, t in ent], 0))
        out.append(('affine_%d' % n, [(aff(pts[i]).hex(), sks[i], t) for i, t in ent], 1))
        inf = [(raw(None, rng).hex(), 0, rng.randrange(R)) for _ in range(3)]
        out.append(('proj_z_inf_%d' % n, inf + [(raw(pts[i], rng).hex(), sks[i], t) for i, t in ent[3:]], 0))
    return out


def v1_windows(cbits):
    """First-generation plan restated (csrc/blsgpu.hip msm_make_plan): W windows of c bits, the last one clast bits."""
    W = 255 // cbits
    clast = 255 - cbits * (W - 1)
    if clast > 16:
        W += 1
        clast = 255 - cbits * (W - 1)
    return W, clast


def v1_cases(group, cbits):
    """Digits of the first generation's unsigned windows of c bits: collisions in a middle window and in the last one."""
    W, clast = v1_windows(cbits)
    P, Q = 0x3141 + group, 0x2718 + group
    cases = {}
    for w in (1, W // 2, W - 1):
        sh = 1 << (cbits * w)
        top = (1 << (clast if w == W - 1 else cbits)) - 1
        cases['v1w%d_dbl' % w] = [(P, 3 * sh)] * 3
        cases['v1w%d_cancel' % w] = [(P, 2 * sh), (R - P, 2 * sh), (Q, 2 * sh), (Q, sh)]
        cases['v1w%d_top' % w] = [(P, top * sh % R), (P, (top - 1) * sh % R), (R - P, top * sh % R)]
    return cases


def expected_msm(group, ent):
    E, gen, comp = GEN[group]
    s = sum((sk or 0) * t for sk, t in ent) % R
    return comp(E.mul(gen, s)).hex()


def spec_and_expect(plan_cases):
    """(spec for the worker, {name: expected compressed hex}) of one child's MSM cases."""
    spec, want = [], {}
    for group, cases, forms in plan_cases:
        for name, ent in cases:
            key = 'g%d/%s' % (group, name)
            spec.append({'group': group, 'name': key, 'pts': [sk for sk, _ in ent], 'ts': ['%x' % t for _, t in ent]})
            want[key] = expected_msm(group, ent)
        for name, ent, fmt in forms:
            key = 'g%d/%s' % (group, name)
            spec.append({'group': group, 'name': key, 'pts': [h for h, _, _ in ent], 'ts': ['%x' % t for _, _, t in ent], 'fmt': fmt})
            want[key] = expected_msm(group, [(sk, t) for _, sk, t in ent])
    return spec, want


def run_child(tmp_path, name, env, spec):
    path = os.path.join(str(tmp_path), name + '.json')
    with open(path, 'w') as f:
        json.dump(spec, f)
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'msm_worker.py'), path],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# plan name -> (environment, run the cases below the threshold too, first-generation window bits)
AB = {'BLSGPU_AB_KNOBS': '1'}
PLANS = [
    ('default', {}, True, None),
    ('c4_q8', {'BLSGPU_MSM2_C': '4', 'BLSGPU_MSM2_Q': '8'}, False, None),                        # base 4, rem 1
    ('c5_ch1', {'BLSGPU_MSM2_C': '5', 'BLSGPU_MSM2_CH': '1'}, False, None),                       # G2 rem 0, G1 rem W - 1
    ('c6_q1_chmax', {'BLSGPU_MSM2_C': '6', 'BLSGPU_MSM2_Q': '1', 'BLSGPU_MSM2_CH': '65536'}, False, None),
    ('c8_q8_ch1', {'BLSGPU_MSM2_C': '8', 'BLSGPU_MSM2_Q': '8', 'BLSGPU_MSM2_CH': '1'}, False, None),
    ('c12_q1', {'BLSGPU_MSM2_C': '12', 'BLSGPU_MSM2_Q': '1'}, False, None),                      # G2 rem 0
    ('c16_q8_chmax', {'BLSGPU_MSM2_C': '16', 'BLSGPU_MSM2_Q': '8', 'BLSGPU_MSM2_CH': '65536'}, False, None),  # 17-bit first window
    ('v1_c4_ch1', dict(AB, BLSGPU_MSM_V1='1', BLSGPU_MSM_C='4', BLSGPU_MSM_CH='1'), False, 4),
    ('v1_c8', dict(AB, BLSGPU_MSM_V1='1', BLSGPU_MSM_C='8'), False, 8),
    ('v1_c13_chmax', dict(AB, BLSGPU_MSM_V1='1', BLSGPU_MSM_C='13', BLSGPU_MSM_CH='65536'), False, 13),
    ('v1_c16_ch1', dict(AB, BLSGPU_MSM_V1='1', BLSGPU_MSM_C='16', BLSGPU_MSM_CH='1'), False, 16),
    ('naive', dict(AB, BLSGPU_MSM_NAIVE='1'), True, None),
    ('lanes64', {'BLSGPU_ACC_LANES': '64'}, True, None),
    ('msm_c16_ungated', {'BLSGPU_MSM_C': '16'}, False, None),      # tuning only: changes nothing while the first generation is off
]


def test_msm_crafted_cases_under_every_plan(tmp_path):
    """Bucket doubling / cancellation (within one part and across parts), collisions across endomorphism images, equal /
    opposite / empty neighbours of the chunk running sums, lo != 0, equal and opposite chunk partials, identity totals, all
    scalars zero, all points the identity, sub-scalar edges (z - 1, all-ones carries into the spare position, one non-zero
    sub-scalar, multiples of z^j, 0, 1, r - 1, r, 2^256 - 1), skew (4,096 copies of one point), Z != 1 and affine inputs,
    and the same below the threshold: both groups, under the second generation's plans (c = 4 .. 16, rem = 0 / 1 / W - 1,
    Q = 1 / 8, CH = 1 / max), the first generation (c = 4, 8, 13, 16), the naive path, 64 lanes, and BLSGPU_MSM_C=16
    without the A/B gate."""
    cache = {}
    for name, env, small, v1c in PLANS:
        key = (small, v1c)
        if key not in cache:
            plan_cases = []
            for group in (1, 2):
                extra = v1_cases(group, v1c) if v1c else None
                plan_cases.append((group, build_msm_cases(group, small, extra), form_cases(group)))
            cache[key] = spec_and_expect(plan_cases)
        spec, want = cache[key]
        res = run_child(tmp_path, name, env, {'msm': spec, 'secure': [], 'aggregate': []})
        got = dict(res['msm'])
        assert sorted(got) == sorted(want), name
        bad = [k for k in want if got[k] != want[k]]
        assert not bad, (name, bad)


def key_sets(sg, n):
    """name -> secret keys of the public keys: all identical, alternating pk / -pk, pk next to [z]pk and [z^2]pk."""
    s = 0x51ec + sg
    return {
        'same': [s] * n,
        'alternating': [s if i % 2 == 0 else R - s for i in range(n)],
        'endo': [(s * Z ** (i % 3)) % R for i in range(n)],
    }


def secure_cases(ns=(1024, 1500)):
    """verify_secure cases: the signature of the true aggregate (OK) and of the aggregate plus one sk * H(m) (INVALID)."""
    spec, want = [], {}
    extra = 0xbad5eed
    for sg in (1, 2):
        C = ref.G1Impl if sg == 1 else ref.G2Impl
        for n in ns:
            for name, sks in key_sets(sg, n).items():
                distinct = {s: C.pk_to_bytes(ref.public_key(C, s)) for s in set(sks)}
                perm, _, ts = ref.secure_coefficients([distinct[s] for s in sks])
                total = sum(t * sks[i] for i, t in zip(perm, ts)) % R
                key = 'sg%d/%d/%s' % (sg, n, name)
                spec.append({'name': key, 'sg': sg, 'msg': key, 'sks': sks, 'sig_sks': [total, (total + extra) % R]})
                want[key] = [0, 1]
    return spec, want


SECURE_PLANS = [
    ('default', {}),
    ('default_plain', {'BLSGPU_MSM2_TABLES': '0'}),
    ('c4', {'BLSGPU_MSM2_C': '4'}),
    ('c4_plain', {'BLSGPU_MSM2_C': '4', 'BLSGPU_MSM2_TABLES': '0'}),
    ('c16', {'BLSGPU_MSM2_C': '16'}),
    ('c16_plain', {'BLSGPU_MSM2_C': '16', 'BLSGPU_MSM2_TABLES': '0'}),
    ('sharded', {'BLSGPU_FAKE_DEVICES': '2', 'BLSGPU_SHARD_MIN': '256'}),     # the per-range sums split runs of equal keys
]


def test_verify_secure_adversarial_key_sets(tmp_path):
    """verify_secure with duplicate keys (the reference gives duplicates different coefficients, so the bucket stages see ONE
    point with many digits: the product-reachable way for a bucket accumulator to meet its next entry), keys next to their
    negatives and next to their endomorphism images; both orientations, at 1,024 and 1,500 keys, with and without the weighted
    tables, under the default plan and c = 4 / 16, and sharded over two (fake) devices.  The aggregate is ONE signature of the
    total scalar sum_i t_i sk_i (coefficients from ref.secure_coefficients), not a sum made by the library."""
    spec, want = secure_cases()
    for name, env in SECURE_PLANS:
        res = run_child(tmp_path, 'secure_' + name, env, {'msm': [], 'secure': spec, 'aggregate': []})
        got = dict(res['secure'])
        assert got == want, (name, {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v})


def test_aggregate_secure_adversarial_key_sets(tmp_path):
    """aggregate_secure (G1 signatures) at 1,024 keys alternating pk / -pk, with duplicate keys carrying DIFFERENT signatures
    (the reference takes the first match): the same point as ref.aggregate_secure."""
    n = 1024
    C = ref.G1Impl
    s = 0xa66
    sks = [s if i % 2 == 0 else R - s for i in range(n)]
    sig_sks = [sk if i < 2 else (sk + 1 + i % 3) % R for i, sk in enumerate(sks)]
    msg = b'aggregate secure, adversarial keys'
    H = C.hash_to_point(msg, C.DST[ref.BASIC])
    pk_pts = {x: ref.public_key(C, x) for x in set(sks)}
    sig_pts = {x: C.sig_curve.mul(H, x) for x in set(sig_sks)}
    want = ref.aggregate_secure(C, [pk_pts[x] for x in sks], [sig_pts[x] for x in sig_sks])
    spec = [{'name': 'alternating', 'sg': 1, 'msg': msg.decode(), 'sks': sks, 'sig_sks': sig_sks}]
    res = run_child(tmp_path, 'aggregate', {}, {'msm': [], 'secure': [], 'aggregate': spec})
    assert res['aggregate'] == [['alternating', 0, C.sig_to_bytes(want).hex()]]
