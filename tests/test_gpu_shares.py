"""Threshold recovery on the GPU (blsgpu_combine_shares; Signature::from_shares / PublicKey::from_shares).

Every point is k * g, made on the device by blsgpu_sign_batch, so the recovered point of a set is (sum_i lambda_i k_i mod r) * g:
the expected value is computed with Python integers (Lagrange at zero, or the constant term of the polynomial the shares were
cut from) and turned into a point by one more sign_batch; the two are compared as compressed bytes."""
import random

import pytest

import util
from util import c

pytestmark = pytest.mark.gpu

R = c.R
MSG = b'threshold message'


def lagrange0(xs, ks):
    """sum_i lambda_i k_i mod r, lambda_i = prod_{j != i} x_j / (x_j - x_i)."""
    tot = 0
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num = num * xj % R
                den = den * (xj - xi) % R
        tot = (tot + ks[i] * num * pow(den, R - 2, R)) % R
    return tot


def points(api, group, ks):
    """k * g of `group` for every k (0 -> the identity), RAW_PROJ."""
    nz = sorted(set(k % R for k in ks if k % R))
    got = dict(zip(nz, api.sign_batch(3 - group, api.BASIC, nz, [b''] * len(nz))[0])) if nz else {}
    ident = util.g1_raw(None) if group == 1 else util.g2_raw(None)
    return [got[k % R] if k % R else ident for k in ks]


def compressed(api, group, raws):
    return api.serialize(group, raws)


def expect_bytes(api, group, scalars):
    return compressed(api, group, points(api, group, scalars))


def poly_shares(rng, secret, t, xs):
    coeffs = [secret] + [rng.randrange(R) for _ in range(t - 1)]
    out = []
    for x in xs:
        v = 0
        for a in reversed(coeffs):
            v = (v * x + a) % R
        out.append(v)
    return out


def distinct_ids(rng, n):
    s = set()
    while len(s) < n:
        s.add(rng.randrange(1, R))
    ids = list(s)
    rng.shuffle(ids)
    return ids


@pytest.mark.parametrize('sig_group', [1, 2])
def test_shares_work(api, sig_group):
    """reference tests/signatures.rs:58-87 (shares_work), both schemes that allow share signing."""
    rng = random.Random(5 + sig_group)
    impl = api.Bls12381G1Impl if sig_group == 1 else api.Bls12381G2Impl
    sk = rng.randrange(1, R)
    ids = [1, 2, 3]
    ks = poly_shares(rng, sk, 2, ids)
    for scheme in (api.BASIC, api.POP):
        pk_sh, sig_sh = api.sign_batch(sig_group, scheme, ks, [MSG] * 3)
        pko, sigo = api.sign_batch(sig_group, scheme, [sk], [MSG])
        sshares = [api.SignatureShare(impl, scheme, ids[i], sig_sh[i]) for i in range(3)]
        pshares = [api.PublicKeyShare(impl, ids[i], pk_sh[i]) for i in range(3)]
        for s, p in zip(sshares, pshares):
            s.verify(p, MSG)
        sig = api.Signature.from_shares(sshares)
        pk = api.PublicKey.from_shares(pshares)
        assert sig.scheme == scheme
        sg, pg = sig_group, 3 - sig_group
        assert compressed(api, sg, [sig.raw]) == compressed(api, sg, sigo)
        assert compressed(api, pg, [pk.raw]) == compressed(api, pg, pko)
        sig.verify(pk, MSG)
        # any two of the three recover the same key
        pk2 = api.PublicKey.from_shares([pshares[2], pshares[0]])
        assert compressed(api, pg, [pk2.raw]) == compressed(api, pg, pko)


@pytest.mark.parametrize('sig_group', [1, 2])
def test_dash_shapes(api, sig_group):
    """255-bit identifiers: exactly t, more than t and t - 1 shares; t - 1 recovers a different signature that fails to verify."""
    rng = random.Random(40 + sig_group)
    impl = api.Bls12381G1Impl if sig_group == 1 else api.Bls12381G2Impl
    t, n = 7, 12
    sk = rng.randrange(1, R)
    ids = distinct_ids(rng, n)
    ks = poly_shares(rng, sk, t, ids)
    _, sig_sh = api.sign_batch(sig_group, api.BASIC, ks, [MSG] * n)
    pko, sigo = api.sign_batch(sig_group, api.BASIC, [sk], [MSG])
    shares = [api.SignatureShare(impl, api.BASIC, ids[i], sig_sh[i]) for i in range(n)]
    pk = api.PublicKey(impl, pko[0])
    for cnt in (t, n):
        sig = api.Signature.from_shares(shares[:cnt])
        assert compressed(api, sig_group, [sig.raw]) == compressed(api, sig_group, sigo)
        sig.verify(pk, MSG)
    bad = api.Signature.from_shares(shares[:t - 1])
    assert compressed(api, sig_group, [bad.raw]) != compressed(api, sig_group, sigo)
    with pytest.raises(api.BlsError) as e:
        bad.verify(pk, MSG)
    assert e.value.kind == 'InvalidSignature'


SIZES = [0, 1, 2, 3, 17, 63, 64, 65, 240, 400, 1000]


@pytest.mark.parametrize('group', [1, 2])
def test_ragged_sets_one_call(api, group):
    rng = random.Random(77 + group)
    sets, expect = [], []
    for t in SIZES:
        ids = distinct_ids(rng, t)
        if t <= 65:
            ks = [rng.randrange(R) for _ in range(t)]
            want = lagrange0(ids, ks) if t >= 2 else None
        else:                                   # the constant term of a polynomial of degree < t through the shares
            secret = rng.randrange(R)
            ks = poly_shares(rng, secret, min(t, 9), ids)
            want = secret
        sets.append(list(zip(ids, points(api, group, ks), [None] * t)))
        expect.append(want)
    out, st = api.combine_shares(group, sets)
    zero = bytes(144 if group == 1 else 288)
    for s, t in enumerate(SIZES):
        if t < 2:
            assert st[s] == api.VSSS_ERROR and out[s] == zero, (t, st[s])
        else:
            assert st[s] == api.OK, (t, st[s])
            assert compressed(api, group, [out[s]]) == expect_bytes(api, group, [expect[s]]), t
    out2, st2 = api.combine_shares(group, sets)
    assert (out2, st2) == (out, st)                  # deterministic bytes


def test_affine_input_matches(api):
    rng = random.Random(3)
    for group in (1, 2):
        ids = distinct_ids(rng, 5)
        ks = [rng.randrange(1, R) for _ in range(5)]
        proj = points(api, group, ks)
        pts, sts = api.deserialize(group, api.serialize(group, proj))     # decompressed points carry Z = 1
        assert all(s == 0 for s in sts)
        half = 96 if group == 1 else 192
        aff = [p[:half] for p in pts]                # Z = 1: x, y are the affine coordinates
        o1, s1 = api.combine_shares(group, [list(zip(ids, proj, [None] * 5))])
        o2, s2 = api.combine_shares(group, [list(zip(ids, aff, [None] * 5))], fmt=api.FMT_RAW_AFFINE)
        assert s1 == s2 == [0]
        assert o1 == o2
        assert compressed(api, group, o1) == expect_bytes(api, group, [lagrange0(ids, ks)])


@pytest.mark.parametrize('group', [1, 2])
def test_errors_interleaved(api, group):
    rng = random.Random(900 + group)
    zero = bytes(144 if group == 1 else 288)

    def good(t):
        ids = distinct_ids(rng, t)
        ks = [rng.randrange(1, R) for _ in range(t)]
        return ids, ks

    cases = []                 # (ids, ks, schemes, expected status)
    ids, ks = good(4)
    cases.append((ids, ks, [2] * 4, api.OK))
    ids, ks = good(4)
    ids[2] = 0
    cases.append((ids, ks, [2] * 4, api.VSSS_ERROR))                 # a zero identifier
    ids, ks = good(5)
    cases.append((ids, ks, [0] * 5, api.OK))
    ids, ks = good(5)
    ids[3] = ids[2]
    cases.append((ids, ks, [2] * 5, api.VSSS_ERROR))                 # duplicates, adjacent
    ids, ks = good(300)
    ids[299] = ids[1]
    cases.append((ids, ks, [2] * 300, api.VSSS_ERROR))               # duplicates, far apart in a large set
    ids, ks = good(3)
    ids[1] = R
    cases.append((ids, ks, [2] * 3, api.BAD_ENCODING))               # identifier == r
    ids, ks = good(3)
    ids[0] = 2 ** 256 - 1
    ids[1] = 0                                                       # encoding wins over the zero identifier
    cases.append((ids, ks, [2] * 3, api.BAD_ENCODING))
    ids, ks = good(4)
    cases.append((ids, ks, [2, 2, 0, 2], api.INVALID_SCHEME))       # mixed tags
    ids, ks = good(4)
    ids[3] = ids[0]
    cases.append((ids, ks, [1, 2, 2, 2], api.INVALID_SCHEME))       # scheme before vsss
    ids, ks = good(1)
    cases.append((ids, ks, [2], api.VSSS_ERROR))
    ids, ks = good(66)
    cases.append((ids, ks, [1] * 66, api.OK))
    sets = [list(zip(ids, points(api, group, ks), sch)) for ids, ks, sch, _ in cases]
    out, st = api.combine_shares(group, sets)
    assert st == [cs[3] for cs in cases]
    for s, (ids, ks, _, want) in enumerate(cases):
        if want == api.OK:
            assert compressed(api, group, [out[s]]) == expect_bytes(api, group, [lagrange0(ids, ks)])
        else:
            assert out[s] == zero
    # schemes = NULL: no scheme check, the same good sets recover the same points
    nsets = [[(x, p, None) for x, p, _ in st_] for st_ in sets]
    out2, st2 = api.combine_shares(group, nsets)
    want2 = [cs[3] for cs in cases]
    want2[7], want2[8] = api.OK, api.VSSS_ERROR      # without tags: the mixed set recovers, the one with a duplicate fails in vsss
    assert st2 == want2
    for s in range(len(cases)):
        if st[s] == api.OK:
            assert out2[s] == out[s]


@pytest.mark.parametrize('group', [1, 2])
def test_exceptional_sums(api, group):
    rng = random.Random(1234 + group)
    ident = util.g1_raw(None) if group == 1 else util.g2_raw(None)
    zero = bytes(144 if group == 1 else 288)
    x1, x2 = distinct_ids(rng, 2)
    l1 = x2 * pow(x2 - x1, R - 2, R) % R           # lambda_1 = x2 / (x2 - x1)
    l2 = x1 * pow(x1 - x2, R - 2, R) % R
    a = rng.randrange(1, R)
    # lambda1 k1 = lambda2 k2 = a: a doubling inside the sum
    k1, k2 = a * pow(l1, R - 2, R) % R, a * pow(l2, R - 2, R) % R
    # lambda1 k1 = -lambda2 k2: the identity
    m1, m2 = a * pow(l1, R - 2, R) % R, (R - a) * pow(l2, R - 2, R) % R
    sets = [list(zip([x1, x2], points(api, group, [k1, k2]), [None] * 2)),
            list(zip([x1, x2], points(api, group, [m1, m2]), [None] * 2)),
            [(x1, ident, None), (x2, points(api, group, [k2])[0], None)],
            [(x1, ident, None), (x2, ident, None)]]
    out, st = api.combine_shares(group, sets)
    assert st == [0, 0, 0, 0]
    assert compressed(api, group, [out[0]]) == expect_bytes(api, group, [2 * a % R])
    assert out[1] == zero
    assert compressed(api, group, [out[2]]) == expect_bytes(api, group, [a])
    assert out[3] == zero


@pytest.mark.parametrize('sig_group', [1, 2])
def test_device_resident_into_verify(api, sig_group):
    """TensorOps: shares on the device, recovered signatures stay there and go straight into verify_batch."""
    import torch
    rng = random.Random(50 + sig_group)
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    n_sets, t = 6, 5
    sks = [rng.randrange(1, R) for _ in range(n_sets)]
    pks, _ = api.sign_batch(sig_group, api.POP, sks, [MSG] * n_sets)
    ids_all, ks_all = [], []
    for s in range(n_sets):
        ids = distinct_ids(rng, t)
        ids_all += ids
        ks_all += poly_shares(rng, sks[s], 3, ids)
    _, sig_sh = api.sign_batch(sig_group, api.POP, ks_all, [MSG] * len(ks_all))
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    ids_t = tens(b''.join(x.to_bytes(32, 'little') for x in ids_all))
    pts_t = tens(b''.join(sig_sh))
    sch_t = tens(bytes([api.POP] * len(ks_all)))
    offs_t = torch.tensor([t * s for s in range(n_sets + 1)], dtype=torch.int64, device=dev)
    sigs_t, st = ops.combine_shares(sig_group, ids_t, pts_t, sch_t, offs_t, n_sets)
    assert st.cpu().tolist() == [0] * n_sets
    pks_t = tens(b''.join(pks))
    msgs = [MSG] * n_sets
    offs, blob = api._offsets(msgs)
    msgs_t = tens(blob)
    moffs_t = torch.tensor(list(offs), dtype=torch.int64, device=dev)
    vst = ops.verify_batch(sig_group, api.POP, pks_t, sigs_t, msgs_t, moffs_t, n_sets)
    assert vst.cpu().tolist() == [0] * n_sets


@pytest.mark.parametrize('group', [1, 2])
def test_one_large_set(api, group):
    """65,536 shares of a degree-2 polynomial in one set; twice, byte-identical."""
    rng = random.Random(65536 + group)
    t = 65536
    ids = distinct_ids(rng, t)
    secret = rng.randrange(1, R)
    ks = poly_shares(rng, secret, 3, ids)
    sets = [list(zip(ids, points(api, group, ks), [None] * t))]
    out, st = api.combine_shares(group, sets)
    assert st == [0]
    assert compressed(api, group, out) == expect_bytes(api, group, [secret])
    out2, st2 = api.combine_shares(group, sets)
    assert (out2, st2) == (out, st)


def test_every_plan_same_bytes(api):
    """Every plan gives the same bytes: per-share ladders for every set, the bucket MSM for every set of two or more shares, and
    the default split (BLSGPU_SHARES_MSM_MIN), each in a child process (tests/shares_worker.py)."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for v in ('2', '64', '1024', '4294967296'):
        env = dict(os.environ, BLSGPU_SHARES_MSM_MIN=v)
        p = subprocess.run([sys.executable, os.path.join(here, 'shares_worker.py')], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        got[v] = json.loads(p.stdout.strip().splitlines()[-1])
    first = got['2']
    for v, r in got.items():
        assert r == first, v
    for g in ('1', '2'):
        st = first[g][0]
        assert st == [api.VSSS_ERROR] * 2 + [api.OK] * 9 + [api.VSSS_ERROR] * 2
