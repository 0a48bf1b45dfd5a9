"""Batched verify_secure on the GPU (blsgpu_verify_secure_batch; Signature::verify_secure / verify_secure_with_mode for many
independent sets).  Expected verdicts come from the coefficients derived in plain Python (tests/secure_coeffs.py) and from the
single call, blsgpu_verify_secure, run on each set alone."""
import json
import os
import random
import subprocess
import sys

import pytest

import util
from secure_batch_cases import identity, mixed_sets, valid_sets

pytestmark = pytest.mark.gpu

KATS = json.load(open(os.path.join(util.ROOT, 'tests', 'golden', 'ref_kats.json')))
SIZES = [0, 1, 2, 3, 57, 200, 600, 1100]       # 1,100: above the default BLSGPU_SECURE_BATCH_MAX


@pytest.mark.parametrize('sg,scheme,legacy', [(1, 0, False), (1, 1, False), (1, 2, False), (2, 0, False), (2, 1, False), (2, 2, False), (2, 0, True)],
                         ids=['g1-basic', 'g1-aug', 'g1-pop', 'g2-basic', 'g2-aug', 'g2-pop', 'g2-basic-legacy'])
def test_closed_form_valid_sets(api, sg, scheme, legacy):
    """sk = sum t_i k_i mod r with t_i from Python's sorted() and hashlib: every ragged set verifies."""
    rng = random.Random(100 * sg + 10 * scheme + legacy)
    sets = valid_sets(api, sg, scheme, SIZES, rng, legacy=legacy)
    st = api.verify_secure_batch(sg, scheme, [s[:3] for s in sets], api.LEGACY if legacy else api.MODERN)
    assert st == [api.OK] * len(SIZES)
    # Bls12381G2Impl: the same sets under the other key serialisation must all fail, except the empty one
    if sg == 2:
        st = api.verify_secure_batch(sg, scheme, [s[:3] for s in sets], api.MODERN if legacy else api.LEGACY)
        assert st == [api.OK] + [api.INVALID_SIGNATURE] * (len(SIZES) - 1)


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('scheme', [0, 1])
def test_equals_single_call(api, sg, scheme):
    sets = mixed_sets(api, sg, scheme, 20 + sg + 2 * scheme)
    got = api.verify_secure_batch(sg, scheme, sets)
    want = [api.verify_secure(sg, scheme, pks, sig, msg) for pks, sig, msg in sets]
    assert got == want
    assert want[0] == api.OK and want[1] == api.INVALID_SIGNATURE and want[7] == api.OK and want[8] == api.INVALID_SIGNATURE
    assert want[4] == api.OK and want[5] == api.OK and want[6] == api.INVALID_SIGNATURE
    assert len(set(want)) >= 3                              # identity checks give statuses of their own


@pytest.mark.parametrize('sg', [1, 2])
def test_affine_signatures(api, sg):
    """fmt = RAW_AFFINE for keys and signatures (decompressed points carry Z = 1; the identity is all-zero)."""
    sets = mixed_sets(api, sg, 0, 40 + sg)
    half = {1: 96, 2: 192}

    def aff(group, raws):
        if not raws:
            return []
        pts, sts = api.deserialize(group, api.serialize(group, raws))
        return [bytes(half[group]) if r == identity(group) else p[:half[group]] for r, p in zip(raws, pts)]

    asets = [(aff(3 - sg, pks), aff(sg, [sig])[0], msg) for pks, sig, msg in sets]
    got = api.verify_secure_batch(sg, 0, asets, fmt=api.FMT_RAW_AFFINE)
    want = [api.verify_secure(sg, 0, pks, sig, msg) for pks, sig, msg in sets]
    assert got == want
    assert got == [api.verify_secure(sg, 0, pks, sig, msg, fmt=api.FMT_RAW_AFFINE) for pks, sig, msg in asets]


def test_reference_kat_in_a_batch(api):
    """The 57-key production vector (reference tests/secure_aggregation_test.rs:143-235) in the middle of other sets."""
    C = util.ref.G2Impl
    p57 = KATS['prod57']
    pks = [util.g1_raw(C.pk_from_bytes(bytes.fromhex(h))) for h in p57['pks']]
    sig = util.g2_raw(C.sig_from_bytes(bytes.fromhex(p57['sig'])))
    msg = bytes.fromhex(p57['message'])
    others = [s[:3] for s in valid_sets(api, 2, 0, [3, 30, 0, 90], random.Random(57))]
    sets = others[:2] + [(pks, sig, msg), (pks[:-1], sig, msg)] + others[2:]
    assert api.verify_secure_batch(2, 0, sets) == [0, 0, 0, api.INVALID_SIGNATURE, 0, 0]


def test_every_plan_same_statuses(api):
    """BLSGPU_SECURE_BATCH_MAX = 1 (every non-empty set one at a time), 64, the default and 2^32 (every set on the batched
    kernels) give the same statuses, each in a child process (tests/secure_batch_worker.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for v in ('1', '64', '1024', '4294967296'):
        env = dict(os.environ, BLSGPU_SECURE_BATCH_MAX=v)
        p = subprocess.run([sys.executable, os.path.join(here, 'secure_batch_worker.py')], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got[v] = json.loads(p.stdout.strip().splitlines()[-1])
    for v, r in got.items():
        assert r == got['1024'], v
    for sg in ('1', '2'):
        st = got['1024'][sg]
        assert st[0] == 0 and st[4] == 0 and st[5] == 0 and st[7] == 0 and st[-2] == 0
        assert st[1] == st[-1] == api.INVALID_SIGNATURE


@pytest.mark.parametrize('sg', [1, 2])
def test_device_resident(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sets = mixed_sets(api, sg, 2, 60 + sg)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    koffs = [0]
    for pks, _, _ in sets:
        koffs.append(koffs[-1] + len(pks))
    moffs, mblob = api._offsets([m for _, _, m in sets])
    st = ops.verify_secure_batch(sg, 2, tens(b''.join(p for pks, _, _ in sets for p in pks)), torch.tensor(koffs, dtype=torch.int64, device=dev),
                                 tens(b''.join(s for _, s, _ in sets)), tens(mblob), torch.tensor(list(moffs), dtype=torch.int64, device=dev), len(sets))
    assert st.device == dev and st.dtype == torch.int32
    assert st.cpu().tolist() == api.verify_secure_batch(sg, 2, sets)


def test_verify_secure_many(api, pkg):
    impl = pkg.Bls12381G2Impl
    rng = random.Random(5)
    items = []
    for scheme in (0, 2, 1, 0):
        (pks, sig, msg, _), = valid_sets(api, 2, scheme, [6], rng, tag=b'%d' % scheme)
        items.append((pkg.Signature(impl, scheme, sig), [pkg.PublicKey(impl, p) for p in pks], msg))
    items.append((items[0][0], items[0][1][1:], items[0][2]))
    got = pkg.verify_secure_many(items)
    assert got == [None] * 4 + [pkg.BlsError('InvalidSignature')]
    assert pkg.verify_secure_many([]) == []


def test_argument_checks(api):
    import ctypes
    lib = api.init()
    sets = [s[:3] for s in valid_sets(api, 2, 0, [2, 3], random.Random(9))]
    pkb = b''.join(p for pks, _, _ in sets for p in pks)
    sgb = b''.join(s for _, s, _ in sets)
    moffs, mblob = api._offsets([m for _, _, m in sets])
    st = (ctypes.c_int32 * 2)()

    def call(sg, koffs, n_sets=2, ser=0, fmt=0):
        ko = (ctypes.c_uint64 * len(koffs))(*koffs)
        return lib.blsgpu_verify_secure_batch(sg, 0, api._ptr(pkb), ctypes.cast(ko, ctypes.c_void_p), n_sets, api._ptr(sgb), api._ptr(mblob),
                                              ctypes.cast(moffs, ctypes.c_void_p), ser, fmt, ctypes.cast(st, ctypes.c_void_p))

    E_ARG = -3
    assert call(2, [0, 2, 5]) == 0 and list(st) == [0, 0]
    assert call(2, [0, 3, 2]) == E_ARG                     # decreasing
    assert call(2, [1, 2, 5]) == E_ARG                     # first offset not 0
    assert call(1, [0, 2, 5], ser=1) == E_ARG              # Legacy with Bls12381G1Impl
    assert call(2, [0, 2, 5], fmt=api.FMT_COMPRESSED) == E_ARG
    assert call(2, [0], n_sets=0) == 0
