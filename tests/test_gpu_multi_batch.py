"""Batched multi verify on the GPU (blsgpu_multi_verify_batch; MultiSignature::verify for many independent sets).  Expected
verdicts come from closed-form valid sets (the signature of a set is made for the sum of its secrets) and from the single call,
blsgpu_multi_verify, run on each set alone."""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

from multi_batch_cases import MIXED_EXPECT, identity, mixed_sets, valid_sets

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 63, 64, 65, 130, 300]      # at and around a workgroup of 64 lanes; several strips per set from 8 keys on
COMBOS = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
COMBO_IDS = ['g1-basic', 'g1-aug', 'g1-pop', 'g2-basic', 'g2-aug', 'g2-pop']


@pytest.mark.parametrize('sg,scheme', COMBOS, ids=COMBO_IDS)
def test_closed_form_valid_sets(api, sg, scheme):
    """sk = sum k_i mod r: every ragged set verifies; the empty one has no key (its signature here is the identity, which
    core_verify looks at first).  With one key dropped nothing verifies: a set that is left without keys sums to the identity key."""
    sets = valid_sets(api, sg, scheme, SIZES, random.Random(100 * sg + scheme))
    st = api.multi_verify_batch(sg, scheme, [s[:3] for s in sets])
    assert st == [api.SIG_IDENTITY] + [api.OK] * (len(SIZES) - 1)
    st = api.multi_verify_batch(sg, scheme, [(pks[:len(pks) // 2] + pks[len(pks) // 2 + 1:], sig, msg) for pks, sig, msg, _ in sets])
    assert st == [api.SIG_IDENTITY, api.PK_IDENTITY] + [api.INVALID_SIGNATURE] * (len(SIZES) - 2)


@pytest.mark.parametrize('sg,scheme', COMBOS, ids=COMBO_IDS)
def test_equals_single_call(api, sg, scheme):
    sets = mixed_sets(api, sg, scheme, 20 + sg + 2 * scheme)
    got = api.multi_verify_batch(sg, scheme, sets)
    want = [api.multi_verify(sg, scheme, pks, sig, msg) for pks, sig, msg in sets]
    print('batch', got, 'single', want)
    assert got == want
    assert want == MIXED_EXPECT
    assert len(set(want)) >= 4                              # both identity checks give statuses of their own


def test_every_plan_same_statuses(api):
    """BLSGPU_MULTI_STRIP = 1 (one strip per key: every addition happens in the fold), 2, 3, 64, 2^32 (one strip per set: none
    does) and unset give the same statuses, each in a child process (tests/multi_batch_worker.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for v in ('1', '2', '3', '64', '4294967296', None):       # one after another: a child that fails ends the test before the next starts
        env = {k: x for k, x in os.environ.items() if k != 'BLSGPU_MULTI_STRIP'}
        if v is not None:
            env['BLSGPU_MULTI_STRIP'] = v
        p = subprocess.run([sys.executable, os.path.join(here, 'multi_batch_worker.py')], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        got[v] = json.loads(p.stdout.strip().splitlines()[-1])
    for v, r in got.items():
        assert r == got[None], v
    for sg in ('1', '2'):
        assert got[None][sg] == MIXED_EXPECT + [api.OK] * 4      # [P, P] (position 6) verifies under every plan


@pytest.mark.parametrize('sg', [1, 2])
def test_affine_input(api, sg):
    """fmt = RAW_AFFINE for keys and signatures (decompressed points carry Z = 1; the identity is all-zero)."""
    sets = mixed_sets(api, sg, 0, 40 + sg, sizes=(65,))
    half = {1: 96, 2: 192}

    def aff(group, raws):
        if not raws:
            return []
        pts, sts = api.deserialize(group, api.serialize(group, raws))
        return [bytes(half[group]) if r == identity(group) else p[:half[group]] for r, p in zip(raws, pts)]

    asets = [(aff(3 - sg, pks), aff(sg, [sig])[0], msg) for pks, sig, msg in sets]
    got = api.multi_verify_batch(sg, 0, asets, fmt=api.FMT_RAW_AFFINE)
    assert got == api.multi_verify_batch(sg, 0, sets) == MIXED_EXPECT + [api.OK]


@pytest.mark.parametrize('sg', [1, 2])
def test_device_resident_and_chained(api, sg):
    """Device tensors in, a device tensor out; the keys come straight from blsgpu_deserialize's device output."""
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sets = mixed_sets(api, sg, 2, 60 + sg, sizes=(64,))
    want = api.multi_verify_batch(sg, 2, sets)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    koffs = [0]
    for pks, _, _ in sets:
        koffs.append(koffs[-1] + len(pks))
    moffs, mblob = api._offsets([m for _, _, m in sets])
    args = (tens(b''.join(s for _, s, _ in sets)), tens(mblob), torch.tensor(list(moffs), dtype=torch.int64, device=dev), len(sets))
    koffs_t = torch.tensor(koffs, dtype=torch.int64, device=dev)
    allk = [p for pks, _, _ in sets for p in pks]
    st = ops.multi_verify_batch(sg, 2, tens(b''.join(allk)), koffs_t, *args)
    assert st.device == dev and st.dtype == torch.int32
    assert st.cpu().tolist() == want == MIXED_EXPECT + [api.OK]
    # compressed bytes -> blsgpu_deserialize on the device -> the batch, no host copy in between
    g, n = 3 - sg, len(allk)
    comp = tens(b''.join(api.serialize(g, allk)))
    pts, dst = ops.empty(n * (144 if g == 1 else 288)), ops.empty(n, torch.int32)
    torch.cuda.synchronize()
    api._check(ops.lib.blsgpu_deserialize(g, ops._p(comp), n, api.FMT_COMPRESSED, ops._p(pts), ops._p(dst)))
    assert dst.cpu().tolist() == [0] * n
    assert ops.multi_verify_batch(sg, 2, pts, koffs_t, *args).cpu().tolist() == want


def test_multi_verify_many(api, pkg):
    impl = pkg.Bls12381G2Impl
    rng = random.Random(5)
    items = []
    for scheme in (0, 2, 1, 0):
        (pks, sig, msg, _), = valid_sets(api, 2, scheme, [6], rng, tag=b'%d' % scheme)
        items.append((pkg.MultiSignature(impl, scheme, sig), pkg.MultiPublicKey.from_public_keys([pkg.PublicKey(impl, p) for p in pks]), msg))
    items.append((items[0][0], pkg.MultiPublicKey(impl, items[0][1].keys[1:]), items[0][2]))
    assert pkg.multi_verify_many(items) == [None] * 4 + [pkg.BlsError('InvalidSignature')]
    assert pkg.multi_verify_many([]) == []
    (pks, sig, msg, _), = valid_sets(api, 1, 0, [2], rng)
    other = (pkg.MultiSignature(pkg.Bls12381G1Impl, 0, sig), pkg.MultiPublicKey(pkg.Bls12381G1Impl, [pkg.PublicKey(pkg.Bls12381G1Impl, p) for p in pks]), msg)
    with pytest.raises(ValueError):
        pkg.multi_verify_many([items[0], other])


def test_argument_checks(api):
    lib = api.init()
    sets = [s[:3] for s in valid_sets(api, 2, 0, [2, 3], random.Random(9))]
    pkb = b''.join(p for pks, _, _ in sets for p in pks)
    sgb = b''.join(s for _, s, _ in sets)
    moffs, mblob = api._offsets([m for _, _, m in sets])
    st = (ctypes.c_int32 * 2)(-99, -99)

    def call(koffs, n_sets=2, fmt=0):
        ko = (ctypes.c_uint64 * len(koffs))(*koffs)
        return lib.blsgpu_multi_verify_batch(2, 0, api._ptr(pkb), ctypes.cast(ko, ctypes.c_void_p), n_sets, api._ptr(sgb), api._ptr(mblob),
                                             ctypes.cast(moffs, ctypes.c_void_p), fmt, ctypes.cast(st, ctypes.c_void_p))

    E_ARG = -3
    assert call([0, 2, 5]) == 0 and list(st) == [0, 0]
    assert call([0, 3, 2]) == E_ARG                     # decreasing
    assert call([1, 2, 5]) == E_ARG                     # first offset not 0
    assert call([0, 2, 5], fmt=api.FMT_COMPRESSED) == E_ARG
    assert call([0], n_sets=0) == 0
    # one set alone is the single call
    for pks, sig, msg in sets + [(sets[0][0][:1], sets[0][1], sets[0][2]), ([], sets[0][1], b''), ([], identity(2), b'm')]:
        assert api.multi_verify_batch(2, 0, [(pks, sig, msg)]) == [api.multi_verify(2, 0, pks, sig, msg)]
