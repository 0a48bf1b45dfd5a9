"""Batched aggregate verify on the GPU (blsgpu_aggregate_verify_batch; AggregateSignature::verify for many independent sets).
Expected results come from the case list (tests/agg_batch_cases.py, checked against the oracle by tests/test_agg_batch_cases.py),
from the single call, blsgpu_aggregate_verify, run on each set alone, and from sets that are valid or tampered by construction."""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

import agg_batch_cases as abc

pytestmark = pytest.mark.gpu

COMBOS = [(sg, scheme) for sg in (1, 2) for scheme in (0, 1, 2)]
IDS = ['g%d-%s' % (sg, ('basic', 'aug', 'pop')[scheme]) for sg, scheme in COMBOS]


@pytest.mark.parametrize('sg,scheme', COMBOS, ids=IDS)
def test_case_list(api, sg, scheme):
    cl = abc.cases(sg, scheme)
    got = api.aggregate_verify_batch(sg, scheme, abc.raw_sets(sg, cl, random.Random(10 * sg + scheme)))
    for (name, _, _, want), g in zip(cl, got):
        assert g == want, name
    assert len(got) == len(cl)


@pytest.mark.parametrize('sg,scheme', COMBOS, ids=IDS)
def test_equals_single_call(api, sg, scheme):
    cl = abc.cases(sg, scheme)
    sets = abc.raw_sets(sg, cl, random.Random(77))
    got = api.aggregate_verify_batch(sg, scheme, sets)
    want = [api.aggregate_verify(sg, scheme, pks, msgs, sig) for pks, msgs, sig in sets]
    assert got == want
    assert len({st for st, _ in want}) >= 4


@pytest.mark.parametrize('sg', [1, 2])
def test_affine_points(api, sg):
    """fmt = RAW_AFFINE for keys and signatures (Z = 1 dropped; the identity is all-zero)."""
    cl = abc.cases(sg, 0)
    sets = abc.raw_sets(sg, cl)                       # Z = 1: the affine form is the first two coordinates
    half = {1: 96, 2: 192}
    ident = {g: abc.raw_sets(g, [('', [], None, None)])[0][2] for g in (1, 2)}      # the identity signature of impl g lives in group g

    def aff(group, raw):
        return bytes(half[group]) if raw == ident[group] else raw[:half[group]]

    asets = [([aff(3 - sg, p) for p in pks], msgs, aff(sg, sig)) for pks, msgs, sig in sets]
    got = api.aggregate_verify_batch(sg, 0, asets, fmt=api.FMT_RAW_AFFINE)
    assert got == [want for _, _, _, want in cl]
    assert got[:12] == [api.aggregate_verify(sg, 0, pks, msgs, sig, fmt=api.FMT_RAW_AFFINE) for pks, msgs, sig in asets[:12]]


def test_every_plan_same_output(api):
    """BLSGPU_AGG_BATCH_MAX = 1 (every non-empty set one at a time), 64, 4096, the default (32,768) and 2^32 (every set on the batched
    kernels) give the same statuses and aux, each in a child process (tests/agg_batch_worker.py), with one set above the default in the list."""
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    for v in ('1', '64', '4096', '4294967296'):
        env = dict(os.environ, BLSGPU_AGG_BATCH_MAX=v)
        p = subprocess.run([sys.executable, os.path.join(here, 'agg_batch_worker.py')], env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        got[v] = json.loads(p.stdout.strip().splitlines()[-1])
    env = dict(os.environ)
    env.pop('BLSGPU_AGG_BATCH_MAX', None)
    p = subprocess.run([sys.executable, os.path.join(here, 'agg_batch_worker.py')], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    got['default'] = json.loads(p.stdout.strip().splitlines()[-1])
    for sg, scheme in ((1, 0), (2, 0), (1, 1), (2, 2)):      # agg_batch_worker.RUNS: Aug and PoP take the one-at-a-time path without a duplicate record
        want = [[st, a0, a1] for _, _, _, (st, (a0, a1)) in abc.cases(sg, scheme)]
        want = want[:5] + [[api.OK, 0, 0]] + want[5:] + [[api.INVALID_SIGNATURE, 0, 0]]
        for v, r in got.items():
            assert r['%d-%d' % (sg, scheme)] == want, (v, sg, scheme)


@pytest.mark.parametrize('sg', [1, 2])
def test_device_resident(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    cl = abc.cases(sg, 0)
    sets = abc.raw_sets(sg, cl, random.Random(3))
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    soffs = [0]
    for pks, _, _ in sets:
        soffs.append(soffs[-1] + len(pks))
    moffs, mblob = api._offsets([m for _, msgs, _ in sets for m in msgs])
    st, aux = ops.aggregate_verify_batch(sg, 0, tens(b''.join(p for pks, _, _ in sets for p in pks)), tens(mblob),
                                         torch.tensor(list(moffs), dtype=torch.int64, device=dev), torch.tensor(soffs, dtype=torch.int64, device=dev),
                                         len(sets), tens(b''.join(s for _, _, s in sets)))
    assert st.device == dev and st.dtype == torch.int32 and aux.device == dev and aux.shape == (len(sets), 2)
    host = api.aggregate_verify_batch(sg, 0, sets)
    assert [(s, (a, b)) for s, (a, b) in zip(st.cpu().tolist(), aux.cpu().tolist())] == host
    assert host == [want for _, _, _, want in cl]


@pytest.mark.parametrize('sg', [1, 2])
def test_large_ragged_call(api, sg):
    """1,100 sets of 64 pairs: 71,500 items, more than one machine round of lane pairs plus its remainder.  Keys and signatures
    are made on the device (sign_batch), every set's aggregate by point_sum; every 97th set has one message changed afterwards."""
    n_sets, size = 1100, 64
    rng = random.Random(1100 + sg)
    msgs = [b'large %d %d' % (s, i) for s in range(n_sets) for i in range(size)]
    pks, sigs = api.sign_batch(sg, api.BASIC, [rng.randrange(1, 2 ** 200) for _ in msgs], msgs)
    sets = []
    for s in range(n_sets):
        m = msgs[s * size:(s + 1) * size]
        if s % 97 == 0:
            k = rng.randrange(size)
            m = m[:k] + [m[k] + b'?'] + m[k + 1:]
        sets.append((pks[s * size:(s + 1) * size], m, api.point_sum(sg, sigs[s * size:(s + 1) * size])))
    got = api.aggregate_verify_batch(sg, api.BASIC, sets)
    assert got == [(api.INVALID_SIGNATURE if s % 97 == 0 else api.OK, (0, 0)) for s in range(n_sets)]
    for s in (0, 1, 96, 97, 98, 1023, 1067, 1099):       # 1023 and 1067: sets at the end of the first round of items and inside the second
        assert got[s] == api.aggregate_verify(sg, api.BASIC, *sets[s]), s


def test_aggregate_verify_many(api, pkg):
    impl = pkg.Bls12381G1Impl
    items, want = [], []
    for scheme in (0, 2, 1):
        cl = abc.cases(1, scheme)
        for (name, pairs, _, (st, aux)), (pks, msgs, sig) in zip(cl, abc.raw_sets(1, cl)):
            if len(pairs) > abc.ORACLE_MAX_PAIRS:
                continue
            items.append((pkg.AggregateSignature(impl, scheme, sig), [(pkg.PublicKey(impl, p), m) for p, m in zip(pks, msgs)]))
            want.append(pkg.error_from_status(st, aux, aggregate=True))
    got = pkg.aggregate_verify_many(items)
    assert got == want
    assert pkg.BlsError('InvalidInputs', 'duplicate messages detected at 1 and 3') in got
    assert pkg.BlsError('InvalidInputs', 'public key at 2 is the identity point') in got
    assert pkg.BlsError('InvalidInputs', 'signature is the identity point') in got and pkg.BlsError('InvalidSignature') in got and None in got
    for (sig, data), w in list(zip(items, want))[:20]:      # the very errors AggregateSignature.verify raises
        try:
            sig.verify(data)
            e = None
        except pkg.BlsError as err:
            e = err
        assert e == w
    assert pkg.aggregate_verify_many([]) == []


def test_argument_checks(api):
    lib = api.init()
    cl = abc.cases(2, 0)[:2]
    sets = abc.raw_sets(2, cl)
    pkb = b''.join(p for pks, _, _ in sets for p in pks)
    sgb = b''.join(s for _, _, s in sets)
    moffs, mblob = api._offsets([m for _, msgs, _ in sets for m in msgs])
    st = (ctypes.c_int32 * 2)()
    aux = (ctypes.c_uint64 * 4)()

    def call(soffs, n_sets=2, fmt=0, with_aux=True):
        so = (ctypes.c_uint64 * len(soffs))(*soffs)
        return lib.blsgpu_aggregate_verify_batch(2, 0, api._ptr(pkb), api._ptr(mblob), ctypes.cast(moffs, ctypes.c_void_p), ctypes.cast(so, ctypes.c_void_p),
                                                 n_sets, api._ptr(sgb), fmt, ctypes.cast(st, ctypes.c_void_p),
                                                 ctypes.cast(aux, ctypes.c_void_p) if with_aux else None)

    E_ARG = -3
    assert call([0, 3, 6]) == 0 and list(st) == [api.OK, api.INVALID_SIGNATURE] and list(aux) == [0, 0, 0, 0]
    st[0] = st[1] = -9
    assert call([0, 3, 6], with_aux=False) == 0 and list(st) == [api.OK, api.INVALID_SIGNATURE]      # aux may be NULL
    assert call([0, 4, 3]) == E_ARG                        # decreasing
    assert call([1, 3, 6]) == E_ARG                        # first offset not 0
    assert call([0, 3, 6], fmt=api.FMT_COMPRESSED) == E_ARG   # a wire format
    assert call([0], n_sets=0) == 0
