"""The doors that share run_pairing2 -- sig_proof_verify_batch, pop_verify_batch, signcrypt_valid_batch, core_verify,
core_verify_hashed, pairing2_check_batch -- on every pairing path, both orientations and both raw input formats.

The items and the result the reference gives each of them come from tests/pairing_door_cases.py (the oracle;
tests/test_pairing_door_cases.py checks the list on the CPU); every comparison is exact equality of result vectors.  Between them
the runs send fixed_g2 = 1 (sig_proof and core_verify_hashed in sig_group 1: the plain -g2 line tables), fixed_g2 = 2 (pop,
signcrypt, core_verify in sig_group 1) and fixed_g2 = 0 (sig_group 2, pairing2) through the row-wide engine, the wave-cooperative
kernel, the lane-split kernels, the first-generation kernels and the segmented final exponentiation, with failing items -- among them
items whose prepare kernel leaves the pair slots unwritten -- next to valid ones at item 0, item n - 1 and on both sides of every
32-item boundary.  Runs that need their own process (knobs are read once; one context) go through tests/pairing_door_worker.py."""
import json
import os
import pickle
import subprocess
import sys

import pytest
import pairing_door_cases as d
import util
from oracle.py import blsful_ref as ref
from pairing_door_worker import call_door
from test_gpu_wire import PLANS as WIRE_PLANS

pytestmark = pytest.mark.gpu

FMT_IDS = {d.RAW_PROJ: 'proj', d.RAW_AFFINE: 'affine'}
# (door, sg, fmt) of every door, orientation and input format the door takes
DOOR_SG_FMT = [(door, sg, fmt) for door in d.DOORS for sg in ((0,) if door == 'pairing2' else (1, 2))
               for fmt in ((d.RAW_PROJ, d.RAW_AFFINE) if door in d.HAS_FMT else (d.RAW_PROJ,))]
DOOR_SG_FMT_IDS = ['%s-g%d-%s' % (door, sg, FMT_IDS[fmt]) for door, sg, fmt in DOOR_SG_FMT]
SIZES_THIN = (1, 33, 513, 4097)                        # Basic and Aug


def main_scheme(door):
    return ref.POP if door in d.HAS_SCHEME else 0


def diff(got, want, names):
    return [(i, names[i], got[i], want[i]) for i in range(len(want)) if i >= len(got) or got[i] != want[i]][:12]


def check_sizes(api, door, sg, scheme, fmt, sizes):
    for n in sizes:
        # one item: every kind alone; otherwise one layout per size
        for seed in (range(len(d.KINDS[door])) if n == 1 else (n % 5,)):
            cols, want, names = d.build_batch(door, sg, scheme, n, seed, fmt=fmt)
            got = call_door(api, door, sg, scheme, cols, fmt, d.CORE_DST)
            assert got == want, (door, sg, scheme, fmt, n, seed, diff(got, want, names))


@pytest.mark.parametrize('door,sg,fmt', DOOR_SG_FMT, ids=DOOR_SG_FMT_IDS)
def test_every_size_class(api, door, sg, fmt):
    """default knobs, every size the host and the kernels branch on (wave and workgroup boundaries, BLSGPU_WIDE_MAX 512, the 513 ..
    1,024 branch of run_verify_items, BLSGPU_COOP_MAX 4,096 and the lane-split kernels above it): the oracle's result vector"""
    check_sizes(api, door, sg, main_scheme(door), fmt, d.SIZES)


@pytest.mark.parametrize('door,sg', [(door, sg) for door in sorted(d.HAS_SCHEME) for sg in (1, 2)])
@pytest.mark.parametrize('scheme', [ref.BASIC, ref.AUG], ids=['basic', 'aug'])
def test_size_classes_basic_and_aug(api, scheme, door, sg):
    """the other two scheme DSTs of the doors that take a scheme, at one size per plan"""
    check_sizes(api, door, sg, scheme, d.RAW_PROJ, SIZES_THIN)


# ------------------------------------------------------------------ child processes
def run_worker(tmp_path, name, env, calls, timeout=300):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'pairing_door_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def door_call(door, sg, scheme, fmt, cols, op='host'):
    return {'op': op, 'door': door, 'sg': sg, 'scheme': scheme, 'fmt': fmt, 'cols': cols, 'dst': d.CORE_DST}


# the plan list of tests/test_gpu_wire.py::test_every_plan, with BLSGPU_COOP_MAX=0 added where a plan's switch acts on the lane-split
# kernels (40 and 130 items would otherwise stay on the engine), and the engine's second mode
_WIRE = {name: env for name, env, _ in WIRE_PLANS}
PLANS = [
    ('no_wide', _WIRE['no_wide']),                                                       # BLSGPU_WIDE_MAX=0: one wave per item
    ('lane_split', _WIRE['lane_split']),                                                 # BLSGPU_COOP_MAX=0
    ('first_generation', dict(_WIRE['first_generation'], BLSGPU_COOP_MAX='0')),          # k_miller2s, k_finalexps
    ('finalexp_seg', dict(_WIRE['finalexp_seg'], BLSGPU_COOP_MAX='0')),
    ('wide_mode', {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_WIDE_MODE': '1'}),
]


@pytest.mark.parametrize('name,env', PLANS, ids=[p[0] for p in PLANS])
def test_every_plan(tmp_path, name, env):
    """every pairing path at 40 and 130 items through the switches: the oracle's result vectors for every door, orientation and
    format"""
    assert env == {'no_wide': {'BLSGPU_WIDE_MAX': '0'}, 'lane_split': {'BLSGPU_COOP_MAX': '0'},
                   'first_generation': {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_MILLER_V1': '1', 'BLSGPU_FINALEXP_V1': '1', 'BLSGPU_COOP_MAX': '0'},
                   'finalexp_seg': {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_FINALEXP_SEG': '1', 'BLSGPU_COOP_MAX': '0'},
                   'wide_mode': {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_WIDE_MODE': '1'}}[name]
    batches = [(door, sg, fmt, n, d.build_batch(door, sg, main_scheme(door), n, 3, fmt=fmt)) for door, sg, fmt in DOOR_SG_FMT for n in d.PLAN_SIZES]
    got = run_worker(tmp_path, name, env, [door_call(door, sg, main_scheme(door), fmt, b[0]) for door, sg, fmt, n, b in batches])
    assert len(got) == len(batches)
    for g, (door, sg, fmt, n, b) in zip(got, batches):
        assert g == b[1], (name, door, sg, fmt, n, diff(g, b[1], b[2]))


@pytest.mark.parametrize('door', d.DOORS)
def test_stale_pairs(tmp_path, door):
    """one process, one context (BLSGPU_CONTEXTS=1); per path -- 40 items (the engine), 600 (one wave per item), 4,200 (lane-split)
    -- a call of n valid items of the door, then the same n with every item failing in the prepare kernel (for pairing2: exactly
    one pair trivial), which leaves every pair slot as the first call wrote it, then the batch with a single survivor.  A stage that
    ran a failed item on what its slots held would report the earlier item's OK."""
    calls, wants = [], []
    scheme = main_scheme(door)
    for sg in ((0,) if door == 'pairing2' else (1, 2)):
        for n in d.STALE_SIZES:
            for layout in ('all_valid', 'all_fail', 'all_but_one'):
                cols, want, names = d.build_batch(door, sg, scheme, n, n % 7, layout)
                calls.append(door_call(door, sg, scheme, d.RAW_PROJ, cols))
                wants.append((sg, n, layout, want, names))
                assert [d.failed(x) for x in want].count(False) == {'all_valid': n, 'all_fail': 0, 'all_but_one': 1}[layout]
    got = run_worker(tmp_path, 'stale_' + door, {'BLSGPU_CONTEXTS': '1'}, calls)
    assert len(got) == len(wants)
    for g, (sg, n, layout, want, names) in zip(got, wants):
        assert g == want, (door, sg, n, layout, diff(g, want, names))


def test_device_resident(tmp_path, api):
    """every argument and the result vector on the device, once per door and orientation (for sig_proof_verify_batch, core_verify and
    signcrypt_valid_batch that covers the read of offsets[n] from device memory): the oracle's vector and the host-argument call's"""
    n = 700
    batches = [(door, sg, d.build_batch(door, sg, main_scheme(door), n, 4)) for door in d.DOORS for sg in ((0,) if door == 'pairing2' else (1, 2))]
    got = run_worker(tmp_path, 'device', {}, [door_call(door, sg, main_scheme(door), d.RAW_PROJ, b[0], op='device') for door, sg, b in batches])
    assert len(got) == len(batches)
    for g, (door, sg, b) in zip(got, batches):
        assert g == b[1], (door, sg, diff(g, b[1], b[2]))
        assert g == call_door(api, door, sg, main_scheme(door), b[0], d.RAW_PROJ, d.CORE_DST), (door, sg)


# ------------------------------------------------------------------ two library calls against each other
def _pick(door, sg, scheme, n):
    """n items of the door's kinds without an identity member, kinds and base items in turn, freshly rendered: (items, cols, want)"""
    cs = d.cases(door, sg, scheme)
    ks = d.NO_IDENTITY[door]
    names = [(ks[i % len(ks)], (i // len(ks)) % d.POOL) for i in range(n)]
    return names, cs


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('n', [130, 4097])
def test_hashed_equals_verify_batch(api, sg, n):
    """core_verify_hashed on hashes from blsgpu_hash_to_g1/g2 under the Basic scheme's DST equals verify_batch on Basic: valid
    items and items whose hash is another message's"""
    import random
    rng = random.Random(n + sg)
    C = d.IMPLS[sg]
    names, cs = _pick('hashed', sg, 0, n)
    msgs_of = d.hashed_messages(sg)
    msgs = [msgs_of[j if k == 'valid' else (j + 1) % d.POOL] for k, j in names]
    hashes = api.hash_to_point(sg, msgs, C.DST[ref.BASIC])
    pks = [d.render_point(3 - sg, cs[nm][0][0], d.RAW_PROJ, rng) for nm in names]
    sigs = [d.render_point(sg, cs[nm][0][1], d.RAW_PROJ, rng) for nm in names]
    got = api.core_verify_hashed(sg, pks, sigs, hashes)
    assert got == api.verify_batch(sg, ref.BASIC, pks, sigs, msgs)
    assert got == [cs[nm][1] for nm in names] and set(got) == {0, 1}


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('n', [130, 4097])
def test_pop_equals_core_verify(api, sg, n):
    """pop_verify_batch equals core_verify with the compressed key as the message under the proof-of-possession DST"""
    import random
    rng = random.Random(n + sg)
    C = d.IMPLS[sg]
    names, cs = _pick('pop', sg, 0, n)
    pks = [d.render_point(3 - sg, cs[nm][0][0], d.RAW_PROJ, rng) for nm in names]
    proofs = [d.render_point(sg, cs[nm][0][1], d.RAW_PROJ, rng) for nm in names]
    got = api.pop_verify_batch(sg, pks, proofs)
    assert got == api.core_verify(sg, C.POP_DST, pks, proofs, api.serialize(3 - sg, pks))
    assert got == [cs[nm][1] for nm in names] and set(got) == {0, 1}


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('n', [130, 4097])
def test_sig_proof_equals_pairing2(api, sg, n):
    """sig_proof_verify_batch equals pairing2_check_batch on the pairs (-V, -g), (T, pk) with T = U + y H(m) from the oracle (once per
    pool item)"""
    import random
    from oracle.py import bls381 as c
    rng = random.Random(n + sg)
    C = d.IMPLS[sg]
    scheme = ref.POP
    names, cs = _pick('sig_proof', sg, scheme, n)
    t_of = {}
    for nm in set(names):
        u, v, pk, y, msg = cs[nm][0]
        t = C.sig_curve.add(u, C.sig_curve.mul(C.hash_to_point(msg, C.DST[scheme]), y))
        assert t is not None
        t_of[nm] = (C.sig_curve.neg(v), C.pk_curve.neg(C.pk_gen), t, pk)          # (sig group, key group) twice
    order = (0, 1, 2, 3) if sg == 1 else (1, 0, 3, 2)                              # the G1 member first
    p2 = [[d.render_point(1 + k % 2, t_of[nm][order[k]], d.RAW_PROJ, rng) for nm in names] for k in range(4)]
    cols = [list(col) for col in zip(*[d.render('sig_proof', sg, cs[nm][0], d.RAW_PROJ, rng) for nm in names])]
    got = call_door(api, 'sig_proof', sg, scheme, cols)
    assert [g == 0 for g in got] == api.pairing2_check_batch(*p2)
    assert got == [cs[nm][1] for nm in names] and set(got) == {0, 1}
