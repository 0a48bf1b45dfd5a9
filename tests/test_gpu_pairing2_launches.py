"""The launch sequence of every entry point that feeds line tables to run_pairing2, held against a recording: three items through
verify_indexed_batch over a key set with lines, verify_shared_batch and verify_msgset_batch (with rows) for Bls12381G2Impl and
signcrypt_share_verify_indexed_batch for both implementations, on default knobs (the row-wide engine) and on each forced plan of
tests/test_gpu_signcrypt_indexed.py -- one wave per item, the lane-split kernels, and those in chunks of two items, so that three
items make two chunks.  On the forced plans BLSGPU_SHARED_LINES_MIN=1 and BLSGPU_SIGNCRYPT_LINES_MIN=1 are set as well: both only
price a table build against the batch's shape (they never change a result), and without them three items would build no table and
the Bls12381G2Impl calls would hand run_pairing2 none.

{kernel: launches} of every call and the sha256 of its status bytes equal tests/golden/pairing2_launches.json, which measure() below
recorded on the commit before run_pairing2 took its tables as one descriptor: a change to how that function or its callers pick a
path or a kernel shows here as a diff of names and counts.  The statuses are the model's as well (verify_shared_cases.Item.expect,
test_gpu_signcrypt_indexed.batch).  Knobs are read once per process: one worker per plan (tests/pairing2_launches_worker.py), one
attempt each, with its own time limit."""
import functools
import hashlib
import json
import os
import pickle
import struct
import subprocess
import sys

import pytest

import test_gpu_signcrypt_indexed as si
import util
import verify_shared_cases as vc
from util import ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(util.ROOT, 'tests', 'golden', 'pairing2_launches.json')
TABLES = {'BLSGPU_SHARED_LINES_MIN': '1', 'BLSGPU_SIGNCRYPT_LINES_MIN': '1'}
PLANS = {'default': {},
         'one wave': dict(TABLES, BLSGPU_WIDE_MAX='0'),
         'lane split': dict(TABLES, BLSGPU_COOP_MAX='0'),
         'lane split, chunked': dict(TABLES, BLSGPU_COOP_MAX='0', BLSGPU_AB_KNOBS='1', BLSGPU_MILLER_CHUNK='2')}
STEPS = ('verify_indexed', 'verify_shared g2', 'verify_msgset g2', 'signcrypt g1', 'signcrypt g2')
ITEMS = (vc.valid(31), vc.Item('tampered: signed by another key', 32, 35), vc.valid(33))


@functools.lru_cache(maxsize=None)
def spec():
    """(worker spec, {step: expected statuses}): three items per call, the second one tampered"""
    FMT_RAW_PROJ, FMT_COMPRESSED = 0, 2
    want = {}
    # verify_indexed_batch, Bls12381G1Impl: item i under key i of a set with lines, every item its own message
    msgs = [b'pairing2 item %d' % i for i in range(3)]
    pts = [it.points(1, ref.BASIC, m) for it, m in zip(ITEMS, msgs)]
    keysets = {'g1 lines': {'sg': 1, 'keys': [util.g2_raw(pk) for pk, _ in pts], 'fmt': FMT_RAW_PROJ, 'lines': True}}
    steps = [{'name': 'verify_indexed', 'keyset': 'g1 lines', 'scheme': ref.BASIC, 'idx': [0, 1, 2], 'sigs': [util.g1_raw(s) for _, s in pts], 'msgs': msgs}]
    want['verify_indexed'] = [it.expect(ref.BASIC, m) for it, m in zip(ITEMS, msgs)]
    # verify_shared_batch and verify_msgset_batch, Bls12381G2Impl: groups of two items and of one
    entries = [b'alpha', b'beta']
    groups = [(0, ITEMS[:2]), (1, ITEMS[2:])]
    raw = vc.raw_groups(2, [(entries[e], [it.points(2, ref.BASIC, entries[e]) for it in items]) for e, items in groups])
    steps.append({'name': 'verify_shared g2', 'sg': 2, 'scheme': ref.BASIC, 'groups': raw})
    steps.append({'name': 'verify_msgset g2', 'msgset': 'g2 rows', 'groups': [(e, pks, sigs) for (e, _), (_, pks, sigs) in zip(groups, raw)]})
    msgsets = {'g2 rows': {'sg': 2, 'scheme': ref.BASIC, 'msgs': entries, 'lines': True}}
    want['verify_shared g2'] = want['verify_msgset g2'] = [it.expect(ref.BASIC, entries[e]) for e, items in groups for it in items]
    # signcrypt_share_verify_indexed_batch: ciphertexts of one share and of two, the middle share under the next member's position
    for sg in (1, 2):
        t = si.ic.table(sg)
        cl, shares, st = si.batch(sg, (1, 2), 3, bad_every=3)
        cts, sh = si.raw_batch(sg, cl, shares)
        keysets['signcrypt g%d' % sg] = {'sg': sg, 'keys': t['blobs'], 'fmt': FMT_COMPRESSED, 'lines': sg == 1}
        steps.append({'name': 'signcrypt g%d' % sg, 'keyset': 'signcrypt g%d' % sg, 'scheme': ref.BASIC, 'cts': cts, 'shares': sh})
        want['signcrypt g%d' % sg] = st
    assert tuple(s['name'] for s in steps) == STEPS and all(len(w) == 3 for w in want.values())
    return {'keysets': keysets, 'msgsets': msgsets, 'steps': steps}, want


def measure(plan, tmp_dir, timeout=240, worker_spec=None):
    """the steps (of this file's spec, or of worker_spec) in one worker under the plan's knobs:
    {step: {'launches': {kernel: count}, 'status_sha256': ..., 'st': [...][, 'aux': what an aggregate door gave]}}"""
    path = os.path.join(str(tmp_dir), 'pairing2.pickle')
    with open(path, 'wb') as f:
        pickle.dump(worker_spec or spec()[0], f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'pairing2_launches_worker.py'), path], env=dict(keep, **PLANS[plan]),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (plan, r.returncode, r.stderr[-3000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    return {name: dict(g, status_sha256=hashlib.sha256(struct.pack('<%di' % len(g['st']), *g['st'])).hexdigest()) for name, g in got.items()}


@pytest.mark.parametrize('plan', sorted(PLANS))
def test_launches_and_statuses_equal_the_recording(tmp_path, plan):
    with open(GOLDEN) as f:
        golden = json.load(f)[plan]
    want = spec()[1]
    got = measure(plan, tmp_path)
    assert sorted(got) == sorted(golden) == sorted(STEPS)
    for name in STEPS:
        print(plan, name, got[name]['launches'])
        assert got[name]['st'] == want[name], (plan, name)
        assert got[name]['launches'] == golden[name]['launches'], (plan, name)
        assert got[name]['status_sha256'] == golden[name]['status_sha256'], (plan, name)


def test_the_recording_names_a_tabled_kernel_on_every_forced_plan():
    """what the recording itself must show, so that it cannot have been taken from runs that fell back: above the row-wide engine
    every call runs a kernel that reads rows, and the chunked plan launches its line kernel once per chunk of two items"""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(PLANS)
    tabled = {'one wave': {'verify_indexed': 'k_pairing_coop_keyed', 'verify_shared g2': 'k_pairing_coop', 'verify_msgset g2': 'k_pairing_coop_rows',
                           'signcrypt g1': 'k_pairing_coop_rows', 'signcrypt g2': 'k_pairing_coop_tables2'},
              'lane split': {'verify_indexed': 'k_lines2s_keyed', 'verify_shared g2': 'k_lines2s', 'verify_msgset g2': 'k_lines2s', 'signcrypt g1': 'k_lines2s',
                             'signcrypt g2': 'k_lines2s_tables2'}}
    tabled['lane split, chunked'] = tabled['lane split']
    for plan, kernels in tabled.items():
        chunks = 2 if plan == 'lane split, chunked' else 1
        for name, kernel in kernels.items():
            launches = golden[plan][name]['launches']
            assert launches.get(kernel, 0) == (chunks if plan != 'one wave' else 1), (plan, name, launches)
            if plan != 'one wave':
                assert launches.get('k_millerf2s', 0) == chunks and launches.get('k_pairing_coop', 0) == 0, (plan, name, launches)
    for name in STEPS:
        assert not any(k.startswith(('k_pairing_coop', 'k_lines2s', 'k_millerf2s')) for k in golden['default'][name]['launches']), name      # the engine
        assert len({golden[plan][name]['status_sha256'] for plan in PLANS}) == 1, name
