"""The launch sequence and the statuses of every one-key-per-item door, keys by value and by index, held against a recording: three
items (or sets of two pairs, one pair and one pair) through verify_shared_batch / verify_shared_indexed_batch, verify_msgset_batch /
verify_msgset_indexed_batch, signcrypt_share_verify_batch, aggregate_verify_indexed_batch, aggregate_verify_msgset_indexed_batch and
verify_indexed_batch (RAW_PROJ and RAW_AFFINE signatures: both ways to the keys' buffer), on the four plans of
tests/test_gpu_pairing2_launches.py, each set through the same knobs.  In every indexed step one item is tampered and one names a
position outside the key set, so the precedence of k_keyset_fin is in the statuses; the by-value steps carry the same items.

{kernel: launches} of every call and the sha256 of its status bytes equal tests/golden/item_keys_launches.json, which measure() of
that test recorded on the commit before these doors took their keys from one provider.  The statuses (and the aggregate doors' aux
words) are the model's as well: verify_shared_cases.Item.expect, msgset_cases' rule on top of it, test_gpu_signcrypt_indexed.batch,
and the oracle_set of test_gpu_agg_indexed / test_gpu_agg_msgset after a closed-form assertion -- a recording taken from a wrong run
cannot pass.  One worker per plan (tests/pairing2_launches_worker.py), one attempt each, with its own time limit."""
import functools
import json
import os

import pytest

import keyset_cases as kc
import msgset_cases as mc
import test_gpu_agg_indexed as ai
import test_gpu_agg_msgset as am
import test_gpu_pairing2_launches as p2
import test_gpu_signcrypt_indexed as si
import util
import verify_shared_cases as vc
from util import ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(util.ROOT, 'tests', 'golden', 'item_keys_launches.json')
PLANS = p2.PLANS
FMT_RAW_PROJ, FMT_RAW_AFFINE = 0, 1
E_ARG = mc.E_ARG
ITEMS = p2.ITEMS                                  # valid, tampered (signed by another key), valid
OUTSIDE = len(ITEMS)                              # the key sets hold the items' three keys: the first position past the end
POSITIONS = (0, 1, OUTSIDE)                       # item 2 names no key
ENTRIES = [b'alpha', b'beta']
GROUPS = [(0, (0, 1)), (1, (2,))]                 # (entry, items): a group of two and a group of one
SHARED = (('g1 basic', 1, ref.BASIC, 'g1 lines'), ('g1 aug', 1, ref.AUG, 'g1 lines'), ('g2 basic', 2, ref.BASIC, 'g2 plain'))
MSGSET = (('g1', 1, 'g1 lines'), ('g2', 2, 'g2 plain'))
LINED = ('verify_shared_indexed g1 basic', 'verify_shared_indexed g1 aug', 'verify_msgset_indexed g1', 'verify_indexed proj', 'verify_indexed affine')
AGGREGATES = ('aggregate_verify_indexed', 'aggregate_verify_msgset_indexed')
BY_VALUE_SIGNCRYPT = ('signcrypt_share_verify g1', 'signcrypt_share_verify g2')
STEPS = tuple(n for tag, _, _, _ in SHARED for n in ('verify_shared ' + tag, 'verify_shared_indexed ' + tag)) + \
    tuple(n for tag, _, _ in MSGSET for n in ('verify_msgset ' + tag, 'verify_msgset_indexed ' + tag)) + BY_VALUE_SIGNCRYPT + AGGREGATES + \
    ('verify_indexed proj', 'verify_indexed affine')


def indexed_expect(by_value):
    """the key set's rule on top of the by-value statuses: a position outside the set is E_ARG, whatever else the item is"""
    return [E_ARG if pos >= OUTSIDE else s for pos, s in zip(POSITIONS, by_value)]


@functools.lru_cache(maxsize=None)
def spec():
    """(worker spec, {step: expected statuses}, {aggregate step: expected aux})"""
    want, aux, steps = {}, {}, []
    keys = {sg: [vc.IMPLS[sg].pk_curve.mul(vc.IMPLS[sg].pk_gen, it.key) for it in ITEMS] for sg in (1, 2)}
    keysets = {'g1 lines': {'sg': 1, 'keys': [util.g2_raw(pk) for pk in keys[1]], 'fmt': FMT_RAW_PROJ, 'lines': True},
               'g2 plain': {'sg': 2, 'keys': [util.g1_raw(pk) for pk in keys[2]], 'fmt': FMT_RAW_PROJ, 'lines': False}}
    msgsets = {}

    def shared_groups(sg, scheme):
        """(by value: [(entry, pks, sigs)], by index: [(entry, positions, sigs)], the by-value statuses)"""
        raw = vc.raw_groups(sg, [(ENTRIES[e], [ITEMS[i].points(sg, scheme, ENTRIES[e]) for i in items]) for e, items in GROUPS])
        by_value = [(e, pks, sigs) for (e, _), (_, pks, sigs) in zip(GROUPS, raw)]
        by_index = [(e, [POSITIONS[i] for i in items], sigs) for (e, items), (_, _, sigs) in zip(GROUPS, raw)]
        return by_value, by_index, [ITEMS[i].expect(scheme, ENTRIES[e]) for e, items in GROUPS for i in items]

    # verify_shared_batch and verify_shared_indexed_batch: the group's message by value
    for tag, sg, scheme, keyset in SHARED:
        by_value, by_index, st = shared_groups(sg, scheme)
        steps.append({'name': 'verify_shared ' + tag, 'sg': sg, 'scheme': scheme, 'groups': [(ENTRIES[e], pks, sigs) for e, pks, sigs in by_value]})
        steps.append({'name': 'verify_shared_indexed ' + tag, 'door': 'verify_shared_indexed', 'keyset': keyset, 'scheme': scheme,
                      'groups': [(ENTRIES[e], ix, sigs) for e, ix, sigs in by_index]})
        want['verify_shared ' + tag], want['verify_shared_indexed ' + tag] = st, indexed_expect(st)
    # verify_msgset_batch and verify_msgset_indexed_batch: the group's message by position (every position inside the message set)
    for tag, sg, keyset in MSGSET:
        by_value, by_index, st = shared_groups(sg, ref.BASIC)
        msgsets[tag] = {'sg': sg, 'scheme': ref.BASIC, 'msgs': ENTRIES, 'lines': sg == 2}
        steps.append({'name': 'verify_msgset ' + tag, 'msgset': tag, 'groups': by_value})
        steps.append({'name': 'verify_msgset_indexed ' + tag, 'door': 'verify_msgset_indexed', 'msgset': tag, 'keyset': keyset, 'groups': by_index})
        want['verify_msgset ' + tag], want['verify_msgset_indexed ' + tag] = st, indexed_expect(st)
    # signcrypt_share_verify_batch: the ciphertexts and shares of the indexed steps of tests/test_gpu_pairing2_launches.py, keys gathered
    for sg in (1, 2):
        cl, shares, st = si.batch(sg, (1, 2), 3, bad_every=3)
        cts, sh = si.raw_batch(sg, cl, shares)
        call, covered = si.gathered_call(sg, cts, sh, FMT_RAW_PROJ, False)
        assert covered == [0, 1, 2]
        steps.append({'name': 'signcrypt_share_verify g%d' % sg, 'door': 'signcrypt_share_verify', 'sg': sg, 'scheme': ref.BASIC, 'cts': cts, 'pairs': call['pairs']})
        want['signcrypt_share_verify g%d' % sg] = st
    # the aggregate doors, Bls12381G1Impl over the 64 keys of tests/test_gpu_agg_msgset.py with lines: two pairs; one pair under
    # another key than signed; one pair at a position outside the key set
    t, bo = am.table(1), util.load_c_oracle()
    p = t['plain']
    sent = [([p[0], p[1]], [0, 1]), ([p[3]], [2]), ([kc.N], [4])]
    sigs = am.signed_sets(1, ref.BASIC, [([(p[0], 0), (p[1], 1)], None), ([(p[2], 2)], None), ([(kc.N, 4)], None)])
    by_msg = [(ix, [am.MSGS[m] for m in midx], g) for (ix, midx), g in zip(sent, sigs)]
    by_midx = [(ix, midx, g) for (ix, midx), g in zip(sent, sigs)]
    closed = [(ai.OK, ai.NO_AUX), (ai.INVALID, ai.NO_AUX), (E_ARG, ai.NO_AUX)]
    assert kc.N >= am.N and [ai.oracle_set(bo, t, 1, ref.BASIC, *s) for s in by_msg] == closed == [am.oracle_set(bo, 1, ref.BASIC, *s) for s in by_midx]
    keysets['agg lines'] = {'sg': 1, 'keys': t['blobs'], 'fmt': t['fmt'], 'lines': True}
    msgsets['agg'] = {'sg': 1, 'scheme': ref.BASIC, 'msgs': am.MSGS, 'lines': False}
    steps.append({'name': 'aggregate_verify_indexed', 'door': 'aggregate_verify_indexed', 'keyset': 'agg lines', 'scheme': ref.BASIC, 'sets': by_msg})
    steps.append({'name': 'aggregate_verify_msgset_indexed', 'door': 'aggregate_verify_msgset_indexed', 'msgset': 'agg', 'keyset': 'agg lines', 'sets': by_midx})
    for name in AGGREGATES:
        want[name], aux[name] = [s for s, _ in closed], [list(a) for _, a in closed]
    # verify_indexed_batch, every item its own message: RAW_PROJ signatures (the keys through k_keyset_to_proj) and RAW_AFFINE
    msgs = [b'item keys %d' % i for i in range(3)]
    pts = [it.points(1, ref.BASIC, m) for it, m in zip(ITEMS, msgs)]
    st = indexed_expect([it.expect(ref.BASIC, m) for it, m in zip(ITEMS, msgs)])
    for tag, fmt, raw in (('proj', FMT_RAW_PROJ, util.g1_raw), ('affine', FMT_RAW_AFFINE, util.g1_aff_raw)):
        steps.append({'name': 'verify_indexed ' + tag, 'door': 'verify_indexed', 'keyset': 'g1 lines', 'scheme': ref.BASIC, 'idx': list(POSITIONS),
                      'sigs': [raw(s) for _, s in pts], 'msgs': msgs, 'fmt': fmt})
        want['verify_indexed ' + tag] = st
    assert tuple(s['name'] for s in steps) == STEPS and all(len(w) == 3 for w in want.values())
    assert all(sorted(want[n]) == [E_ARG, vc.OK, vc.INVALID_SIGNATURE] for n in STEPS if 'indexed' in n)
    return {'keysets': keysets, 'msgsets': msgsets, 'steps': steps}, want, aux


def measure(plan, tmp_dir):
    """the steps in one worker under the plan's knobs, as tests/test_gpu_pairing2_launches.py measures its own"""
    return p2.measure(plan, tmp_dir, worker_spec=spec()[0])


@pytest.mark.parametrize('plan', sorted(PLANS))
def test_launches_and_statuses_equal_the_recording(tmp_path, plan):
    with open(GOLDEN) as f:
        golden = json.load(f)[plan]
    _, want, aux = spec()
    got = measure(plan, tmp_path)
    assert sorted(got) == sorted(golden) == sorted(STEPS)
    for name in STEPS:
        print(plan, name, got[name]['st'], got[name]['launches'])
        assert got[name]['st'] == want[name], (plan, name)
        assert got[name].get('aux') == aux.get(name), (plan, name)
        assert got[name]['launches'] == golden[name]['launches'], (plan, name)
        assert got[name]['status_sha256'] == golden[name]['status_sha256'], (plan, name)


def test_the_recording_names_a_keyed_kernel_on_every_forced_plan():
    """what the recording itself must show, so that it cannot have been taken from runs that fell back: above the row-wide engine every
    indexed call over the set with lines runs the kernel that reads the keys' rows, once per chunk of two items on the chunked plan
    (aggregate_verify_indexed_batch: its keyed line kernel, on every plan); the by-value signcryption calls build no table on any plan"""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(PLANS)
    for plan in PLANS:
        assert sorted(golden[plan]) == sorted(STEPS)
        for name in BY_VALUE_SIGNCRYPT:            # the profile counts the door's small kernels under one name: prefix, copy, pairs, status and
            launches = golden[plan][name]['launches']  # no more -- a fifth would be k_signcrypt_ct_affine, _tab_of or _swap_pairs
            assert launches.get('k_signcrypt_share_pairs', 0) == 4 and launches.get('k_group_lines', 0) == 0, (plan, name, launches)
        for name in AGGREGATES:                   # by message index the keys of one message are summed first: a sum has no rows, and is walked
            launches = golden[plan][name]['launches']
            want = (1, 0) if name == 'aggregate_verify_indexed' else (0, 1)
            assert (launches.get('k_linesp_keyed', 0), launches.get('k_linesp', 0)) == want, (plan, name, launches)
        if plan == 'default':
            continue
        keyed, chunks = ('k_pairing_coop_keyed', 1) if plan == 'one wave' else ('k_lines2s_keyed', 2 if plan == 'lane split, chunked' else 1)
        for name in LINED:
            launches = golden[plan][name]['launches']
            assert launches.get(keyed, 0) == chunks, (plan, name, launches)
            assert launches.get('k_pairing_coop', 0) == 0 and launches.get('k_lines2s', 0) == 0, (plan, name, launches)
    for name in STEPS:
        assert not any(k.startswith(('k_pairing_coop', 'k_lines2s', 'k_millerf2s')) for k in golden['default'][name]['launches']) or name in AGGREGATES, name
        assert len({golden[plan][name]['status_sha256'] for plan in PLANS}) == 1, name
