"""The G1 map with the 11-isogeny at an affine x (csrc/h2c.cuh sswu_g1_inv + iso_map_g1) on the device, on every hash path of the
one-lane field type: the 96 inputs of tests/h2c_affine_cases.py (poles, tv2 = 0, 0, 1, p - 1, both signs of chi, all as u + k p) in pairs
through the door blsgpu_debug_map_to_curve -- one lane and two lanes per item, cleared and uncleared -- and whole calls on 130 items
(three waves in the two-lane form, the last one ragged) in the kernels' one-lane and two-lane forms: blsgpu_verify_batch
(k_prepare<1>) and blsgpu_aggregate_verify (k_prepare_agg<1>) with the benchmark's tamper pattern against the C oracle, and
blsgpu_hash_to_g1 (k_hash_to_g1, expand_message_xmd included) against the Python oracle.  Points are compared as points (RAW_PROJ
normalised with Python integers, the identity is Z = 0), exactly.

The kernel form of a whole call is chosen by knobs that the library reads once, so those calls run in a worker process
(tests/h2c_affine_worker.py), one per form, one attempt each under its own time limit; the launch counts it reports say which kernel
ran, so no form can pass by taking another path."""
import ctypes
import functools
import json
import os
import pickle
import subprocess
import sys

import pytest

import h2c_affine_cases as ac
import h2c_cases as hc
import util
from util import ref
from oracle.py import bls381 as c

pytestmark = pytest.mark.gpu

LANE, PAIR = 0, 1                       # the door's paths of the one-lane field type (tests/test_gpu_h2c_map.py lists them all)
FORMS = [(LANE, 0), (LANE, 1), (PAIR, 0), (PAIR, 1)]
IDS = ['%s-%s' % ('LANE' if p == LANE else 'PAIR', 'Q' if u else 'H') for p, u in FORMS]
N = 130
TAMPERED = list(range(37, N, 100))      # bench.py: one message bit of every hundredth item from 37 on, flipped after signing
# Bls12381G1Impl calls on 130 items.  Without the one-wave-per-item and row-wide plans (BLSGPU_COOP_MAX / BLSGPU_WIDE_MAX = 0)
# blsgpu_verify_batch runs the two-lane k_prepare<1> of the benchmark, blsgpu_aggregate_verify the two-lane k_prepare_agg<1> and
# blsgpu_hash_to_g1 the one-lane k_hash_to_g1; the A/B switches select the one-lane k_prepare<1> and k_prepare_agg<1> (the latter
# is the benchmark's form at 262,144 pairs), and with BLSGPU_COOP_MAX left alone blsgpu_hash_to_g1 runs two lanes per message
PLANS = [('two_lanes', {'BLSGPU_COOP_MAX': '0', 'BLSGPU_WIDE_MAX': '0'}),
         ('one_lane', {'BLSGPU_WIDE_MAX': '0', 'BLSGPU_AB_KNOBS': '1', 'BLSGPU_PREPARE_LANES': '1', 'BLSGPU_AGG_LANES': '1'})]


# ---------------------------------------------------------------- the door: chosen field elements
@pytest.mark.parametrize('form', FORMS, ids=IDS)
def test_map_to_curve_door(api, form):
    path, uncleared = form
    cases = ac.pairs()
    outs = api.debug_map_to_curve(1, path, uncleared, [cs['uniform'] for cs in cases])
    assert len(outs) == len(cases)
    for cs, o in zip(cases, outs):
        hc.check(cs, o, uncleared, 'G1 %s, affine isogeny,' % ('LANE' if path == LANE else 'PAIR'))


def test_map_to_curve_door_single_maps(api):
    """every input beside u = 0 and beside itself: Q - map(0) and Q / 2 would need the oracle's arithmetic, so the expected sums are
    formed from the oracle's single maps -- a pole leaves the other map's point, twice a pole the identity"""
    ins, ex = ac.inputs(), ac.expected()
    zero = next(i for i, d in enumerate(ins) if d['u'] == 0)
    cases = []
    for i, d in enumerate(ins):
        for j in (zero, i):
            q = c.E1.add(ex[i], ex[j])
            cases.append({'name': '%s | %s' % (d['name'], ins[j]['name']), 'group': 1, 'uniform': d['block'] + ins[j]['block'], 'Q': q, 'H': None})
    for path in (LANE, PAIR):
        outs = api.debug_map_to_curve(1, path, 1, [cs['uniform'] for cs in cases])
        for cs, o in zip(cases, outs):
            hc.check(cs, o, 1, 'G1 %s, affine isogeny,' % ('LANE' if path == LANE else 'PAIR'))


# ---------------------------------------------------------------- whole calls on 130 items
V = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)  # noqa: E731


def _offs(msgs):
    o = (ctypes.c_uint64 * (len(msgs) + 1))()
    for i, m in enumerate(msgs):
        o[i + 1] = o[i] + len(m)
    return o


@functools.lru_cache(maxsize=None)
def reference():
    """the 130 items (signed on the device, 32-byte messages, one bit flipped after signing in the benchmark's pattern), the two
    aggregates (all messages as signed; the tampered ones) and what the ORACLES say of them -- computed once, shared by the plans"""
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    bo = util.load_c_oracle()
    import hashlib
    signed = [hashlib.sha256(b'affine isogeny %d' % i).digest() for i in range(N)]
    sks = [ref.keygen_from_hash(bytes([i]) * 32) for i in range(N)]
    pks, sigs = api.sign_batch(1, ref.BASIC, sks, signed)
    msgs = list(signed)
    for i in TAMPERED:
        msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
    agg = api.point_sum(1, sigs)
    st = (ctypes.c_int32 * N)()
    bo.bo_verify_batch(1, ref.BASIC, V(b''.join(pks)), V(b''.join(sigs)), V(b''.join(msgs)), ctypes.cast(_offs(msgs), ctypes.c_void_p), N,
                       ctypes.cast(st, ctypes.c_void_p), 8)
    want_verify = list(st)
    assert want_verify == [1 if i in TAMPERED else 0 for i in range(N)] and TAMPERED == [37]
    want_agg = []
    for ms in (signed, msgs):
        aux = (ctypes.c_uint64 * 2)()
        s = bo.bo_aggregate_verify(1, ref.BASIC, V(b''.join(pks)), V(b''.join(ms)), ctypes.cast(_offs(ms), ctypes.c_void_p), N, V(agg), 8,
                                   ctypes.cast(aux, ctypes.c_void_p))
        want_agg.append([s, [aux[0], aux[1]]])
    assert [w[0] for w in want_agg] == [0, 1]
    dst = ref.G1Impl.DST[ref.BASIC]
    want_hash = [c.hash_to_g1(m, dst) for m in msgs]
    spec = {'scheme': ref.BASIC, 'pks': pks, 'sigs': sigs, 'msgs': msgs, 'aggregates': [(pks, signed, agg), (pks, msgs, agg)], 'hash_msgs': msgs,
            'dst': dst}
    return spec, want_verify, want_agg, want_hash


@pytest.mark.parametrize('plan', PLANS, ids=[p[0] for p in PLANS])
def test_whole_calls_130_items(tmp_path, plan):
    name, env = plan
    spec, want_verify, want_agg, want_hash = reference()
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump(spec, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    # one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'h2c_affine_worker.py'), path], env=dict(keep, **env), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    # the kernels this plan is about ran: one k_prepare<1> (the row-wide plans of small batches do not launch it), two
    # k_prepare_agg<1>, one hash kernel
    ln = res['launches']
    assert ln.get('k_prepare') == 1 and ln.get('k_prepare_agg') == 2 and ln.get('k_hash_to_point') == 1, ln
    assert res['verify'] == want_verify
    assert res['aggregate'] == want_agg
    got = [hc.normalise(1, bytes.fromhex(h)) for h in res['hash']]
    assert got == want_hash
    assert all(p is not None and c.E1.on_curve(p) for p in got)
