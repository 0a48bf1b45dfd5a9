"""Every device form of the final exponentiation + verdict on crafted Fp12 inputs (tests/finalexp_cases.py), against the oracle.

Miller values of real points are random-looking and nonzero, so the verify tests never give the final exponentiation a zero
(which is not in Fp12* and must fail) nor an element whose easy part is 1 (every a^x then meets z2 = 0 and the compressed
squarings decline to the plain chain).  Here the records go in directly:
  batch forms    blsgpu_debug_finalexp_batch: form 0 k_finalexp2s, 1 k_finalexp_seg + k_cyc_run4 (both through the verify path's
                 chunk launcher, chunk 0 = the library's and 64 so that chunks with first > 0 occur), 2 k_finalexps; the families
                 shuffled together so that declining and compressed items share a wave, and preset non-OK statuses that must
                 come back unchanged
  product forms  blsgpu_fp12_product_is_one under the default (engine, program FINAL), BLSGPU_WIDE_MAX=0 (wave form) and
                 BLSGPU_COOP_MAX=0 (lane-pair form), at sizes that reach the k_f12_fold halvings, the k_f12_tree_wide levels
                 and their padding of absent items with 1
The knobs are read once at library init, so each plan runs in a child process (tests/finalexp_worker.py), one at a time."""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import finalexp_cases as fc
import util

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 127, 128, 129, 257)
KS = (1, 2, 3, 16, 17, 300, 4096, 4097, 4100)
BATCH_RUNS = ((0, 0), (0, 64), (1, 0), (1, 64), (2, 0))       # (form, chunk)
PRODUCT_PLANS = (('default', {}), ('wide_max0', {'BLSGPU_WIDE_MAX': '0'}), ('coop_max0', {'BLSGPU_COOP_MAX': '0'}))


class Records:
    """The records of a spec, each value encoded once (index into the blob the worker reads)."""

    def __init__(self):
        self.blobs, self.index = [], {}

    def add(self, v):
        key = 'zero' if v is None else id(v)
        if key not in self.index:
            self.index[key] = len(self.blobs)
            self.blobs.append(fc.record(v))
        return self.index[key]


@functools.lru_cache(maxsize=None)
def pool():
    return [(name, fam, v, fc.verdict(v)) for name, fam, v in fc.family_pool()]


def batch_spec(recs):
    """Cases and per-item expectations of the batch forms."""
    pl = pool()
    names = [p[0] for p in pl]
    rng = random.Random(21)
    cases, expect = [], {}
    for n in NS:
        if n == 1:
            order = [names.index('zero')]
        elif n == 2:
            order = [names.index('fp6_0'), names.index('y^r_0')]
        else:
            order = []
            while len(order) < n:        # every member of every family, shuffled: decliners and compressed items share waves
                order += rng.sample(range(len(pl)), len(pl))
            order = order[:n]
        preset = [2 if n > 2 and i % 9 == 4 else 3 if n > 2 and i % 13 == 7 else fc.OK for i in range(n)]
        want = [preset[i] if preset[i] != fc.OK else pl[order[i]][3] for i in range(n)]
        labels = [pl[o][0] for o in order]
        for form, chunk in BATCH_RUNS:
            name = 'form%d_chunk%d_n%d' % (form, chunk, n)
            cases.append({'name': name, 'form': form, 'chunk': chunk, 'records': [recs.add(pl[o][2]) for o in order], 'status': preset})
            expect[name] = (want, labels)
    return cases, expect


@functools.lru_cache(maxsize=None)
def product_values():
    """[(name, values, expected verdict)] of the product forms."""
    rng = random.Random(31)
    out = []
    for k in KS:
        for name, (vals, v) in fc.product_sets(k, rng).items():
            out.append(('k%d_%s' % (k, name), vals, v))
    for name, _, val, v in pool():
        out.append(('single_' + name, [val], v))
    return out


def product_spec(recs):
    cases, expect = [], {}
    for name, vals, v in product_values():
        cases.append({'name': name, 'records': [recs.add(x) for x in vals]})
        expect[name] = v == fc.OK
    return cases, expect


def run_child(tmp_path, name, env, spec, recs):
    path = os.path.join(str(tmp_path), name + '.json')
    blob = os.path.join(str(tmp_path), name + '.bin')
    json.dump(spec, open(path, 'w'))
    with open(blob, 'wb') as f:
        f.write(b''.join(recs.blobs))
    # one attempt: a worker that dies by a signal or outlives the limit fails the test (nothing is retried)
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'finalexp_worker.py'), path, blob],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_batch_forms_on_crafted_records(tmp_path):
    recs = Records()
    cases, expect = batch_spec(recs)
    res = run_child(tmp_path, 'batch', {}, {'batch': cases, 'product': []}, recs)
    assert [r[0] for r in res['batch']] == [cs['name'] for cs in cases]
    bad = []
    for name, got in res['batch']:
        want, labels = expect[name]
        assert len(got) == len(want), name
        bad += [(name, i, labels[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:40]


@pytest.mark.parametrize('plan', [p[0] for p in PRODUCT_PLANS])
def test_product_forms_on_crafted_records(tmp_path, plan):
    env = dict(PRODUCT_PLANS)[plan]
    recs = Records()
    cases, expect = product_spec(recs)
    res = run_child(tmp_path, 'product_' + plan, env, {'batch': [], 'product': cases}, recs)
    assert [r[0] for r in res['product']] == [cs['name'] for cs in cases]
    bad = [(name, got, expect[name]) for name, got in res['product'] if got != expect[name]]
    assert not bad, (plan, bad)
