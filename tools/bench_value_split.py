#!/usr/bin/env python3
"""Pairing values: the one-wave plan (k_pairing_value / k_pairing_value_rows over 4,096-item chunks) against the lane-split plan
(k_linesp + k_millerfp3 or k_millerf_rows1, then k_finalexp2s_value) -- the measurement behind the default of BLSGPU_VALUE_SPLIT_MIN.

usage: python tools/bench_value_split.py [--sizes 4096,4097,8192,16384,32768,65536] [--reps 5] [--repeats 2] [--distinct 4096]
                                         [--entries 64] [--step-timeout 280] [--out profiles/value_split_bench.json]
Without --worker this is a driver.  The knobs are parsed once per process, so every (size, plan) is a child process of its own, run
--repeats times with the two plans ALTERNATING (BLSGPU_VALUE_SPLIT_MIN=0, =1, =0, =1, ...), each under `timeout -k 10 <step-timeout>`
and chained with `&&`: the first step that fails, faults or runs out of time ends the run.  Each step appends one row to --out and
prints it; the last step (--worker summary) appends the table and the default that follows from it.

A step (--worker run): `distinct` pairs (a_i g1, b_i g2) from public scalars, made with the library itself, repeated to the size; host
lists through the flat Python calls.  Three forms, each checked against the first call of the process on the same pairs:
  by_value        blsgpu_pairing_batch (the pairing step of blsgpu_timecrypt_open_batch is the same launches under both impls)
  indexed_g1      blsgpu_pairing_sigset_batch over a Bls12381G1Impl set of --entries signatures (no rows exist there: every pair is walked)
  indexed_rows    the same over a Bls12381G2Impl set created with BLSGPU_SIGSET_LINES (k_pairing_value_rows / k_millerf_rows1)
After a warm-up of every form, --reps rounds time them alternately (host clock around blocking calls); then one more call of each under
blsgpu_profile_enable gives the per-kernel device times, and `pairing_step_ms` is their sum over the kernels of the pairing step.

The default (--worker summary): per size and form, a plan's figure is the median over its repeats of the per-process medians, and the
spread of the one-wave plan is the largest minus the smallest of its per-process medians.  A size QUALIFIES when, in every form, the
lane-split figure is below the one-wave figure by more than that spread.  The default is the smallest measured size that qualifies
together with every larger measured size; 0 (never) if there is none."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_KERNELS = ('k_pairing_value', 'k_pairing_value_rows', 'k_linesp', 'k_millerfp', 'k_millerf_rows1', 'k_finalexp2s_value')
FORMS = ('by_value', 'indexed_g1', 'indexed_rows')
ms = lambda v: round(v * 1e3, 3)  # noqa: E731


def append_row(out, row):
    print(json.dumps(row), flush=True)
    rows = []
    if os.path.exists(out):
        with open(out) as fh:
            rows = json.load(fh)
    with open(out, 'w') as fh:
        json.dump(rows + [row], fh, indent=1)


def scalars(tag, count):
    return [int.from_bytes(hashlib.sha256(b'%s %d' % (tag, i)).digest(), 'little') >> 2 for i in range(count)]


def worker(a):
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    n, E = a.size, a.entries
    d = min(n, a.distinct)
    # sign_batch(sg, ...) returns (public keys, signatures): keys of Bls12381G1Impl are multiples of g2, of Bls12381G2Impl multiples of g1
    g1s = api.sign_batch(2, api.BASIC, scalars(b'value split g1', d), [b''] * d)[0]
    g2s = api.sign_batch(1, api.BASIC, scalars(b'value split g2', d), [b''] * d)[0]
    e1 = api.sign_batch(2, api.BASIC, scalars(b'value split e1', E), [b''] * E)[0]      # the entries of the Bls12381G1Impl set: G1 points
    e2 = api.sign_batch(1, api.BASIC, scalars(b'value split e2', E), [b''] * E)[0]      # ... of the Bls12381G2Impl set: G2 points
    rep = lambda xs: [xs[i % d] for i in range(n)]  # noqa: E731
    idx = [(i % d) % E for i in range(n)]
    s1 = api.SignatureSet.create(1, e1, [api.BASIC] * E, lines=True)
    s2 = api.SignatureSet.create(2, e2, [api.BASIC] * E, lines=True)
    G1, G2 = rep(g1s), rep(g2s)
    forms = {
        'by_value': lambda: api.pairing_batch(G1, G2),
        'indexed_g1': lambda: api.pairing_sigset_batch(s1, idx, G2),
        'indexed_rows': lambda: api.pairing_sigset_batch(s2, idx, G1),
    }
    got = {k: f() for k, f in forms.items()}                          # warm-up, and the results to check
    want1 = api.pairing_batch([e1[k] for k in idx[:d]], g2s)
    want2 = api.pairing_batch(g1s, [e2[k] for k in idx[:d]])
    ok = all(st == [0] * n for _, st in got.values()) and got['by_value'][0][:d] == got['by_value'][0][n - n % d - d:n - n % d] and \
        got['indexed_g1'][0][:d] == want1[0] and got['indexed_rows'][0][:d] == want2[0] and \
        all(got[k][0][i] == got[k][0][i % d] for k in forms for i in range(0, n, max(1, n // 64)))
    ts = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    prof = {}
    for k, f in forms.items():
        api.profile_enable(True)
        f()
        prof[k] = {kk: [round(v[0], 3), v[1]] for kk, v in api.profile_read().items() if v[1]}
        api.profile_enable(False)
    row = {'what': 'run', 'plan': 'lane_split' if a.plan else 'one_wave', 'items': n, 'distinct_pairs': d, 'entries': E, 'rounds': a.reps, 'repeat': a.repeat,
           'values_agree': ok, 'rows_built': s2.info()['has_lines']}
    for k in forms:
        row[k + '_ms'] = ms(statistics.median(ts[k]))
        row[k + '_min_ms'], row[k + '_max_ms'] = ms(min(ts[k])), ms(max(ts[k]))
        row[k + '_pairing_step_ms'] = round(sum(v[0] for kk, v in prof[k].items() if kk in STEP_KERNELS), 3)
    row['kernel_ms_launches'] = prof
    s1.close()
    s2.close()
    append_row(a.out, row)
    return 0 if ok else 1


def summary(a):
    with open(a.out) as fh:
        rows = [r for r in json.load(fh) if r.get('what') == 'run']
    sizes = sorted({r['items'] for r in rows})
    table, qualifies = [], {}
    for n in sizes:
        line, good = {'items': n}, True
        for f in FORMS:
            for key in ('_ms', '_pairing_step_ms'):
                one = [r[f + key] for r in rows if r['items'] == n and r['plan'] == 'one_wave']
                two = [r[f + key] for r in rows if r['items'] == n and r['plan'] == 'lane_split']
                if not one or not two:
                    good = False
                    continue
                spread = round(max(one) - min(one), 3)
                line[f + key] = {'one_wave': round(statistics.median(one), 3), 'lane_split': round(statistics.median(two), 3), 'one_wave_spread': spread}
                if key == '_ms' and not statistics.median(two) < statistics.median(one) - spread:
                    good = False
        qualifies[n] = good
        line['qualifies'] = good
        table.append(line)
    default = 0
    for n in reversed(sizes):
        if not qualifies[n]:
            break
        default = n
    append_row(a.out, {'what': 'summary', 'rule': 'smallest measured size from which, at it and at every larger measured size, the lane-split call is faster than '
                       'the one-wave call in every form by more than the spread of the repeated one-wave runs; 0 if none', 'table': table, 'default': default})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='4096,4097,8192,16384,32768,65536')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--distinct', type=int, default=4096)
    ap.add_argument('--entries', type=int, default=64)
    ap.add_argument('--step-timeout', type=int, default=280)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'value_split_bench.json'))
    ap.add_argument('--worker', choices=['run', 'summary'])
    ap.add_argument('--size', type=int, default=1)
    ap.add_argument('--plan', type=int, default=0)
    ap.add_argument('--repeat', type=int, default=0)
    a = ap.parse_args()
    if a.worker == 'run':
        return worker(a)
    if a.worker == 'summary':
        return summary(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):
        os.remove(a.out)
    q = lambda s: "'" + str(s).replace("'", "'\\''") + "'"  # noqa: E731
    tail = '%s %s --reps %d --distinct %d --entries %d --out %s' % (q(sys.executable), q(os.path.abspath(__file__)), a.reps, a.distinct, a.entries, q(a.out))
    steps = []
    for n in (int(s) for s in a.sizes.split(',') if s):
        for rep in range(a.repeats):
            for plan in (0, 1):
                steps.append('BLSGPU_VALUE_SPLIT_MIN=%d timeout -k 10 %d %s --worker run --size %d --plan %d --repeat %d' % (plan, a.step_timeout, tail, n, plan, rep))
    steps.append(tail + ' --worker summary')
    return subprocess.call(['bash', '-c', ' && '.join(steps)])


if __name__ == '__main__':
    sys.exit(main())
