#!/usr/bin/env python3
"""Time-lock decryption over a registered signature set (blsgpu_timecrypt_open_indexed_batch) beside the by-value call on the same
ciphertexts in the same process.

usage: python tools/bench_sigset.py [--reps 5] [--shapes 2:1,2:512,2:4096,2:65536,1:4096] [--entries 1,64] [--create 64,16384]
                                    [--distinct 4096] [--step-timeout 280] [--out profiles/sigset_bench.json]
Without --worker this is a driver: every (impl, items, entries) and every creation size is one child process under
`timeout -k 10 <step-timeout>`, chained with `&&`, so the first step that fails, faults or runs out of time ends the run.  Each step
appends one row to --out and prints it.

A step (--worker): scheme Basic, 64-byte messages, host lists through the flat Python calls.  `entries` round signatures of one key
over distinct round names; the ciphertexts are sealed with the library itself from public scalars (as tools/bench_timecrypt.py), at
most --distinct of them, ciphertext i under entry i mod entries, repeated to the size.  Three forms:
  (a) by_value      blsgpu_timecrypt_open_batch with the items grouped by signature -- unchanged code, the yardstick
  (b) indexed       blsgpu_timecrypt_open_indexed_batch over a set without rows, the items in arrival order (entry i mod entries)
  (c) indexed_rows  the same over a set created with BLSGPU_SIGSET_LINES
After a warm-up of every form, --reps rounds time them alternately (host clock around blocking calls); then one more call of each
under blsgpu_profile_enable gives the per-kernel device times.  Reported: median, minimum and maximum per form, whether every
ciphertext opened to its message, and the per-kernel times.  A creation step times SignatureSet.create (median of --reps, after one
warm-up) with and without rows and reports info()'s device bytes."""
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

SALT = b'TIMELOCK_BLS12381_XOF:HKDF-SHA2-256_'
MSG_BYTES = 64
ms = lambda v: round(v * 1e3, 3)  # noqa: E731


def append_row(out, row):
    print(json.dumps(row), flush=True)
    rows = []
    if os.path.exists(out):
        with open(out) as fh:
            rows = json.load(fh)
    with open(out, 'w') as fh:
        json.dump(rows + [row], fh, indent=1)


def round_sigs(api, sg, count):
    sk = int.from_bytes(hashlib.sha256(b'bench time-lock key %d' % sg).digest(), 'little') >> 2
    return api.sign_batch(sg, api.BASIC, [sk] * count, [b'round %d' % (424242 + e) for e in range(count)])[1]


def create_worker(a):
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    sg, E = a.impl, a.size
    sigs = round_sigs(api, sg, E)
    row = {'what': 'create', 'impl': 'Bls12381G%dImpl' % sg, 'entries': E, 'rounds': a.reps}
    for lines in (False, True):
        ts = []
        for k in range(a.reps + 1):
            t0 = time.perf_counter()
            s = api.SignatureSet.create(sg, sigs, [api.BASIC] * E, lines=lines)
            ts.append(time.perf_counter() - t0)
            info = s.info()
            s.close()
        key = 'rows' if lines else 'plain'
        row['create_%s_ms' % key] = ms(statistics.median(ts[1:]))
        row['create_%s_min_ms' % key], row['create_%s_max_ms' % key] = ms(min(ts[1:])), ms(max(ts[1:]))
        row['device_bytes_%s' % key], row['has_lines_%s' % key] = info['device_bytes'], info['has_lines']
    append_row(a.out, row)


def worker(a):
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    sg, n, E = a.impl, a.size, a.entries
    d = min(n, a.distinct)
    xor = lambda x, y: (int.from_bytes(x, 'little') ^ int.from_bytes(y, 'little')).to_bytes(len(x), 'little')  # noqa: E731
    sigs = round_sigs(api, sg, E)
    msgs = [hashlib.shake_128(b'm%d' % i).digest(MSG_BYTES) for i in range(d)]
    alphas = [hashlib.sha256(b'a%d' % i).digest() for i in range(d)]
    rs = api.hash_to_scalar([al + hashlib.sha256(m).digest() for al, m in zip(alphas, msgs)], SALT)
    us = api.sign_batch(sg, api.BASIC, rs, [b''] * d)[0]
    of = [i % E for i in range(d)]
    sg_pts = [sigs[e] for e in of]
    ks, st = api.pairing_batch(sg_pts, us) if sg == 1 else api.pairing_batch(us, sg_pts)
    assert st == [0] * d
    vs = [xor(hashlib.sha256(k).digest(), al) for k, al in zip(ks, alphas)]
    frames = [bytes([MSG_BYTES]) + m for m in msgs]
    ws = [xor(hashlib.shake_128(al).digest(len(f)), f) for al, f in zip(alphas, frames)]
    arrival = [i % d for i in range(n)]                               # the items as they arrive: entry (i mod d) mod E
    items = [(of[i], us[i], vs[i], ws[i], api.BASIC) for i in arrival]
    grouped_order = sorted(range(n), key=lambda j: of[arrival[j]])    # (a) needs them sorted into groups
    groups = [(sigs[e], api.BASIC, []) for e in range(E)]
    for j in grouped_order:
        i = arrival[j]
        groups[of[i]][2].append((us[i], vs[i], ws[i], api.BASIC))
    plain = api.SignatureSet.create(sg, sigs, [api.BASIC] * E, lines=False)
    rows = api.SignatureSet.create(sg, sigs, [api.BASIC] * E, lines=True)
    forms = {
        'by_value': lambda: api.timecrypt_open_batch(sg, groups),
        'indexed': lambda: api.timecrypt_open_indexed_batch(plain, items),
        'indexed_rows': lambda: api.timecrypt_open_indexed_batch(rows, items),
    }
    got = {k: f() for k, f in forms.items()}                          # warm-up, and the results to check
    opened = got['by_value'] == [msgs[arrival[j]] for j in grouped_order] and got['indexed'] == got['indexed_rows'] == [msgs[i] for i in arrival]
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
    row = {'what': 'open', 'impl': 'Bls12381G%dImpl' % sg, 'items': n, 'entries': E, 'distinct_ciphertexts': d, 'message_bytes': MSG_BYTES, 'rounds': a.reps,
           'all_opened': opened, 'rows_built': rows.info()['has_lines']}
    for k in forms:
        row[k + '_ms'] = ms(statistics.median(ts[k]))
        row[k + '_min_ms'] = ms(min(ts[k]))
        row[k + '_max_ms'] = ms(max(ts[k]))
    row['kernel_ms_launches'] = prof
    plain.close()
    rows.close()
    append_row(a.out, row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='2:1,2:512,2:4096,2:65536,1:4096', help='impl:items, comma separated')
    ap.add_argument('--entries', default='1,64')
    ap.add_argument('--create', default='64,16384', help='set sizes whose creation is timed (Bls12381G2Impl)')
    ap.add_argument('--distinct', type=int, default=4096)
    ap.add_argument('--step-timeout', type=int, default=280)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sigset_bench.json'))
    ap.add_argument('--worker', choices=['open', 'create'])
    ap.add_argument('--impl', type=int, default=2)
    ap.add_argument('--size', type=int, default=1)
    a = ap.parse_args()
    if a.worker == 'open':
        a.entries = int(a.entries)
        return worker(a)
    if a.worker == 'create':
        return create_worker(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):
        os.remove(a.out)
    q = lambda s: "'" + str(s).replace("'", "'\\''") + "'"  # noqa: E731
    head = 'timeout -k 10 %d %s %s --reps %d --distinct %d --out %s' % (a.step_timeout, q(sys.executable), q(os.path.abspath(__file__)), a.reps, a.distinct, q(a.out))
    steps = ['%s --worker open --impl %d --size %d --entries %d' % (head, int(sh.split(':')[0]), int(sh.split(':')[1]), int(e))
             for sh in a.shapes.split(',') if sh for e in a.entries.split(',')]
    steps += ['%s --worker create --impl 2 --size %d' % (head, int(e)) for e in a.create.split(',') if e]
    return subprocess.call(['bash', '-c', ' && '.join(steps)])


if __name__ == '__main__':
    sys.exit(main())
