#!/usr/bin/env python3
"""Time-lock decryption (blsgpu_timecrypt_open_batch) and the pairing value it rests on (blsgpu_pairing_batch) beside the yardstick
of this library's one-wave pairing, blsgpu_verify_batch at the same number of items in the same process.

usage: python tools/bench_timecrypt.py [--reps 5] [--sizes 1,512,4096,65536] [--impls 1,2] [--distinct 4096] [--step-timeout 280]
                                       [--out profiles/timecrypt_bench.json]
Without --worker this is a driver: every (impl, size) is one child process under `timeout -k 10 <step-timeout>`, chained with `&&`,
so the first step that fails, faults or runs out of time ends the run.  Each step appends one row to --out and prints it.

A step (--worker): scheme Basic, 64-byte messages, host lists through the flat Python calls (all three calls pay the same kind of
staging).  The ciphertexts are sealed with the library itself from public scalars -- u = r g by blsgpu_sign_batch, r by
blsgpu_hash_to_scalar, K = e(sig, u) by blsgpu_pairing_batch, the hashes by hashlib -- at most --distinct of them, repeated to the
size.  After a warm-up of every form, --reps rounds time them alternately (host clock around blocking calls): the group shapes 1 x n
(one signature, n ciphertexts) and n x 1, the pairing values alone, and verify_batch.  Then one more call of each under
blsgpu_profile_enable gives the per-kernel device times.  Reported: median, minimum and maximum per form, whether every ciphertext
opened to its message, and the per-kernel times."""
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


def worker(a):
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    sg, n = a.impl, a.size
    d = min(n, a.distinct)
    xor = lambda x, y: (int.from_bytes(x, 'little') ^ int.from_bytes(y, 'little')).to_bytes(len(x), 'little')  # noqa: E731
    sk = int.from_bytes(hashlib.sha256(b'bench time-lock key %d' % sg).digest(), 'little') >> 2
    ident = b'round 424242'
    pks, sigs = api.sign_batch(sg, api.BASIC, [sk], [ident])
    sig = sigs[0]
    msgs = [hashlib.shake_128(b'm%d' % i).digest(MSG_BYTES) for i in range(d)]
    alphas = [hashlib.sha256(b'a%d' % i).digest() for i in range(d)]
    rs = api.hash_to_scalar([al + hashlib.sha256(m).digest() for al, m in zip(alphas, msgs)], SALT)
    us = api.sign_batch(sg, api.BASIC, rs, [b''] * d)[0]
    ks, st = api.pairing_batch([sig] * d, us) if sg == 1 else api.pairing_batch(us, [sig] * d)
    assert st == [0] * d
    vs = [xor(hashlib.sha256(k).digest(), al) for k, al in zip(ks, alphas)]
    frames = [bytes([MSG_BYTES]) + m for m in msgs]
    ws = [xor(hashlib.shake_128(al).digest(len(f)), f) for al, f in zip(alphas, frames)]
    rep = lambda xs: [xs[i % d] for i in range(n)]  # noqa: E731
    cts = list(zip(rep(us), rep(vs), rep(ws), [api.BASIC] * n))
    one_group = [(sig, api.BASIC, cts)]
    n_groups = [(sig, api.BASIC, [ct]) for ct in cts]
    g1s, g2s = ([sig] * n, rep(us)) if sg == 1 else (rep(us), [sig] * n)
    # the yardstick: n valid (key, signature, message) items of the same impl
    vsks = [sk + 1 + i for i in range(d)]
    vmsgs = [b'verify %d' % i for i in range(d)]
    vpks, vsigs = api.sign_batch(sg, api.BASIC, vsks, vmsgs)
    vpks, vsigs, vmsgs = rep(vpks), rep(vsigs), rep(vmsgs)

    forms = {
        'timecrypt_1xn': lambda: api.timecrypt_open_batch(sg, one_group),
        'timecrypt_nx1': lambda: api.timecrypt_open_batch(sg, n_groups),
        'pairing_batch': lambda: api.pairing_batch(g1s, g2s),
        'verify_batch': lambda: api.verify_batch(sg, api.BASIC, vpks, vsigs, vmsgs),
    }
    got = {k: f() for k, f in forms.items()}                       # warm-up, and the results to check
    opened = got['timecrypt_1xn'] == rep(msgs) and got['timecrypt_nx1'] == rep(msgs)
    values_ok = got['pairing_batch'][0] == rep(ks) and got['verify_batch'] == [0] * n
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
    ms = lambda v: round(v * 1e3, 3)  # noqa: E731
    row = {'impl': 'Bls12381G%dImpl' % sg, 'items': n, 'distinct_ciphertexts': d, 'message_bytes': MSG_BYTES, 'rounds': a.reps,
           'all_opened': opened, 'values_and_verdicts_ok': values_ok}
    for k in forms:
        row[k + '_ms'] = ms(statistics.median(ts[k]))
        row[k + '_min_ms'] = ms(min(ts[k]))
        row[k + '_max_ms'] = ms(max(ts[k]))
    row['kernel_ms_launches'] = prof
    print(json.dumps(row), flush=True)
    rows = []
    if os.path.exists(a.out):
        with open(a.out) as fh:
            rows = json.load(fh)
    with open(a.out, 'w') as fh:
        json.dump(rows + [row], fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='1,512,4096,65536')
    ap.add_argument('--impls', default='1,2')
    ap.add_argument('--distinct', type=int, default=4096)
    ap.add_argument('--step-timeout', type=int, default=280)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'timecrypt_bench.json'))
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--impl', type=int, default=1)
    ap.add_argument('--size', type=int, default=1)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):
        os.remove(a.out)
    q = lambda s: "'" + str(s).replace("'", "'\\''") + "'"  # noqa: E731
    steps = ['timeout -k 10 %d %s %s --worker --impl %d --size %d --reps %d --distinct %d --out %s' %
             (a.step_timeout, q(sys.executable), q(os.path.abspath(__file__)), int(sg), int(n), a.reps, a.distinct, q(a.out))
             for sg in a.impls.split(',') for n in a.sizes.split(',')]
    return subprocess.call(['bash', '-c', ' && '.join(steps)])


if __name__ == '__main__':
    sys.exit(main())
