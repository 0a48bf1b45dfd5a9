#!/usr/bin/env python3
"""The signcryption share check by key index (blsgpu_signcrypt_share_verify_indexed_batch) against the by-value call, three versions on
the same seeded inputs:
    byvalue_parent   blsgpu_signcrypt_share_verify_batch of the PARENT commit (--parent-root: a checkout of it, built)
    indexed_plain    the indexed call without tables: BLSGPU_SIGNCRYPT_LINES_MIN=0 and a key set without line rows
    indexed_tables   the indexed call with tables: BLSGPU_SIGNCRYPT_LINES_MIN=1 and, for Bls12381G1Impl, a key set with line rows

usage: python tools/bench_signcrypt_indexed.py --parent-root DIR [--reps 5] [--passes 2] [--impls 1,2] [--shapes 0,1,2,3,4]
                                               [--step-timeout 280] [--out profiles/signcrypt_indexed_bench.json]
Knobs and the library are per process, so every version is a worker process of its own (three at a time; each under
`timeout -k 10 <step-timeout>`).  The driver lets the three warm up (two calls each), then times them ALTERNATELY, one call each per
round, --reps rounds: what drifts over the run drifts for all three.  A pass is that whole procedure; --passes 2 repeats it with fresh
workers -- the same command run twice -- and the row reports each pass's medians and the spread between the passes.  The first worker
that fails, faults or runs out of time ends the run: nothing further is started.

A call is timed at the C interface with host pointers, as a caller in another language pays it: the by-value form ships a key share
with every decryption share, the indexed forms four bytes.  Inputs come from public scalars (blsgpu_sign_batch): a committee of t
members, n_ct ciphertexts of t shares each, 1 % of the shares replaced by the next member's.  After the rounds every worker runs one
more call under the in-library profile (per-kernel device time and launches) and reports its statuses, which must be identical in the
three versions and equal to the tamper pattern."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SHAPES = [(64, 32), (256, 16), (4096, 4), (1024, 64), (16384, 1)]          # ciphertexts x shares each
VERSIONS = ('byvalue_parent', 'indexed_plain', 'indexed_tables')


def worker(a):
    if a.version == 'byvalue_parent':
        sys.path.insert(0, os.path.abspath(a.parent_root))     # the parent's package and library, not this tree's
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    lib = api.init()
    sg = a.impl
    n_ct, t = SHAPES[a.shape]
    n = n_ct * t
    rng = random.Random(1000 * sg + a.shape)
    s0, s1 = rng.randrange(1, R), rng.randrange(1, R)
    f = lambda x: (s0 + s1 * x) % R
    rs = [rng.randrange(1, R) for _ in range(n_ct)]
    pts = lambda ks: api.sign_batch(sg, api.BASIC, ks, [b''] * len(ks))[0]
    us = pts(rs)
    vs = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(n_ct)]
    ub = api.serialize(3 - sg, us)
    ws = api.sign_batch(sg, api.BASIC, rs, [b + v for b, v in zip(ub, vs)])[1]
    members = t + 1                                            # one more than a ciphertext names: a tamper can name "the next member"
    pk_sh = pts([f(i + 1) for i in range(members)])
    tampered = [rng.random() < 0.01 for _ in range(n)]
    scal = [f((k + 1 if tampered[c * t + k] else k) + 1) * rs[c] % R for c in range(n_ct) for k in range(t)]
    sh = pts(scal)
    want = [14 if x else 0 for x in tampered]
    p = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)
    u64 = lambda xs: (ctypes.c_uint64 * len(xs))(*xs)
    ublob, wblob, vblob, shblob = b''.join(us), b''.join(ws), b''.join(vs), b''.join(sh)
    voffs, soffs = u64([32 * c for c in range(n_ct + 1)]), u64([t * c for c in range(n_ct + 1)])
    st = (ctypes.c_int32 * n)()
    keep = [ublob, wblob, vblob, shblob]
    if a.version == 'byvalue_parent':
        pkblob = b''.join(pk_sh[k] for _ in range(n_ct) for k in range(t))
        keep.append(pkblob)

        def call():
            return lib.blsgpu_signcrypt_share_verify_batch(sg, api.BASIC, p(ublob), p(wblob), p(vblob), ctypes.cast(voffs, ctypes.c_void_p), n_ct, p(shblob),
                                                           p(pkblob), ctypes.cast(soffs, ctypes.c_void_p), api.FMT_RAW_PROJ, ctypes.cast(st, ctypes.c_void_p))
        ks = None
    else:
        ks = api.KeySet.create(sg, pk_sh, api.FMT_RAW_PROJ, lines=(a.version == 'indexed_tables' and sg == 1))
        idx = (ctypes.c_uint32 * n)(*[k for _ in range(n_ct) for k in range(t)])

        def call():
            return lib.blsgpu_signcrypt_share_verify_indexed_batch(api.BASIC, ks.handle, ctypes.cast(idx, ctypes.c_void_p), p(ublob), p(wblob), p(vblob),
                                                                   ctypes.cast(voffs, ctypes.c_void_p), n_ct, p(shblob), ctypes.cast(soffs, ctypes.c_void_p),
                                                                   api.FMT_RAW_PROJ, ctypes.cast(st, ctypes.c_void_p))
    for _ in range(2):                                         # warm up: the arena, the line workspace, the code objects
        assert call() == 0
    print('ready', flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == 'go':
            t0 = time.perf_counter()
            rc = call()
            dt = time.perf_counter() - t0
            assert rc == 0
            print('t %.6f' % (dt * 1e3), flush=True)
        elif cmd == 'prof':
            api.profile_enable(True)
            assert call() == 0
            prof = {k: [round(v[0], 3), v[1]] for k, v in api.profile_read().items() if v[1]}
            api.profile_enable(False)
            flat = list(st)
            print('p ' + json.dumps({'kernel_ms_launches': prof, 'status_sha256': hashlib.sha256(bytes(x & 0xff for x in flat)).hexdigest(),
                                     'not_ok': sum(1 for x in flat if x), 'equals_tamper_pattern': flat == want,
                                     'set': ks.info() if ks else None}), flush=True)
        else:
            break
    if ks:
        ks.close()


def one_pass(a, sg, shape):
    """three fresh workers, warmed up, timed alternately; None when one of them failed"""
    procs = []
    try:
        for v in VERSIONS:
            env = {k: x for k, x in os.environ.items() if not k.startswith('BLSGPU_')}
            if v != 'byvalue_parent':
                env['BLSGPU_SIGNCRYPT_LINES_MIN'] = '1' if v == 'indexed_tables' else '0'
            cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--worker', '--version', v, '--impl', str(sg),
                   '--shape', str(shape), '--parent-root', a.parent_root]
            pr = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            procs.append(pr)
            if pr.stdout.readline().strip() != 'ready':
                return None
        times = {v: [] for v in VERSIONS}
        for _ in range(a.reps):
            for v, pr in zip(VERSIONS, procs):
                pr.stdin.write('go\n')
                pr.stdin.flush()
                ans = pr.stdout.readline().split()
                if len(ans) != 2 or ans[0] != 't':
                    return None
                times[v].append(float(ans[1]))
        info = {}
        for v, pr in zip(VERSIONS, procs):                     # the profiled call: a run of its own, after every timed one
            pr.stdin.write('prof\n')
            pr.stdin.flush()
            ans = pr.stdout.readline()
            if not ans.startswith('p '):
                return None
            info[v] = json.loads(ans[2:])
        return times, info
    finally:
        for pr in procs:
            try:
                pr.stdin.write('quit\n')
                pr.stdin.flush()
                pr.stdin.close()
            except (BrokenPipeError, ValueError):
                pass
        for pr in procs:
            pr.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-root', default='')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--impls', default='1,2')
    ap.add_argument('--shapes', default='0,1,2,3,4')
    ap.add_argument('--step-timeout', type=int, default=280)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'signcrypt_indexed_bench.json'))
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--version', default='indexed_plain')
    ap.add_argument('--impl', type=int, default=1)
    ap.add_argument('--shape', type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not os.path.exists(os.path.join(a.parent_root, 'agora-blsful_amd', 'libblsgpu.so')):
        sys.exit('--parent-root: a built checkout of the parent commit is needed for the by-value version')
    if a.reps < 3:
        sys.exit('--reps: at least three')
    rows = []
    ms = lambda x: round(x, 3)
    for sg in (int(x) for x in a.impls.split(',')):
        for shape in (int(x) for x in a.shapes.split(',')):
            n_ct, t = SHAPES[shape]
            row = {'impl': 'Bls12381G%dImpl' % sg, 'ciphertexts': n_ct, 'shares_each': t, 'shares': n_ct * t, 'rounds': a.reps, 'passes': []}
            for _ in range(a.passes):
                res = one_pass(a, sg, shape)
                if res is None:
                    print('a worker failed at', row, file=sys.stderr)
                    return 1
                times, info = res
                row['passes'].append({v: {'median_ms': ms(statistics.median(times[v])), 'min_ms': ms(min(times[v])), 'max_ms': ms(max(times[v]))} for v in VERSIONS})
                row['profile'] = info
            med = {v: [ps[v]['median_ms'] for ps in row['passes']] for v in VERSIONS}
            row['median_ms'] = {v: ms(statistics.median(med[v])) for v in VERSIONS}
            row['spread_between_passes'] = {v: round((max(med[v]) - min(med[v])) / min(med[v]), 4) for v in VERSIONS}
            row['tables_vs_plain'] = round(row['median_ms']['indexed_plain'] / row['median_ms']['indexed_tables'], 3)
            row['plain_vs_byvalue'] = round(row['median_ms']['byvalue_parent'] / row['median_ms']['indexed_plain'], 3)
            row['statuses_identical'] = len({info[v]['status_sha256'] for v in VERSIONS}) == 1 and all(info[v]['equals_tamper_pattern'] for v in VERSIONS)
            print(json.dumps({k: v for k, v in row.items() if k != 'profile'}), flush=True)
            rows.append(row)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(rows, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
