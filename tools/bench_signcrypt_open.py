#!/usr/bin/env python3
"""Batched threshold signcryption (blsgpu_signcrypt_share_verify_batch + blsgpu_signcrypt_open_batch) against what a caller has
without them: per ciphertext, hash_to_point of U || V, the two-pair check of every share (pairing2_check_batch, the negated hash
repeated per share), signcrypt_valid_batch, combine_shares, serialize, then hashlib.shake_128, the xor and the prefix on the host.

usage: python tools/bench_signcrypt_open.py [--reps 5] [--base-cts 16] [--impls 1,2] [--shapes 0,1,2,3] [--step-timeout 280]
                                            [--out profiles/signcrypt_open_bench.json]
Without --worker this is a driver: every (impl, shape) is one child process under `timeout -k 10 <step-timeout>`, chained with `&&`,
so the first step that fails, faults or runs out of time ends the run.  Each step appends one row to --out and prints it.

A step (--worker): scheme Basic, host lists through the flat Python calls for both forms (both pay the same staging).  Inputs come
from public scalars: u = r g, the key G = (s0 r) g, w = r H(U || V) and the shares (f(i) r) g by blsgpu_sign_batch, v by
hashlib.shake_128.  After a warm-up of both forms, --reps rounds time them alternately: the two batched calls over all
ciphertexts, then the loop over --base-cts ciphertexts taken at even distances (scaled to all by count).  Reported: median, minimum
and maximum for both forms, whether plaintexts and verdicts agree, the per-kernel device time of one more batched open
(blsgpu_profile_enable), and -- for pricing the one-lane squeeze -- the keystream kernel's and the host's SHAKE128 time per MiB."""
import argparse
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
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
SHAPES = [('1,024 x 8 shares, 32 B', 1024, 8, 32), ('1,024 x 64 shares, 32 B', 1024, 64, 32), ('16 x 1,024 shares, 32 B', 16, 1024, 32),
          ('64 x 2 shares, 64 KiB', 64, 2, 65536)]


def varint(n):
    out = bytearray()
    while True:
        b, n = n & 0x7f, n >> 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def negate(group, raw):
    """-P of a RAW_PROJ point: Montgomery form is linear, so each Fp word of Y becomes p - word."""
    w = 48 * group
    y = b''.join(((P - int.from_bytes(raw[w + 48 * k:w + 48 * k + 48], 'little')) % P).to_bytes(48, 'little') for k in range(group))
    return raw[:w] + y + raw[2 * w:]


def worker(a):
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    sg, pkg = a.impl, 3 - a.impl
    name, n_ct, t, mlen = SHAPES[a.shape]
    rng = random.Random(99 + sg)
    s0, s1 = rng.randrange(1, R), rng.randrange(1, R)
    f = lambda x: (s0 + s1 * x) % R
    rs = [rng.randrange(1, R) for _ in range(n_ct)]
    pts = lambda ks: api.sign_batch(sg, api.BASIC, ks, [b''] * len(ks))[0]
    us = pts(rs)
    gb = api.serialize(pkg, pts([s0 * r % R for r in rs]))
    msgs = [bytes((c + j) & 0xff for j in range(mlen)) for c in range(n_ct)]
    frames = [varint(mlen) + m for m in msgs]
    xor = lambda x, y: (int.from_bytes(x, 'little') ^ int.from_bytes(y, 'little')).to_bytes(len(x), 'little')
    vs = [xor(hashlib.shake_128(g).digest(len(fr)), fr) for g, fr in zip(gb, frames)]
    ub = api.serialize(pkg, us)
    ws = api.sign_batch(sg, api.BASIC, rs, [b + v for b, v in zip(ub, vs)])[1]
    ids = list(range(1, t + 1))
    pk_sh = pts([f(i) for i in ids])
    sh = pts([f(i) * r % R for r in rs for i in ids])
    cts = list(zip(us, vs, ws))
    vsh = [[(sh[c * t + k], pk_sh[k]) for k in range(t)] for c in range(n_ct)]
    osh = [[(ids[k], sh[c * t + k]) for k in range(t)] for c in range(n_ct)]
    dst = api.DST[(sg, api.BASIC)]

    def batched():
        return api.signcrypt_share_verify_batch(sg, api.BASIC, cts, vsh), api.signcrypt_open_batch(sg, api.BASIC, cts, osh)

    def one(c):
        u, v, w = cts[c]
        nh = negate(sg, api.hash_to_point(sg, [ub[c] + v], dst)[0])
        if sg == 1:
            ok = api.pairing2_check_batch([nh] * t, [s for s, _ in vsh[c]], [w] * t, [p for _, p in vsh[c]])
        else:
            ok = api.pairing2_check_batch([s for s, _ in vsh[c]], [nh] * t, [p for _, p in vsh[c]], [w] * t)
        valid = api.signcrypt_valid_batch(sg, api.BASIC, [u], [w], [v])[0]
        key, _ = api.combine_shares(pkg, [[(i, p, None) for i, p in osh[c]]])
        fr = xor(hashlib.shake_128(api.serialize(pkg, key)[0]).digest(len(v)), v)
        n = k = 0
        while fr[k] & 0x80:
            n |= (fr[k] & 0x7f) << (7 * k)
            k += 1
        n |= fr[k] << (7 * k)
        return ok, fr[k + 1:k + 1 + n] if valid else None

    bs = min(n_ct, a.base_cts)
    base = [c * n_ct // bs for c in range(bs)]
    got = batched()
    loop = [one(c) for c in base[:2]]
    ts, bts = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = batched()
        ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        loop = [one(c) for c in base]
        bts.append((time.perf_counter() - t0) * n_ct / bs)
    api.profile_enable(True)
    api.signcrypt_open_batch(sg, api.BASIC, cts, osh)
    prof = {k: [round(v[0], 3), v[1]] for k, v in api.profile_read().items()}
    api.profile_enable(False)
    t0 = time.perf_counter()
    for g, v in zip(gb, vs):
        hashlib.shake_128(g).digest(len(v))
    host_shake = time.perf_counter() - t0
    mib = sum(len(v) for v in vs) / 2 ** 20
    ms = lambda v: round(v * 1e3, 3)
    agree = all(got[0][c] == [0 if o else 14 for o in loop[j][0]] for j, c in enumerate(base)) and \
        all(got[1][c] == loop[j][1] == msgs[c] for j, c in enumerate(base))
    row = {'impl': 'Bls12381G%dImpl' % sg, 'shape': name, 'ciphertexts': n_ct, 'shares_each': t, 'message_bytes': mlen,
           'batched_ms': ms(statistics.median(ts)), 'batched_min_ms': ms(min(ts)), 'batched_max_ms': ms(max(ts)),
           'loop_ms': ms(statistics.median(bts)), 'loop_min_ms': ms(min(bts)), 'loop_max_ms': ms(max(bts)), 'loop_ciphertexts_timed': bs,
           'speedup': round(statistics.median(bts) / statistics.median(ts), 2), 'results_match_loop': agree,
           'all_opened': all(p == m for p, m in zip(got[1], msgs)), 'kernel_ms_launches': prof,
           'keystream_kernel_ms_per_MiB': round(prof.get('k_signcrypt_keystream', [0, 0])[0] / mib, 3), 'host_shake128_ms_per_MiB': round(host_shake * 1e3 / mib, 3),
           'rounds': a.reps}
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
    ap.add_argument('--base-cts', type=int, default=16)
    ap.add_argument('--impls', default='1,2')
    ap.add_argument('--shapes', default='0,1,2,3')
    ap.add_argument('--step-timeout', type=int, default=280)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'signcrypt_open_bench.json'))
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--impl', type=int, default=1)
    ap.add_argument('--shape', type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):
        os.remove(a.out)
    q = lambda s: "'" + str(s).replace("'", "'\\''") + "'"
    steps = ['timeout -k 10 %d %s %s --worker --impl %d --shape %d --reps %d --base-cts %d --out %s' %
             (a.step_timeout, q(sys.executable), q(os.path.abspath(__file__)), int(sg), int(sh), a.reps, a.base_cts, q(a.out))
             for sg in a.impls.split(',') for sh in a.shapes.split(',')]
    return subprocess.call(['bash', '-c', ' && '.join(steps)])


if __name__ == '__main__':
    sys.exit(main())
