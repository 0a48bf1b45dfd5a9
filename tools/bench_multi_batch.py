#!/usr/bin/env python3
"""Batched multi verify (blsgpu_multi_verify_batch) against what a caller has without it: one blsgpu_multi_verify call per set.

usage: python tools/bench_multi_batch.py [--reps 7] [--base-sets 64] [--impls 1,2] [--shapes 0,1,2,3] [--step-timeout 240]
                                         [--out profiles/multi_batch_bench.json]
Without --worker this is a driver: every (impl, shape) is one child process of its own under `timeout -k 10 <step-timeout>`, and
the steps are chained with `&&`, so the first one that fails, faults or runs out of time ends the run.  Each step appends one row
to --out and prints it as a JSON line.

A step (--worker): scheme Basic, inputs on the device (TensorOps) for both forms, so neither pays host staging.  Keys are drawn
from a pool of 65,536 distinct k g (blsgpu_sign_batch); the signature of a set is made for the sum of its secrets, so every
non-empty set verifies (empty sets, in the ragged shape, get the identity signature).  After a warm-up of both forms, --reps
rounds time them alternately: the batched call repeated until the window is at least 0.1 s (time per call), then the loop of
single calls over --base-sets sets taken at even distances through the list (scaled to all sets by key count).  Both forms return
after a device synchronise.  The loop is code this entry point does not change: it stands for the library before it.  Reported:
median, minimum and maximum of the rounds for both forms, whether the statuses agree, and -- from one more batched call with
blsgpu_profile_enable on -- the device time and launch count per kernel."""
import argparse
import ctypes
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
KEY_POOL = 65536
SHAPES = [('1,024 x 512', 1024, 512), ('64 x 16,384', 64, 16384), ('16,384 x 8', 16384, 8), ('ragged', 2048, None)]


def set_sizes(n_sets, t):
    """Equal sets of t keys; t = None: 2,048 sets of 1 to 4,095 keys, log-uniform, every 64th one empty."""
    if t is not None:
        return [t] * n_sets
    rng = random.Random(7)
    return [0 if s % 64 == 63 else int(2 ** rng.uniform(0, 12)) for s in range(n_sets)]


def worker(a):
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sg = a.impl
    name, n_sets, t = SHAPES[a.shape]
    sizes = set_sizes(n_sets, t)
    n = sum(sizes)
    rng = random.Random(2026 + sg)
    ks = [rng.randrange(1, R) for _ in range(KEY_POOL)]
    tens = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    pool = tens(b''.join(api.sign_batch(sg, api.BASIC, ks, [b''] * KEY_POOL)[0])).view(KEY_POOL, -1)
    sel = [rng.randrange(KEY_POOL) for _ in range(n)]
    pks_t = pool[torch.tensor(sel, dtype=torch.int64, device=dev)].reshape(-1).contiguous()
    koffs = [0]
    for q in sizes:
        koffs.append(koffs[-1] + q)
    msgs = [b'committee attestation %06d' % s for s in range(n_sets)]
    sks = [sum(ks[i] for i in sel[koffs[s]:koffs[s + 1]]) % R for s in range(n_sets)]
    live = [s for s in range(n_sets) if sks[s]]
    made = api.sign_batch(sg, api.BASIC, [sks[s] for s in live], [msgs[s] for s in live])[1]
    ssz = 144 if sg == 1 else 288
    sig_list = [bytes(ssz)] * n_sets
    for s, sig in zip(live, made):
        sig_list[s] = sig
    sigs_t = tens(b''.join(sig_list))
    moffs, mblob = api._offsets(msgs)
    msgs_t = tens(mblob)
    moffs_t = torch.tensor(list(moffs), dtype=torch.int64, device=dev)
    koffs_t = torch.tensor(koffs, dtype=torch.int64, device=dev)
    psz = pks_t.numel() // n
    run = lambda: ops.multi_verify_batch(sg, api.BASIC, pks_t, koffs_t, sigs_t, msgs_t, moffs_t, n_sets)
    bs = min(n_sets, a.base_sets)
    base = [s * n_sets // bs for s in range(bs)]
    base_keys = sum(sizes[s] for s in base)
    stb = torch.full((n_sets,), -99, dtype=torch.int32, device=dev)

    def one(s):
        rc = ops.lib.blsgpu_multi_verify(sg, api.BASIC, ctypes.c_void_p(pks_t.data_ptr() + koffs[s] * psz), sizes[s],
                                         ctypes.c_void_p(sigs_t.data_ptr() + s * ssz), api._ptr(msgs[s]), len(msgs[s]), api.FMT_RAW_PROJ,
                                         ctypes.c_void_p(stb.data_ptr() + 4 * s))
        assert rc == 0, rc

    torch.cuda.synchronize()
    st = run()                                                               # warm-up of both forms (workspace growth, code objects)
    t0 = time.perf_counter()
    st = run()
    inner = max(1, int(0.1 / max(time.perf_counter() - t0, 1e-6)) + 1)
    for s in base[:4]:
        one(s)
    ts, bts = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            st = run()
        ts.append((time.perf_counter() - t0) / inner)
        t0 = time.perf_counter()
        for s in base:
            one(s)
        bts.append((time.perf_counter() - t0) * (n / base_keys if t is None else n_sets / bs))
    api.profile_enable(True)
    run()
    prof = {k: [round(v[0], 3), v[1]] for k, v in api.profile_read().items()}
    api.profile_enable(False)
    got = st.cpu().tolist()
    single = stb.cpu().tolist()
    ms = lambda v: round(v * 1e3, 3)
    row = {'impl': 'Bls12381G%dImpl' % sg, 'shape': name, 'sets': n_sets, 'keys': n, 'largest_set': max(sizes), 'empty_sets': sizes.count(0),
           'strip_knob': os.environ.get('BLSGPU_MULTI_STRIP', 'default'),
           'batched_ms': ms(statistics.median(ts)), 'batched_min_ms': ms(min(ts)), 'batched_max_ms': ms(max(ts)), 'batched_calls_per_round': inner,
           'loop_ms': ms(statistics.median(bts)), 'loop_min_ms': ms(min(bts)), 'loop_max_ms': ms(max(bts)), 'loop_sets_timed': bs,
           'loop_scaled_by': 'keys' if t is None else 'sets', 'speedup': round(statistics.median(bts) / statistics.median(ts), 2),
           'statuses_match_single_call': all(got[s] == single[s] for s in base),
           'status_counts': {str(k): got.count(k) for k in sorted(set(got))}, 'kernel_ms_launches': prof, 'rounds': a.reps}
    print(json.dumps(row), flush=True)
    rows = []
    if os.path.exists(a.out):
        with open(a.out) as f:
            rows = json.load(f)
    with open(a.out, 'w') as f:
        json.dump(rows + [row], f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--base-sets', type=int, default=64)
    ap.add_argument('--impls', default='1,2')
    ap.add_argument('--shapes', default='0,1,2,3')
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_batch_bench.json'))
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
    steps = ['timeout -k 10 %d %s %s --worker --impl %d --shape %d --reps %d --base-sets %d --out %s' %
             (a.step_timeout, q(sys.executable), q(os.path.abspath(__file__)), int(sg), int(sh), a.reps, a.base_sets, q(a.out))
             for sg in a.impls.split(',') for sh in a.shapes.split(',')]
    return subprocess.call(['bash', '-c', ' && '.join(steps)])


if __name__ == '__main__':
    sys.exit(main())
