#!/usr/bin/env python3
"""Batched aggregation (blsgpu_aggregate_secure_batch, blsgpu_sum_batch) against what a caller has without it: one
blsgpu_aggregate_secure, or one blsgpu_sum_g1 / blsgpu_sum_g2, call per set.

usage: python tools/bench_aggregate_batch.py [--reps 7] [--base-sets 64] [--impls 1,2] [--shapes 0,1,2,3] [--step-timeout 240]
                                             [--out profiles/aggregate_batch_bench.json]
Without --worker this is a driver: every (impl, shape) is one child process of its own under `timeout -k 10 <step-timeout>`, and
the steps are chained with `&&`, so the first one that fails, faults or runs out of time ends the run.  Each step appends one row
to --out and prints it as a JSON line.

A step (--worker): inputs and outputs on the device (TensorOps) for every form, so none pays host staging.  Keys k g and signatures
k H(m) come from a pool of 65,536 secrets (blsgpu_sign_batch); a set draws its members without repetition, so no set holds a
duplicate key (the single call sorts again on every byte when its prefix sort ties).  After a warm-up of every form, --reps rounds
time them alternately: the batched call repeated until the window is at least 0.1 s (time per call), then the loop of single
calls over --base-sets sets taken at even distances through the list (scaled to all sets by key count).  Every form returns after
a device synchronise.  The loops are code these entry points do not change: they stand for the library before them.  Reported per
pair of forms: median, minimum and maximum of the rounds, whether the serialised results agree on the sets the loop ran, and --
from one more batched call with blsgpu_profile_enable on -- the device time and launch count per kernel."""
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
SHAPES = [('1,024 x 64', 1024, 64), ('256 x 400', 256, 400), ('16,384 x 8', 16384, 8), ('ragged', 2048, None)]


def set_sizes(n_sets, t):
    """Equal sets of t keys; t = None: 2,048 sets of 0 to 1,100 keys, uniform."""
    if t is not None:
        return [t] * n_sets
    rng = random.Random(7)
    return [rng.randrange(0, 1101) for _ in range(n_sets)]


def timed(run, one, base, scale, reps):
    """rounds of (batched call, loop of single calls), alternating -> (batched seconds per call, scaled loop seconds, calls per window)"""
    run()
    t0 = time.perf_counter()
    run()
    inner = max(1, int(0.1 / max(time.perf_counter() - t0, 1e-6)) + 1)
    for s in base[:4]:
        one(s)
    ts, bts = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            run()
        ts.append((time.perf_counter() - t0) / inner)
        t0 = time.perf_counter()
        for s in base:
            one(s)
        bts.append((time.perf_counter() - t0) * scale)
    return ts, bts, inner


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
    pk_list, sig_list = api.sign_batch(sg, api.BASIC, ks, [b'quorum commitment'] * KEY_POOL)
    pk_pool, sig_pool = tens(b''.join(pk_list)).view(KEY_POOL, -1), tens(b''.join(sig_list)).view(KEY_POOL, -1)
    sel = [i for q in sizes for i in rng.sample(range(KEY_POOL), q)]
    sel_t = torch.tensor(sel, dtype=torch.int64, device=dev)
    pks_t, sigs_t = pk_pool[sel_t].reshape(-1).contiguous(), sig_pool[sel_t].reshape(-1).contiguous()
    koffs = [0]
    for q in sizes:
        koffs.append(koffs[-1] + q)
    koffs_t = torch.tensor(koffs, dtype=torch.int64, device=dev)
    psz, ssz = pks_t.numel() // n, sigs_t.numel() // n
    bs = min(n_sets, a.base_sets)
    base = [s * n_sets // bs for s in range(bs)]
    scale = n / sum(sizes[s] for s in base) if t is None else n_sets / bs
    out1 = torch.zeros(n_sets * ssz, dtype=torch.uint8, device=dev)
    st1 = torch.full((n_sets,), -99, dtype=torch.int32, device=dev)
    sum_fn = ops.lib.blsgpu_sum_g1 if sg == 1 else ops.lib.blsgpu_sum_g2
    P = lambda tsr, off=0: ctypes.c_void_p(tsr.data_ptr() + off)

    def one_secure(s):
        rc = ops.lib.blsgpu_aggregate_secure(sg, P(pks_t, koffs[s] * psz), P(sigs_t, koffs[s] * ssz), sizes[s], api.MODERN, api.FMT_RAW_PROJ,
                                             P(out1, s * ssz), P(st1, 4 * s))
        assert rc == 0, rc

    def one_sum(s):
        rc = sum_fn(P(sigs_t, koffs[s] * ssz), sizes[s], api.FMT_RAW_PROJ, P(out1, s * ssz))
        assert rc == 0, rc

    res = {}
    run_secure = lambda: res.__setitem__('secure', ops.aggregate_secure_batch(sg, pks_t, sigs_t, koffs_t, n_sets))
    run_sum = lambda: res.__setitem__('sum', ops.sum_batch(sg, sigs_t, koffs_t, n_sets))
    torch.cuda.synchronize()
    ms = lambda v: round(v * 1e3, 3)
    row = {'impl': 'Bls12381G%dImpl' % sg, 'shape': name, 'sets': n_sets, 'keys': n, 'largest_set': max(sizes), 'empty_sets': sizes.count(0),
           'secure_batch_max': os.environ.get('BLSGPU_SECURE_BATCH_MAX', 'default'), 'strip_knob': os.environ.get('BLSGPU_MULTI_STRIP', 'default'),
           'loop_sets_timed': bs, 'loop_scaled_by': 'keys' if t is None else 'sets', 'rounds': a.reps}
    for what, run, one in (('secure', run_secure, one_secure), ('sum', run_sum, one_sum)):
        ts, bts, inner = timed(run, one, base, scale, a.reps)
        batched = res[what][0] if what == 'secure' else res[what]
        same = all(bytes(ops.serialize(sg, batched[s * ssz:(s + 1) * ssz], 1).cpu().tolist()) == bytes(ops.serialize(sg, out1[s * ssz:(s + 1) * ssz], 1).cpu().tolist())
                   for s in base)
        api.profile_enable(True)
        run()
        prof = {k: [round(v[0], 3), v[1]] for k, v in api.profile_read().items()}
        api.profile_enable(False)
        row[what] = {'batched_ms': ms(statistics.median(ts)), 'batched_min_ms': ms(min(ts)), 'batched_max_ms': ms(max(ts)), 'batched_calls_per_round': inner,
                     'loop_ms': ms(statistics.median(bts)), 'loop_min_ms': ms(min(bts)), 'loop_max_ms': ms(max(bts)),
                     'speedup': round(statistics.median(bts) / statistics.median(ts), 2), 'results_match_single_call': same, 'kernel_ms_launches': prof}
        if what == 'secure':
            sts = res[what][1].cpu().tolist()
            row[what]['status_counts'] = {str(k): sts.count(k) for k in sorted(set(sts))}
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'aggregate_batch_bench.json'))
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
