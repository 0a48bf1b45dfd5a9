#!/usr/bin/env python3
"""Batched verify_secure throughput (blsgpu_verify_secure_batch) against what a caller has without it: one blsgpu_verify_secure
call per set.

usage: python tools/bench_secure_batch.py [--reps 5] [--base-sets 32] [--out profiles/secure_batch_bench.json]
Inputs live on the device (TensorOps) for both forms, so neither pays host staging.  Keys are drawn from a pool of 65,536
distinct k * g (blsgpu_sign_batch), signatures from a pool of 4,096; the verdicts are mostly INVALID_SIGNATURE, which costs
the same as OK (every set runs the whole sort, digest, sum and pairing check).  The batched time is the median of --reps
calls; the last shape (16 sets of 2,048 keys) is there to place BLSGPU_SECURE_BATCH_MAX.  The baseline times the first --base-sets sets one call each and scales per set.  The one-set shape compares the
batched call with blsgpu_verify_secure on the same 65,536 keys.  Prints one JSON line per shape and writes them all to --out."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KEY_POOL, SIG_POOL = 65536, 4096
SHAPES = [('Bls12381G2Impl Modern', 2, 1024, 400), ('Bls12381G2Impl Modern', 2, 4096, 50), ('Bls12381G1Impl', 1, 256, 400),
          ('Bls12381G2Impl one large set', 2, 1, 65536), ('Bls12381G2Impl sets at twice the default knob', 2, 16, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--base-sets', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'secure_batch_bench.json'))
    ap.add_argument('--shapes', default='')
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    rng = random.Random(2026)
    pools = {}
    for sg in (1, 2):
        ks = [rng.randrange(1, R) for _ in range(KEY_POOL)]
        pks = api.sign_batch(sg, api.BASIC, ks, [b''] * KEY_POOL)[0]
        sigs = api.sign_batch(sg, api.BASIC, ks[:SIG_POOL], [b'bench'] * SIG_POOL)[1]
        pools[sg] = (torch.tensor(list(b''.join(pks)), dtype=torch.uint8, device=dev).view(KEY_POOL, -1),
                     torch.tensor(list(b''.join(sigs)), dtype=torch.uint8, device=dev).view(SIG_POOL, -1))
    rows = []
    shapes = [SHAPES[int(i)] for i in a.shapes.split(',')] if a.shapes else SHAPES
    for name, sg, n_sets, t in shapes:
        n = n_sets * t
        gen = torch.Generator(device=dev).manual_seed(n)
        sel = torch.randperm(KEY_POOL, device=dev, generator=gen) if n == KEY_POOL else torch.randint(0, KEY_POOL, (n,), device=dev, generator=gen)
        pks_t = pools[sg][0][sel].reshape(-1).contiguous()
        ssel = torch.randint(0, SIG_POOL, (n_sets,), device=dev, generator=gen)
        sigs_t = pools[sg][1][ssel].reshape(-1).contiguous()
        msgs = [b'quorum commitment %06d' % s for s in range(n_sets)]
        moffs, mblob = api._offsets(msgs)
        msgs_t = torch.tensor(list(mblob), dtype=torch.uint8, device=dev)
        moffs_t = torch.tensor(list(moffs), dtype=torch.int64, device=dev)
        koffs_t = torch.arange(0, n + 1, t, dtype=torch.int64, device=dev)
        run = lambda: ops.verify_secure_batch(sg, api.BASIC, pks_t, koffs_t, sigs_t, msgs_t, moffs_t, n_sets)
        st = run()                                                           # warm-up (workspace growth)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            st = run()
            ts.append(time.perf_counter() - t0)
        batched = statistics.median(ts)
        api.profile_enable(True)
        run()
        prof = {k: round(v[0], 3) for k, v in api.profile_read().items()}
        api.profile_enable(False)
        # baseline: one blsgpu_verify_secure call per set on the same device-resident inputs
        bs = min(n_sets, a.base_sets)
        psz, ssz = pks_t.numel() // n, sigs_t.numel() // n_sets
        stb = ops.empty(4 * bs)
        one = lambda s: api._check(ops.lib.blsgpu_verify_secure(sg, api.BASIC, ctypes.c_void_p(pks_t.data_ptr() + s * t * psz), t,
                                                                ctypes.c_void_p(sigs_t.data_ptr() + s * ssz), api._ptr(msgs[s]), len(msgs[s]),
                                                                api.MODERN, api.FMT_RAW_PROJ, ctypes.c_void_p(stb.data_ptr() + 4 * s)))
        for s in range(min(bs, 2)):                                          # warm-up
            one(s)
        torch.cuda.synchronize()
        bts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for s in range(bs):
                one(s)
            bts.append((time.perf_counter() - t0) * n_sets / bs)
        baseline = statistics.median(bts)
        same = stb.view(torch.int32)[:bs].cpu().tolist() == st[:bs].cpu().tolist()
        row = {'shape': name, 'sig_group': sg, 'sets': n_sets, 'keys_per_set': t, 'batched_ms': round(batched * 1e3, 3),
               'batched_sets_per_s': round(n_sets / batched, 1), 'baseline_ms': round(baseline * 1e3, 3),
               'baseline_sets_per_s': round(n_sets / baseline, 1), 'baseline_sets_timed': bs, 'speedup': round(baseline / batched, 2),
               'statuses_match_single_call': same, 'status_counts': {str(k): v for k, v in zip(*[x.tolist() for x in st.cpu().unique(return_counts=True)])},
               'kernel_ms': prof, 'reps': a.reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
