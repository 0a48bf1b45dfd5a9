#!/usr/bin/env python3
"""Threshold recovery throughput (blsgpu_combine_shares) against what a caller has without it: one blsgpu_msm_* call per set.

usage: python tools/bench_shares.py [--reps 5] [--out profiles/shares_bench.json]
Inputs live on the device (TensorOps) for both forms, so neither pays host staging.  The points are a pool of 4,096 distinct
k * g (blsgpu_sign_batch) reused across sets; identifiers are random 255-bit values, distinct within a set.
The baseline is timed on its MSM calls alone, with random 255-bit scalars in place of the coefficients (the MSM's cost does not
depend on their values): the host-side Lagrange a real caller would also run is NOT charged to it, so the baseline is a lower
bound.  For the many-set shapes the baseline times the first `--base-sets` sets and scales per set.
Prints one JSON line per shape and writes them all to --out."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
POOL = 4096
SHAPES = [('G2 signatures (Bls12381G2Impl)', 2, 4096, 240), ('G2 signatures (Bls12381G2Impl)', 2, 65536, 3),
          ('G1 public keys (Bls12381G2Impl)', 1, 4096, 240), ('G2 one large set', 2, 1, 4096)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--base-sets', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shares_bench.json'))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    rng = random.Random(2024)
    pools = {}
    for g in (1, 2):
        ks = [rng.randrange(1, R) for _ in range(POOL)]
        pts = api.sign_batch(3 - g, api.BASIC, ks, [b''] * POOL)[0]
        pools[g] = torch.tensor(list(b''.join(pts)), dtype=torch.uint8, device=dev).view(POOL, -1)
    rows = []
    for name, g, n_sets, t in SHAPES:
        n = n_sets * t
        ids = bytearray()
        for s in range(n_sets):
            for x in rng.sample(range(1, 1 << 62), t):      # distinct within the set; spread over the full width below
                ids += ((x * 0x9e3779b97f4a7c15 << 190 | x) % R).to_bytes(32, 'little')
        ids_t = torch.tensor(list(ids), dtype=torch.uint8, device=dev)
        sel = torch.randint(0, POOL, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(n))
        pts_t = pools[g][sel].reshape(-1).contiguous()
        offs_t = torch.arange(0, n + 1, t, dtype=torch.int64, device=dev)
        ops.combine_shares(g, ids_t, pts_t, None, offs_t, n_sets)          # warm-up (workspace growth)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, st = ops.combine_shares(g, ids_t, pts_t, None, offs_t, n_sets)
            ts.append(time.perf_counter() - t0)
        assert int(st.ne(0).sum().item()) == 0
        api.profile_enable(True)
        ops.combine_shares(g, ids_t, pts_t, None, offs_t, n_sets)
        prof = {k: round(v[0], 3) for k, v in api.profile_read().items() if k.startswith('k_share')}
        api.profile_enable(False)
        batched = statistics.median(ts)
        # baseline: one MSM call per set on the same points
        scal_t = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev)
        scal_t.view(n, 32)[:, 31] &= 0x3f
        bs = min(n_sets, a.base_sets)
        fn = ops.lib.blsgpu_msm_g1 if g == 1 else ops.lib.blsgpu_msm_g2
        out = ops.empty(288)
        psz = pts_t.numel() // n
        import ctypes
        base = pts_t.data_ptr()
        sbase = scal_t.data_ptr()
        for s in range(min(bs, 4)):                                         # warm-up
            fn(ctypes.c_void_p(base + s * t * psz), ctypes.c_void_p(sbase + s * t * 32), t, 0, ctypes.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        bts = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            for s in range(bs):
                api._check(fn(ctypes.c_void_p(base + s * t * psz), ctypes.c_void_p(sbase + s * t * 32), t, 0, ctypes.c_void_p(out.data_ptr())))
            bts.append((time.perf_counter() - t0) * n_sets / bs)
        baseline = statistics.median(bts)
        row = {'shape': name, 'group': g, 'sets': n_sets, 'shares_per_set': t, 'batched_ms': round(batched * 1e3, 3),
               'batched_recoveries_per_s': round(n_sets / batched, 1), 'baseline_ms': round(baseline * 1e3, 3),
               'baseline_recoveries_per_s': round(n_sets / baseline, 1), 'baseline_sets_timed': bs, 'speedup': round(baseline / batched, 2),
               'kernel_ms': prof, 'reps': a.reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
