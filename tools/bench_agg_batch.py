#!/usr/bin/env python3
"""Batched aggregate verify throughput (blsgpu_aggregate_verify_batch) against what a caller has without it: one
blsgpu_aggregate_verify call per set.

usage: python tools/bench_agg_batch.py [--reps 5] [--base-sets 32] [--shapes 0,1] [--force-batched | --knob N] [--baseline-lib PATH]
                                       [--append] [--out profiles/agg_batch_bench.json]
Inputs live on the device (TensorOps) for both forms, so neither pays host staging.  Keys are drawn from a pool of 65,536
distinct k * g (blsgpu_sign_batch), signatures from a pool of 4,096, every message is distinct; the verdicts are
INVALID_SIGNATURE, which costs the same as OK (every set runs the whole hash, Miller loops, product and final exponentiation).
The batched time is the median of --reps calls.  The baseline times the first --base-sets sets one call each and scales per set;
the two are timed alternately, rep by rep.  --baseline-lib names a second libblsgpu.so (a build of the commit before this entry
point existed) whose blsgpu_aggregate_verify is then the baseline; without it the baseline is this build's single call.
The one-set shape compares the batched entry point with blsgpu_aggregate_verify on the same 262,144 pairs.  The shapes 5 to 10
(16 sets of 1,024 to 65,536 pairs) place BLSGPU_AGG_BATCH_MAX and the shapes 11 to 14 (1, 2, 4, 8 sets of 64 pairs) show the call's
own floor: run them with --force-batched, which sets the knob to 2^32
before the library starts, so that `batched_ms` is the segmented kernels' time, and with --knob 1, so that it is the
one-at-a-time path's inside the same entry point.
Prints one JSON line per shape and writes them all to --out (--append: after the rows already there)."""
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
SHAPES = [('Bls12381G1Impl Basic', 1, 4096, 16), ('Bls12381G1Impl Basic', 1, 1024, 64), ('Bls12381G1Impl Basic', 1, 256, 600),
          ('Bls12381G2Impl Basic', 2, 1024, 64), ('Bls12381G1Impl one large set', 1, 1, 262144),
          ('knob: 16 sets', 1, 16, 1024), ('knob: 16 sets', 1, 16, 4096), ('knob: 16 sets', 1, 16, 16384),
          ('knob: 16 sets', 1, 16, 24576), ('knob: 16 sets', 1, 16, 32768), ('knob: 16 sets', 1, 16, 65536),
          ('few sets', 1, 1, 64), ('few sets', 1, 2, 64), ('few sets', 1, 4, 64), ('few sets', 1, 8, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--base-sets', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'agg_batch_bench.json'))
    ap.add_argument('--shapes', default='0,1,2,3,4')
    ap.add_argument('--force-batched', action='store_true')
    ap.add_argument('--knob', type=int, default=None, help='BLSGPU_AGG_BATCH_MAX for this run')
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--append', action='store_true')
    a = ap.parse_args()
    if a.force_batched:
        a.knob = 2 ** 32
    if a.knob is not None:
        os.environ['BLSGPU_AGG_BATCH_MAX'] = str(a.knob)
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    base_lib = ops.lib
    if a.baseline_lib:
        base_lib = ctypes.CDLL(a.baseline_lib)
        assert base_lib.blsgpu_init(0) == 0
        vp = ctypes.c_void_p
        base_lib.blsgpu_aggregate_verify.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_int, vp, vp]
    rng = random.Random(2026)
    pools = {}
    shapes = [SHAPES[int(i)] for i in a.shapes.split(',')]
    for sg in sorted({s[1] for s in shapes}):
        ks = [rng.randrange(1, R) for _ in range(KEY_POOL)]
        pks = api.sign_batch(sg, api.BASIC, ks, [b''] * KEY_POOL)[0]
        sigs = api.sign_batch(sg, api.BASIC, ks[:SIG_POOL], [b'bench'] * SIG_POOL)[1]
        pools[sg] = (torch.tensor(list(b''.join(pks)), dtype=torch.uint8, device=dev).view(KEY_POOL, -1),
                     torch.tensor(list(b''.join(sigs)), dtype=torch.uint8, device=dev).view(SIG_POOL, -1))
    rows = []
    for name, sg, n_sets, t in shapes:
        n = n_sets * t
        gen = torch.Generator(device=dev).manual_seed(n)
        sel = torch.randint(0, KEY_POOL, (n,), device=dev, generator=gen)
        pks_t = pools[sg][0][sel].reshape(-1).contiguous()
        ssel = torch.randint(0, SIG_POOL, (n_sets,), device=dev, generator=gen)
        sigs_t = pools[sg][1][ssel].reshape(-1).contiguous()
        mlen = 24
        msgs_t = torch.tensor(list(b''.join(b'attestation %012d' % i for i in range(n))), dtype=torch.uint8, device=dev)
        moffs_t = torch.arange(0, mlen * n + 1, mlen, dtype=torch.int64, device=dev)
        soffs_t = torch.arange(0, n + 1, t, dtype=torch.int64, device=dev)
        run = lambda: ops.aggregate_verify_batch(sg, api.BASIC, pks_t, msgs_t, moffs_t, soffs_t, n_sets, sigs_t)
        bs = min(n_sets, a.base_sets)
        psz, ssz = pks_t.numel() // n, sigs_t.numel() // n_sets
        stb = ops.empty(4 * bs)

        def one(s):
            # baseline: one blsgpu_aggregate_verify call for set s on the same device-resident inputs
            rc = base_lib.blsgpu_aggregate_verify(sg, api.BASIC, ctypes.c_void_p(pks_t.data_ptr() + s * t * psz), ctypes.c_void_p(msgs_t.data_ptr()),
                                                  ctypes.c_void_p(moffs_t.data_ptr() + 8 * s * t), t, ctypes.c_void_p(sigs_t.data_ptr() + s * ssz),
                                                  api.FMT_RAW_PROJ, ctypes.c_void_p(stb.data_ptr() + 4 * s), None)
            assert rc == 0, rc

        st, _ = run()                                                        # warm-up (workspace growth)
        for s in range(min(bs, 2)):
            one(s)
        torch.cuda.synchronize()
        ts, bts = [], []
        for _ in range(a.reps):                                              # both entry points return after a device synchronise
            t0 = time.perf_counter()
            st, _ = run()
            ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for s in range(bs):
                one(s)
            bts.append((time.perf_counter() - t0) * n_sets / bs)
        batched, baseline = statistics.median(ts), statistics.median(bts)
        api.profile_enable(True)
        run()
        prof = {k: [round(v[0], 3), v[1]] for k, v in api.profile_read().items()}
        api.profile_enable(False)
        same = stb.view(torch.int32)[:bs].cpu().tolist() == st[:bs].cpu().tolist()
        row = {'shape': name, 'sig_group': sg, 'sets': n_sets, 'pairs_per_set': t, 'knob': os.environ.get('BLSGPU_AGG_BATCH_MAX', 'default'),
               'batched_ms': round(batched * 1e3, 3), 'batched_min_ms': round(min(ts) * 1e3, 3), 'batched_sets_per_s': round(n_sets / batched, 1),
               'baseline_ms': round(baseline * 1e3, 3), 'baseline_min_ms': round(min(bts) * 1e3, 3),
               'baseline': 'previous build' if a.baseline_lib else 'this build', 'baseline_sets_per_s': round(n_sets / baseline, 1), 'baseline_sets_timed': bs,
               'speedup': round(baseline / batched, 2), 'statuses_match_single_call': same,
               'status_counts': {str(k): v for k, v in zip(*[x.tolist() for x in st.cpu().unique(return_counts=True)])},
               'kernel_ms_launches': prof, 'reps': a.reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            rows = json.load(f) + rows
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
