#!/usr/bin/env python3
"""Registered message sets against blsgpu_verify_shared_batch on the same items: what hashing a message at registration instead of in
every call saves, and what the registered rows save on top.

usage: python tools/bench_msgset.py [--reps 5] [--shapes 1x1,8x256,..] [--sig-groups 2,1] [--out profiles/msgset_bench.json]
Every input lives on the device (TensorOps), scheme Basic, 32-byte messages; every figure is the median of --reps calls after one
warm-up call, and every column is measured three times over: the range of the three medians is the run-to-run spread the columns
are read against.  Per shape (groups x items per group) and orientation:
  (a) blsgpu_verify_shared_batch (on a build without message sets -- the parent commit -- this column alone: it is (a'));
  (b) blsgpu_verify_msgset_batch over a set without rows;
  (c) the same over a set with rows (Bls12381G2Impl only: a Bls12381G1Impl set has none);
  Bls12381G1Impl also over a key set with line tables: (a_keyed) blsgpu_verify_shared_indexed_batch, (b_keyed)
  blsgpu_verify_msgset_indexed_batch.
The statuses of every column must equal (a)'s.  Prints one JSON line per row and writes them all to --out."""
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
SHAPES = [(1, 1), (1, 64), (1, 400), (8, 256), (4, 1024), (64, 1024)]
KEY_POOL = 4096


def median_ms(run, reps, sync):
    run()                                                                    # warm-up (workspace growth)
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def three(run, reps, sync):
    return [round(median_ms(run, reps, sync), 3) for _ in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='', help='GROUPSxITEMS pairs, comma-separated')
    ap.add_argument('--sig-groups', default='2,1')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msgset_bench.json'))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sync = torch.cuda.synchronize
    have = hasattr(api, 'MessageSet')
    shapes = [tuple(int(x) for x in i.split('x')) for i in a.shapes.split(',')] if a.shapes else SHAPES
    tens = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    rows = []
    for sg in [int(x) for x in a.sig_groups.split(',')]:
        rng = random.Random(2026 + sg)
        ks = [rng.randrange(1, R) for _ in range(KEY_POOL)]
        pool = api.sign_batch(sg, api.BASIC, ks, [b''] * KEY_POOL)[0]
        keyset = api.KeySet.create(sg, pool, api.FMT_RAW_PROJ, lines=True) if sg == 1 else None
        for n_groups, per in shapes:
            n = n_groups * per
            msgs = [b'sign hash %08d' % g + bytes(18) for g in range(n_groups)]                 # 32-byte messages
            # item i: key i mod KEY_POOL, signed under its group's message, so all verify -- but one, where there is room
            pks, sigs = api.sign_batch(sg, api.BASIC, [ks[i % KEY_POOL] for i in range(n)], [msgs[i // per] for i in range(n)])
            if n > 1:
                sigs[n // 2] = sigs[n // 2 - 1]
            pk_t, sig_t = tens(b''.join(pks)), tens(b''.join(sigs))
            del pks, sigs
            moffs, mblob = api._offsets(msgs)
            msg_t, moffs_t = tens(mblob), torch.tensor(list(moffs), dtype=torch.int64, device=dev)
            ioffs_t = torch.arange(0, n + 1, per, dtype=torch.int64, device=dev)
            midx_t = torch.arange(0, n_groups, dtype=torch.int32, device=dev)
            idx_t = (torch.arange(0, n, dtype=torch.int64, device=dev) % KEY_POOL).to(torch.int32)
            sync()
            shared = lambda: ops.verify_shared_batch(sg, api.BASIC, pk_t, sig_t, ioffs_t, n_groups, msg_t, moffs_t, n)  # noqa: E731
            row = {'sig_group': sg, 'groups': n_groups, 'items_per_group': per, 'reps': a.reps}
            want = shared().cpu()
            row['invalid_items'] = int((want != 0).sum())
            cols = [('a_verify_shared', shared)]
            sets = []
            if have:
                plain = api.MessageSet.create(sg, api.BASIC, msgs)
                sets.append(plain)
                cols.append(('b_msgset_no_rows', lambda: ops.verify_msgset_batch(plain, midx_t, pk_t, sig_t, ioffs_t, n_groups, n)))
                if sg == 2:
                    rowed = api.MessageSet.create(sg, api.BASIC, msgs, lines=True)
                    sets.append(rowed)
                    row['rows_built'] = rowed.info()['has_lines']
                    cols.append(('c_msgset_rows', lambda: ops.verify_msgset_batch(rowed, midx_t, pk_t, sig_t, ioffs_t, n_groups, n)))
            if keyset is not None:
                cols.append(('a_keyed_verify_shared_indexed', lambda: ops.verify_shared_indexed_batch(keyset, api.BASIC, idx_t, sig_t, ioffs_t, n_groups, msg_t, moffs_t, n)))
                if have:
                    cols.append(('b_keyed_msgset_indexed', lambda: ops.verify_msgset_indexed_batch(plain, midx_t, keyset, idx_t, sig_t, ioffs_t, n_groups, n)))
            for tag, run in cols:
                ms3 = three(run, a.reps, sync)
                row[tag + '_ms'] = ms3
                row[tag + '_spread_ms'] = round(max(ms3) - min(ms3), 3)
                row[tag + '_statuses_match'] = bool((run().cpu() == want).all())
                api.profile_enable(True)
                run()
                row[tag + '_kernel_ms'] = {k: round(v[0], 3) for k, v in api.profile_read().items() if v[0] >= 0.005}
                api.profile_enable(False)
            if have:
                row['b_gain_over_a_ms'] = round(statistics.median(row['a_verify_shared_ms']) - statistics.median(row['b_msgset_no_rows_ms']), 3)
                if sg == 2:
                    # the bar a row form is held to: the slowest (c) median below the fastest (b) median
                    row['c_slowest_below_b_fastest'] = max(row['c_msgset_rows_ms']) < min(row['b_msgset_no_rows_ms'])
            for s in sets:
                s.close()
            print(json.dumps(row), flush=True)
            rows.append(row)
        if keyset is not None:
            keyset.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
