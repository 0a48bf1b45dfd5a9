#!/usr/bin/env python3
"""Shared-message verify against blsgpu_verify_batch on the same items with the messages repeated: what hashing once per group
and the per-group line tables save.

usage: python tools/bench_verify_shared.py [--reps 5] [--shapes 0,1,..|96x1024,..] [--sig-groups 2,1] [--out profiles/verify_shared_bench.json]
Every input lives on the device (TensorOps); every figure is the median of --reps calls after one warm-up call.  Per shape
(groups x items per group) and orientation:
  (a) blsgpu_verify_batch with one message per item -- measured three times over: the range of the three medians is the
      run-to-run spread the other figures are read against;
  (b) blsgpu_verify_shared_batch with the per-group line tables off (BLSGPU_SHARED_LINES_MIN=0): hash sharing alone;
  (c) the same with the tables on at every group size (BLSGPU_SHARED_LINES_MIN=1), and its per-kernel times.
The knob is read when the library binds its devices, so (b) and (c) run in a child process each (--child).  On a build without
the call (the parent commit) only (a) runs: the tool skips what the library lacks.  The statuses of (b) and (c) must equal (a)'s.
Prints one JSON line per row and writes them all to --out."""
import argparse
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
SHAPES = [(64, 1024), (1024, 64), (16384, 4), (65536, 1), (400, 400)]
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


def measure(a, mode):
    """mode 'a': the baseline three times; 'b' / 'c': the shared call under this process's knob"""
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sync = torch.cuda.synchronize
    have = hasattr(ops, 'verify_shared_batch')
    rows = []
    shapes = [tuple(int(x) for x in i.split('x')) if 'x' in i else SHAPES[int(i)] for i in a.shapes.split(',')] if a.shapes else SHAPES
    for sg in [int(x) for x in a.sig_groups.split(',')]:
        rng = random.Random(2026 + sg)
        ks = [rng.randrange(1, R) for _ in range(KEY_POOL)]
        for n_groups, per in shapes:
            n = n_groups * per
            msgs = [b'sign hash %08d' % g + bytes(18) for g in range(n_groups)]                 # 32-byte messages
            # item i of group g: key i mod KEY_POOL; the signatures come from sign_batch under the item's message, so all verify
            item_msgs = [msgs[i // per] for i in range(n)]
            pks, sigs = api.sign_batch(sg, api.BASIC, [ks[i % KEY_POOL] for i in range(n)], item_msgs)
            sigs[n // 2] = sigs[n // 2 - 1] if n > 1 else sigs[0]                                # one invalid item when there is room
            tens = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
            pk_t, sig_t = tens(b''.join(pks)), tens(b''.join(sigs))
            del pks, sigs
            moffs, mblob = api._offsets(msgs)
            xoffs, xblob = api._offsets(item_msgs)
            msg_t, moffs_t = tens(mblob), torch.tensor(list(moffs), dtype=torch.int64, device=dev)
            xmsg_t, xoffs_t = tens(xblob), torch.tensor(list(xoffs), dtype=torch.int64, device=dev)
            ioffs_t = torch.arange(0, n + 1, per, dtype=torch.int64, device=dev)
            del item_msgs
            by_item = lambda: ops.verify_batch(sg, api.BASIC, pk_t, sig_t, xmsg_t, xoffs_t, n)  # noqa: E731
            row = {'sig_group': sg, 'groups': n_groups, 'items_per_group': per, 'reps': a.reps}
            want = by_item().cpu()
            row['invalid_items'] = int((want != 0).sum())
            if mode == 'a':
                a3 = [median_ms(by_item, a.reps, sync) for _ in range(3)]
                row.update(a_verify_batch_ms=[round(x, 3) for x in a3], a_spread_ms=round(max(a3) - min(a3), 3))
            elif have:
                shared = lambda: ops.verify_shared_batch(sg, api.BASIC, pk_t, sig_t, ioffs_t, n_groups, msg_t, moffs_t, n)  # noqa: E731
                tag = {'b': 'b_shared_no_tables', 'c': 'c_shared_tables'}[mode]
                row[tag + '_ms'] = round(median_ms(shared, a.reps, sync), 3)
                row[tag + '_statuses_match'] = bool((shared().cpu() == want).all())
                api.profile_enable(True)
                shared()
                row[tag + '_kernel_ms'] = {k: round(v[0], 3) for k, v in api.profile_read().items() if v[0] >= 0.01}
                api.profile_enable(False)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows, have


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='', help='indices into the fixed list, or GROUPSxITEMS pairs, comma-separated')
    ap.add_argument('--sig-groups', default='2,1')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'verify_shared_bench.json'))
    ap.add_argument('--child', default='')
    a = ap.parse_args()
    if a.child:
        rows, _ = measure(a, a.child)
        print('ROWS ' + json.dumps(rows), flush=True)
        return
    rows, have = measure(a, 'a')
    if have:
        for mode, knob in (('b', '0'), ('c', '1')):
            env = dict(os.environ, BLSGPU_SHARED_LINES_MIN=knob)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--reps', str(a.reps), '--shapes', a.shapes, '--sig-groups', a.sig_groups], env=env,
                               capture_output=True, text=True)
            sys.stderr.write(p.stderr[-2000:])
            if p.returncode != 0:
                raise SystemExit('child %s failed with %d' % (mode, p.returncode))
            more = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('ROWS ')][-1][5:])
            for row, m in zip(rows, more):
                assert (row['sig_group'], row['groups'], row['items_per_group']) == (m['sig_group'], m['groups'], m['items_per_group'])
                row.update(m)
        for row in rows:
            best_a = min(row['a_verify_batch_ms'])
            row['tables_gain_over_no_tables_ms'] = round(row['b_shared_no_tables_ms'] - row['c_shared_tables_ms'], 3)
            row['shared_gain_over_verify_batch_ms'] = round(best_a - min(row['b_shared_no_tables_ms'], row['c_shared_tables_ms']), 3)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
