#!/usr/bin/env python3
"""Aggregate verify by message index against blsgpu_aggregate_verify_batch by value on the same sets: what summing the keys of equal
messages and hashing nothing saves.

usage: python tools/bench_agg_msgset.py [--reps 5] [--shapes 1024x64x64,..] [--sig-groups 2,1] [--parent-lib PATH]
                                        [--out profiles/agg_msgset_bench.json]
Scheme ProofOfPossession, 32-byte messages, every input on the device; every figure is the median of --reps timed calls after one
warm-up call.  A shape is SETS x PAIRS x DISTINCT: every set has PAIRS pairs under DISTINCT messages, drawn from one message set of
4,096 entries.  Per shape and orientation:
  (a)  blsgpu_aggregate_verify_batch by value on THIS build (message bytes per pair);
  (a') the same call on the library given by --parent-lib (the parent commit's build), measured by a child process that loads that
       library alone, twice: the two medians' difference is the run-to-run spread the other columns are read against;
  (b)  blsgpu_aggregate_verify_msgset_batch over a set without rows;
  (c)  the same over a set with rows (Bls12381G2Impl only: a Bls12381G1Impl set has none).
The statuses of every column must equal (a)'s.  Per-kernel times come from blsgpu_profile_*.  Prints one JSON line per row and writes
them all to --out."""
import argparse
import ctypes
import json
import os
import pickle
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SHAPES = [(1024, 64, 64), (1024, 64, 8), (1024, 64, 1), (4096, 16, 16), (4096, 16, 2), (256, 600, 8)]
KEY_POOL, MSG_POOL = 4096, 4096
POP = 2


def median_ms(run, reps, sync):
    run()                                                                    # warm-up (workspace growth)
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def child(path, lib_path, reps):
    """(a'): blsgpu_aggregate_verify_batch of the pickled sets on the library at lib_path, loaded by itself; one JSON line"""
    import torch
    d = pickle.load(open(path, 'rb'))
    lib = ctypes.CDLL(lib_path)
    vp = ctypes.c_void_p
    lib.blsgpu_init.argtypes = [ctypes.c_int]
    lib.blsgpu_aggregate_verify_batch.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_int, vp, vp]
    assert lib.blsgpu_init(-1) == 0
    dev = torch.device('cuda', 0)
    tens = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
    pk, sig, msg, moffs, soffs = tens(d['pks']), tens(d['sigs']), tens(d['msgs']), i64(d['moffs']), i64(d['soffs'])
    n = d['n_sets']
    st, aux = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(2 * n, dtype=torch.int64, device=dev)

    def run():
        rc = lib.blsgpu_aggregate_verify_batch(d['sg'], POP, pk.data_ptr(), msg.data_ptr(), moffs.data_ptr(), soffs.data_ptr(), n, sig.data_ptr(), 0, st.data_ptr(),
                                               aux.data_ptr())
        assert rc == 0, rc
    ms = median_ms(run, reps, torch.cuda.synchronize)
    print(json.dumps({'ms': ms, 'statuses': st.cpu().tolist()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='', help='SETSxPAIRSxDISTINCT triples, comma-separated')
    ap.add_argument('--sig-groups', default='2,1')
    ap.add_argument('--parent-lib', default='', help="the parent commit's libblsgpu.so, for column (a')")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'agg_msgset_bench.json'))
    ap.add_argument('--child', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.parent_lib, a.reps)
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sync = torch.cuda.synchronize
    shapes = [tuple(int(x) for x in i.split('x')) for i in a.shapes.split(',')] if a.shapes else SHAPES
    tens = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
    rows = []
    tmp = tempfile.mkdtemp(prefix='agg_msgset_bench_')
    for sg in [int(x) for x in a.sig_groups.split(',')]:
        rng = random.Random(2030 + sg)
        ks = [rng.randrange(1, R) for _ in range(KEY_POOL)]
        pool = api.sign_batch(sg, api.POP, ks, [b''] * KEY_POOL)[0]
        msgs = [b'slot message %08d' % g + bytes(11) for g in range(MSG_POOL)]                  # 32-byte messages
        plain = api.MessageSet.create(sg, api.POP, msgs)
        rowed = api.MessageSet.create(sg, api.POP, msgs, lines=True) if sg == 2 else None
        for n_sets, per, distinct in shapes:
            T = n_sets * per
            # pair j of set s: key (s per + j) mod KEY_POOL under entry (s distinct + j mod distinct) mod MSG_POOL; one set in 64 carries its
            # neighbour's signature
            kidx = [(s * per + j) % KEY_POOL for s in range(n_sets) for j in range(per)]
            midx = [(s * distinct + j % distinct) % MSG_POOL for s in range(n_sets) for j in range(per)]
            secrets, signed = [], []
            for s in range(n_sets):
                by = {}
                for j in range(per):
                    by[midx[s * per + j]] = (by.get(midx[s * per + j], 0) + ks[kidx[s * per + j]]) % R
                secrets += list(by.values())
                signed += [msgs[m] for m in by]
            parts = api.sign_batch(sg, api.POP, secrets, signed)[1]
            sigs = api.sum_batch(sg, [parts[s * distinct:(s + 1) * distinct] for s in range(n_sets)])
            for s in range(5, n_sets, 64):
                sigs[s] = sigs[s - 1]
            data = {'sg': sg, 'n_sets': n_sets, 'pks': b''.join(pool[k] for k in kidx), 'sigs': b''.join(sigs), 'msgs': b''.join(msgs[m] for m in midx),
                    'moffs': list(range(0, 32 * T + 1, 32)), 'soffs': list(range(0, T + 1, per))}
            del parts, sigs
            pk_t, sig_t, msg_t, moffs_t, soffs_t = tens(data['pks']), tens(data['sigs']), tens(data['msgs']), i64(data['moffs']), i64(data['soffs'])
            midx_t = torch.tensor(midx, dtype=torch.int32, device=dev)
            sync()
            by_value = lambda: ops.aggregate_verify_batch(sg, api.POP, pk_t, msg_t, moffs_t, soffs_t, n_sets, sig_t)[0]  # noqa: E731
            row = {'sig_group': sg, 'sets': n_sets, 'pairs_per_set': per, 'distinct_per_set': distinct, 'reps': a.reps}
            want = by_value().cpu()
            row['invalid_sets'] = int((want != 0).sum())
            cols = [('a_by_value', by_value), ('b_msgset_no_rows', lambda: ops.aggregate_verify_msgset_batch(plain, midx_t, pk_t, soffs_t, n_sets, sig_t)[0])]
            if rowed is not None:
                row['rows_built'] = rowed.info()['has_lines']
                cols.append(('c_msgset_rows', lambda: ops.aggregate_verify_msgset_batch(rowed, midx_t, pk_t, soffs_t, n_sets, sig_t)[0]))
            for tag, run in cols:
                row[tag + '_ms'] = median_ms(run, a.reps, sync)
                row[tag + '_statuses_match'] = bool((run().cpu() == want).all())
                api.profile_enable(True)
                before = {k: v[0] for k, v in api.profile_read().items()}
                run()
                row[tag + '_kernel_ms'] = {k: round(v[0] - before.get(k, 0), 3) for k, v in api.profile_read().items() if v[0] - before.get(k, 0) >= 0.005}
                api.profile_enable(False)
            if a.parent_lib:
                path = os.path.join(tmp, 'sets.pickle')
                with open(path, 'wb') as f:
                    pickle.dump(data, f)
                two = []
                for _ in range(2):
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path, '--parent-lib', a.parent_lib, '--reps', str(a.reps)],
                                       capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:
                        raise RuntimeError('the parent column failed: ' + r.stderr[-2000:])
                    res = json.loads(r.stdout.strip().splitlines()[-1])
                    two.append(res['ms'])
                    row['a_parent_statuses_match'] = res['statuses'] == want.tolist()
                row['a_parent_ms'] = two
                row['a_parent_spread_ms'] = round(abs(two[0] - two[1]), 3)
                base = statistics.mean(two)
                row['b_over_parent'] = round(row['b_msgset_no_rows_ms'] / base, 3)
                if rowed is not None:
                    row['c_over_parent'] = round(row['c_msgset_rows_ms'] / base, 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del data, pk_t, sig_t, msg_t
        for s in (plain, rowed):
            if s is not None:
                s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
