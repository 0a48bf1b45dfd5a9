#!/usr/bin/env python3
"""Registered key sets against keys by value: what the index-addressed entry points and the fixed-base tables cost and save.

usage: python tools/bench_keyset.py [--lines | --coop | --agg | --update] [--reps 5] [--table 16384] [--shapes 0,1,..] [--out profiles/keyset_bench.json]
Every input lives on the device (TensorOps).  Per shape, indices are drawn at random from a table of --table keys k * g
(blsgpu_sign_batch) and four things are timed, each the median of --reps calls:
  (a) the non-indexed entry point on the same keys laid out contiguously (three repeats of the whole measurement: their range is the
      run-to-run spread the other figures are read against);
  (b) the indexed entry point on a key set without tables;
  (c) the indexed entry point on a key set with tables (the multi shapes never multiply, so (c) only shows that tables cost nothing);
  (d) blsgpu_keyset_create from RAW_PROJ device memory, with and without tables.
On a build without key sets (the parent commit) only (a) runs: the tool skips what the library does not export.  The verdicts are
mostly INVALID_SIGNATURE, which costs the same as OK.  Prints one JSON line per shape and writes them all to --out.

--lines [--out profiles/keyset_lines_bench.json]: the per-key line tables (BLSGPU_KEYSET_LINES) instead -- one key per item,
Bls12381G1Impl, Basic: blsgpu_verify_batch / blsgpu_verify_indexed_batch at 8,192, 65,536 and 262,144 items and
blsgpu_verify_shared_batch / blsgpu_verify_shared_indexed_batch at 64 x 1,024 and 400 x 400, with (a) keys by value, (b) indexed over a
set without lines, (c) indexed over a set with lines; EVERY cell three medians of --reps calls (their range is the cell's spread),
the line kernel's time per call from the profile, and blsgpu_keyset_create with and without the flag.  A library that refuses the
flag (the parent commit) runs (a) and (b) only.

--coop [--out profiles/keyset_lines_coop_bench.json]: the same cells on the one-wave-per-item pairing path (BLSGPU_WIDE_MAX < items <=
BLSGPU_COOP_MAX), where a set with lines runs k_pairing_coop_keyed in the place of k_pairing_coop: blsgpu_verify_indexed_batch at 513,
1,024, 2,048 and 4,096 items, 4,097 (the first lane-split size) beside them, and blsgpu_verify_shared_indexed_batch at 8 x 256.  On
the parent commit (c) walks the keys as (b) does: its (a) and (b) are the yardstick.

--agg [--out profiles/keyset_agg_bench.json]: the batched aggregate verify (many keys with one message each per set), Basic with
distinct messages: (a) blsgpu_aggregate_verify_batch by value, (b) blsgpu_aggregate_verify_indexed_batch over a set without lines,
(c) the same over a set with lines, at 4,096 x 16, 1,024 x 64 and 256 x 600 for Bls12381G1Impl and 1,024 x 64 for Bls12381G2Impl
((a) and (b): its keys have no lines); every cell three medians of --reps calls, the kernel times of one call from the profile,
and for (c) the bytes per second k_linesp_keyed reached against its own traffic (per item and entry one 224-byte row read and
336 bytes of line value written, 68 entries, plus the item's G1 point).  A library without the indexed entry point (the parent
commit) runs (a) only.

--update [--out profiles/keyset_update_bench.json]: following a list that changes.  Per impl a set of --table keys with BOTH flags
(fixed-base tables, and line tables where the keys have them), keys as RAW_PROJ in device memory: blsgpu_keyset_update of 1, 16, 256
and 4,096 random distinct positions and blsgpu_keyset_append of 256 keys (onto a fresh set of --table keys each time, made outside
the timed region), each against blsgpu_keyset_create of the final list on the same build -- the only way to the same set without
these calls.  EVERY cell three medians of --reps calls, and the kernel times of one call from the profile."""
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
SIG_POOL = 4096
SHAPES = [('secure', 'Bls12381G2Impl Modern', 2, 1024, 400), ('secure', 'Bls12381G2Impl Modern', 2, 4096, 50), ('secure', 'Bls12381G1Impl', 1, 256, 400),
          ('multi', 'Bls12381G2Impl', 2, 1024, 512), ('multi', 'Bls12381G1Impl', 1, 1024, 512)]


def median_ms(run, reps, sync):
    run()                                                                    # warm-up (workspace growth)
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


LINES_SHAPES = [('verify', 8192, 1), ('verify', 65536, 1), ('verify', 262144, 1), ('shared', 64, 1024), ('shared', 400, 400)]
COOP_SHAPES = [('verify', 513, 1), ('verify', 1024, 1), ('verify', 2048, 1), ('verify', 4096, 1), ('verify', 4097, 1), ('shared', 8, 256)]


def lines_bench(a, api, ops, torch, dev, sync, all_shapes=LINES_SHAPES):
    rng = random.Random(2027)
    ks = [rng.randrange(1, R) for _ in range(a.table)]
    pks = api.sign_batch(1, api.BASIC, ks, [b''] * a.table)[0]
    sigs = api.sign_batch(1, api.BASIC, ks[:SIG_POOL], [b'bench'] * SIG_POOL)[1]
    pk_pool = torch.tensor(list(b''.join(pks)), dtype=torch.uint8, device=dev).view(a.table, -1)
    sig_pool = torch.tensor(list(b''.join(sigs)), dtype=torch.uint8, device=dev).view(SIG_POOL, -1)
    sync()
    made, create = {}, {}
    for lines in (False, True):
        ts = []
        try:
            for _ in range(3):
                if lines in made:
                    made.pop(lines).close()
                t0 = time.perf_counter()
                made[lines] = api.KeySet.create_device(1, pk_pool.data_ptr(), a.table, api.FMT_RAW_PROJ, lines=lines)
                ts.append((time.perf_counter() - t0) * 1e3)
        except api.BlsGpuRuntimeError as e:                                  # a library without the flag
            create['with lines'] = 'refused: %s' % e
            continue
        create['with lines' if lines else 'without lines'] = dict(ms=round(statistics.median(ts), 3), first_ms=round(ts[0], 3), **made[lines].info())
    rows = [{'table_entries': a.table, 'create': create}]
    print(json.dumps(rows[0]), flush=True)
    shapes = [all_shapes[int(i)] for i in a.shapes.split(',')] if a.shapes else all_shapes
    for kind, n_groups, per in shapes:
        n = n_groups * per
        gen = torch.Generator(device=dev).manual_seed(n + n_groups)
        sel = torch.randint(0, a.table, (n,), device=dev, generator=gen)
        pks_t = pk_pool[sel].reshape(-1).contiguous()
        idx_t = sel.to(torch.int32).contiguous()
        sigs_t = sig_pool[torch.randint(0, SIG_POOL, (n,), device=dev, generator=gen)].reshape(-1).contiguous()
        moffs, mblob = api._offsets([b'attestation %06d' % s for s in range(n_groups)])
        msgs_t = torch.tensor(list(mblob), dtype=torch.uint8, device=dev)
        moffs_t = torch.tensor(list(moffs), dtype=torch.int64, device=dev)
        if kind == 'verify':
            by_value = lambda: ops.verify_batch(1, api.BASIC, pks_t, sigs_t, msgs_t, moffs_t, n)
            indexed = lambda kset: (lambda: ops.verify_indexed_batch(kset, api.BASIC, idx_t, sigs_t, msgs_t, moffs_t, n))
        else:
            ioffs_t = torch.arange(0, n + 1, per, dtype=torch.int64, device=dev)
            by_value = lambda: ops.verify_shared_batch(1, api.BASIC, pks_t, sigs_t, ioffs_t, n_groups, msgs_t, moffs_t, n)
            indexed = lambda kset: (lambda: ops.verify_shared_indexed_batch(kset, api.BASIC, idx_t, sigs_t, ioffs_t, n_groups, msgs_t, moffs_t, n))
        row = {'kind': kind, 'shape': 'Bls12381G1Impl Basic', 'groups': n_groups, 'items_per_group': per, 'items': n, 'reps': a.reps}
        want = by_value().cpu().tolist()
        cells = [('a_by_value', by_value)] + [(tag, indexed(made[lines])) for tag, lines in (('b_indexed', False), ('c_indexed_lines', True)) if lines in made]
        for tag, run in cells:
            m3 = [median_ms(run, a.reps, sync) for _ in range(3)]
            row[tag + '_ms'] = [round(x, 3) for x in m3]
            row[tag + '_spread_ms'] = round(max(m3) - min(m3), 3)
            row[tag + '_statuses_match'] = run().cpu().tolist() == want
            api.profile_enable(True)
            run()
            row[tag + '_kernel_ms'] = {k: round(v[0], 3) for k, v in api.profile_read().items() if v[0] >= 0.01}
            api.profile_enable(False)
        print(json.dumps(row), flush=True)
        rows.append(row)
    for kset in made.values():
        kset.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


AGG_SHAPES = [(1, 4096, 16), (1, 1024, 64), (1, 256, 600), (2, 1024, 64)]
LINESP_KEYED_ITEM_BYTES = 68 * (4 + 6) * 14 * 4 + 2 * 14 * 4      # rows read + line values written + the G1 point


def agg_bench(a, api, ops, torch, dev, sync):
    have = hasattr(ops, 'aggregate_verify_indexed_batch')
    rng = random.Random(2028)
    shapes = [AGG_SHAPES[int(i)] for i in a.shapes.split(',')] if a.shapes else AGG_SHAPES
    pools, made = {}, {}
    for sg in sorted({s[0] for s in shapes}):
        ks = [rng.randrange(1, R) for _ in range(a.table)]
        pks = api.sign_batch(sg, api.BASIC, ks, [b''] * a.table)[0]
        sigs = api.sign_batch(sg, api.BASIC, ks[:SIG_POOL], [b'bench'] * SIG_POOL)[1]
        pools[sg] = (torch.tensor(list(b''.join(pks)), dtype=torch.uint8, device=dev).view(a.table, -1),
                     torch.tensor(list(b''.join(sigs)), dtype=torch.uint8, device=dev).view(SIG_POOL, -1))
        sync()
        if have:
            made[sg] = {lines: api.KeySet.create_device(sg, pools[sg][0].data_ptr(), a.table, api.FMT_RAW_PROJ, lines=lines)
                        for lines in ((False, True) if sg == 1 else (False,))}
    rows = [{'table_entries': a.table, 'sets': {'sig_group %d %s lines' % (sg, 'with' if lines else 'without'): k.info()
                                                for sg, m in made.items() for lines, k in m.items()}}]
    print(json.dumps(rows[0]), flush=True)
    for sg, n_sets, t in shapes:
        n = n_sets * t
        gen = torch.Generator(device=dev).manual_seed(n + sg)
        sel = torch.randint(0, a.table, (n,), device=dev, generator=gen)
        pks_t = pools[sg][0][sel].reshape(-1).contiguous()
        idx_t = sel.to(torch.int32).contiguous()
        sigs_t = pools[sg][1][torch.randint(0, SIG_POOL, (n_sets,), device=dev, generator=gen)].reshape(-1).contiguous()
        moffs, mblob = api._offsets([b'block %05d vote %05d' % (i // t, i % t) for i in range(n)])
        msgs_t = torch.tensor(list(mblob), dtype=torch.uint8, device=dev)
        moffs_t = torch.tensor(list(moffs), dtype=torch.int64, device=dev)
        soffs_t = torch.arange(0, n + 1, t, dtype=torch.int64, device=dev)
        tail = (msgs_t, moffs_t, soffs_t, n_sets, sigs_t)
        by_value = lambda: ops.aggregate_verify_batch(sg, api.BASIC, pks_t, *tail)[0]
        indexed = lambda kset: (lambda: ops.aggregate_verify_indexed_batch(kset, api.BASIC, idx_t, *tail)[0])
        row = {'kind': 'aggregate', 'shape': 'Bls12381G%dImpl Basic' % sg, 'sig_group': sg, 'sets': n_sets, 'pairs_per_set': t, 'pairs': n, 'reps': a.reps}
        want = by_value().cpu().tolist()
        cells = [('a_by_value', by_value)]
        if have:
            cells += [(tag, indexed(made[sg][lines])) for tag, lines in (('b_indexed', False), ('c_indexed_lines', True)) if lines in made[sg]]
        for tag, run in cells:
            m3 = [median_ms(run, a.reps, sync) for _ in range(3)]
            row[tag + '_ms'] = [round(x, 3) for x in m3]
            row[tag + '_spread_ms'] = round(max(m3) - min(m3), 3)
            row[tag + '_statuses_match'] = run().cpu().tolist() == want
            api.profile_enable(True)
            before = {k: v[0] for k, v in api.profile_read().items()}
            run()
            km = {k: v[0] - before.get(k, 0.0) for k, v in api.profile_read().items()}
            api.profile_enable(False)
            row[tag + '_kernel_ms'] = {k: round(v, 3) for k, v in km.items() if v >= 0.01}
            if km.get('k_linesp_keyed', 0) > 0:
                row[tag + '_linesp_keyed_GBps'] = round((n + n_sets) * LINESP_KEYED_ITEM_BYTES / (km['k_linesp_keyed'] * 1e-3) / 1e9, 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    for m in made.values():
        for kset in m.values():
            kset.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


UPDATE_COUNTS = [1, 16, 256, 4096]
APPEND_COUNT = 256


def update_bench(a, api, ops, torch, dev, sync):
    rng = random.Random(2029)
    rows = [{'table_entries': a.table, 'flags': 'tables + lines', 'reps': a.reps}]

    def kernel_ms(run):
        api.profile_enable(True)
        before = {k: v[0] for k, v in api.profile_read().items()}
        run()
        km = {k: v[0] - before.get(k, 0.0) for k, v in api.profile_read().items()}
        api.profile_enable(False)
        return {k: round(v, 3) for k, v in km.items() if v >= 0.001}

    def three(run):
        m3 = [median_ms(run, a.reps, sync) for _ in range(3)]
        return {'ms': [round(x, 3) for x in m3], 'spread_ms': round(max(m3) - min(m3), 3)}

    for sg in (1, 2):
        total = a.table + APPEND_COUNT
        ks = [rng.randrange(1, R) for _ in range(total + max(UPDATE_COUNTS))]
        pks = api.sign_batch(sg, api.BASIC, ks, [b''] * len(ks))[0]
        pool = torch.tensor(list(b''.join(pks)), dtype=torch.uint8, device=dev).view(len(ks), -1)
        fresh = pool[total:].contiguous()                                    # the keys an update writes
        grown = pool[:total].contiguous()
        sync()
        make = lambda n: api.KeySet.create_device(sg, grown.data_ptr(), n, api.FMT_RAW_PROJ, tables=True, lines=True)
        kset = make(a.table)
        row = {'impl': 'Bls12381G%dImpl' % sg, 'sig_group': sg, 'set': kset.info()}

        def recreate(n):
            make(n).close()
        row['create_%d' % a.table] = dict(three(lambda: recreate(a.table)), kernel_ms=kernel_ms(lambda: recreate(a.table)))
        row['create_%d' % total] = dict(three(lambda: recreate(total)), kernel_ms=kernel_ms(lambda: recreate(total)))
        for count in UPDATE_COUNTS:
            pos = torch.tensor(rng.sample(range(a.table), count), dtype=torch.int32, device=dev)
            keys = fresh[:count].reshape(-1).contiguous()
            sync()
            run = lambda: ops.keyset_update(kset, pos, keys, count, api.FMT_RAW_PROJ)
            cell = dict(three(run), kernel_ms=kernel_ms(run))
            cell['against_create'] = round(statistics.median(cell['ms']) / statistics.median(row['create_%d' % a.table]['ms']), 3)
            row['update_%d' % count] = cell
        kset.close()
        # append: every timed call grows a set of --table keys, made (and closed) outside the timed region
        tail = grown[a.table:].reshape(-1).contiguous()
        ts, km = [], None
        for r in range(3 * a.reps + 2):
            kset = make(a.table)
            sync()
            if r == 1:
                km = kernel_ms(lambda: ops.keyset_append(kset, tail, APPEND_COUNT, api.FMT_RAW_PROJ))
            else:
                t0 = time.perf_counter()
                ops.keyset_append(kset, tail, APPEND_COUNT, api.FMT_RAW_PROJ)
                ts.append((time.perf_counter() - t0) * 1e3)
            after = kset.info()
            kset.close()
        ts = ts[1:]                                                          # the first call is the warm-up
        m3 = [statistics.median(ts[i * a.reps:(i + 1) * a.reps]) for i in range(3)]
        row['append_%d' % APPEND_COUNT] = {'ms': [round(x, 3) for x in m3], 'spread_ms': round(max(m3) - min(m3), 3), 'kernel_ms': km, 'set_after': after,
                                           'against_create': round(statistics.median(m3) / statistics.median(row['create_%d' % total]['ms']), 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lines', action='store_true')
    ap.add_argument('--coop', action='store_true')
    ap.add_argument('--update', action='store_true')
    ap.add_argument('--agg', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--table', type=int, default=16384)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'keyset_bench.json'))
    ap.add_argument('--shapes', default='')
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sync = torch.cuda.synchronize
    if a.update:
        if a.out.endswith('keyset_bench.json'):
            a.out = os.path.join(ROOT, 'profiles', 'keyset_update_bench.json')
        return update_bench(a, api, ops, torch, dev, sync)
    if a.agg:
        if a.out.endswith('keyset_bench.json'):
            a.out = os.path.join(ROOT, 'profiles', 'keyset_agg_bench.json')
        return agg_bench(a, api, ops, torch, dev, sync)
    if a.coop:
        if a.out.endswith('keyset_bench.json'):
            a.out = os.path.join(ROOT, 'profiles', 'keyset_lines_coop_bench.json')
        return lines_bench(a, api, ops, torch, dev, sync, COOP_SHAPES)
    if a.lines:
        if a.out.endswith('keyset_bench.json'):
            a.out = os.path.join(ROOT, 'profiles', 'keyset_lines_bench.json')
        return lines_bench(a, api, ops, torch, dev, sync)
    have = hasattr(api, 'KeySet')                                            # the parent commit has no key sets: (a) only
    rng = random.Random(2026)
    pools, sets, create = {}, {}, {}
    shapes = [SHAPES[int(i)] for i in a.shapes.split(',')] if a.shapes else SHAPES
    for sg in sorted({s[2] for s in shapes}):
        ks = [rng.randrange(1, R) for _ in range(a.table)]
        pks = api.sign_batch(sg, api.BASIC, ks, [b''] * a.table)[0]
        sigs = api.sign_batch(sg, api.BASIC, ks[:SIG_POOL], [b'bench'] * SIG_POOL)[1]
        pools[sg] = (torch.tensor(list(b''.join(pks)), dtype=torch.uint8, device=dev).view(a.table, -1),
                     torch.tensor(list(b''.join(sigs)), dtype=torch.uint8, device=dev).view(SIG_POOL, -1))
        if have:
            sync()
            made = {}
            for tables in (False, True):
                ts = []
                for _ in range(3):
                    if tables in made:
                        made[tables].close()
                    t0 = time.perf_counter()
                    made[tables] = api.KeySet.create_device(sg, pools[sg][0].data_ptr(), a.table, api.FMT_RAW_PROJ, tables=tables)
                    ts.append((time.perf_counter() - t0) * 1e3)
                create['sig_group %d %s tables' % (sg, 'with' if tables else 'without')] = dict(
                    ms=round(statistics.median(ts), 3), first_ms=round(ts[0], 3), **made[tables].info())
            sets[sg] = made
    rows = [{'table_entries': a.table, 'create': create}]
    print(json.dumps(rows[0]), flush=True)
    for kind, name, sg, n_sets, t in shapes:
        n = n_sets * t
        gen = torch.Generator(device=dev).manual_seed(n + sg)
        sel = torch.randint(0, a.table, (n,), device=dev, generator=gen)
        pks_t = pools[sg][0][sel].reshape(-1).contiguous()
        idx_t = sel.to(torch.int32).contiguous()
        sigs_t = pools[sg][1][torch.randint(0, SIG_POOL, (n_sets,), device=dev, generator=gen)].reshape(-1).contiguous()
        moffs, mblob = api._offsets([b'quorum commitment %06d' % s for s in range(n_sets)])
        msgs_t = torch.tensor(list(mblob), dtype=torch.uint8, device=dev)
        moffs_t = torch.tensor(list(moffs), dtype=torch.int64, device=dev)
        koffs_t = torch.arange(0, n + 1, t, dtype=torch.int64, device=dev)
        tail = (koffs_t, sigs_t, msgs_t, moffs_t, n_sets)
        if kind == 'secure':
            by_value = lambda: ops.verify_secure_batch(sg, api.BASIC, pks_t, *tail)
            indexed = lambda ks: (lambda: ops.verify_secure_indexed_batch(ks, api.BASIC, idx_t, *tail))
        else:
            by_value = lambda: ops.multi_verify_batch(sg, api.BASIC, pks_t, *tail)
            indexed = lambda ks: (lambda: ops.multi_verify_indexed_batch(ks, api.BASIC, idx_t, *tail))
        a3 = [median_ms(by_value, a.reps, sync) for _ in range(3)]
        row = {'kind': kind, 'shape': name, 'sig_group': sg, 'sets': n_sets, 'keys_per_set': t, 'reps': a.reps,
               'a_by_value_ms': [round(x, 3) for x in a3], 'a_spread_ms': round(max(a3) - min(a3), 3)}
        if have:
            want = by_value().cpu().tolist()
            for tag, tables in (('b_indexed_ms', False), ('c_indexed_tables_ms', True)):
                run = indexed(sets[sg][tables])
                row[tag] = round(median_ms(run, a.reps, sync), 3)
                row[tag.replace('_ms', '_statuses_match')] = run().cpu().tolist() == want
            api.profile_enable(True)
            indexed(sets[sg][True])()
            row['c_kernel_ms'] = {k: round(v[0], 3) for k, v in api.profile_read().items() if v[0] >= 0.01}
            api.profile_enable(False)
        print(json.dumps(row), flush=True)
        rows.append(row)
    for made in sets.values():
        for ks in made.values():
            ks.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
