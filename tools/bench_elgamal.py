#!/usr/bin/env python3
"""ElGamal proof verification throughput (blsgpu_elgamal_proof_verify_batch) against the same point arithmetic composed from the
older entry points: blsgpu_keyset_mul without tables over the 5 n (point, scalar) terms plus blsgpu_sum_batch over the 2 n sums.

usage: python tools/bench_elgamal.py [--reps 5] [--sizes 1,1024,65536] [--out profiles/elgamal_bench.json]
Inputs live on the device (TensorOps) for both forms.  The points are a pool of 4,096 distinct k * g (blsgpu_sign_batch) reused
across proofs; the scalars are random 254-bit values, so every proof is well formed and fails only at the challenge comparison
(status 18): all of the arithmetic and the whole transcript run for every item.
The transcript is excluded on both sides: the joint ladder is charged k_elgamal_prep + k_elgamal_ladder from the library's profile
counters, the composition everything its two calls launch (the key set's creation is not timed).  Wall times of the whole calls
are reported next to them.  Prints one JSON line per shape and writes them all to --out."""
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
POOL = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='1,1024,65536')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'elgamal_bench.json'))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    rng = random.Random(2025)
    rows = []

    def profiled(fn):
        api.profile_enable(True)
        fn()
        prof = {k: round(v[0], 3) for k, v in api.profile_read().items() if v[1]}
        api.profile_enable(False)
        return prof

    def timed(fn):
        fn()                                              # warm-up (workspace growth)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    for sg in (1, 2):
        kgroup = 3 - sg
        osz = 144 * kgroup
        ks = [rng.randrange(1, R) for _ in range(POOL)]
        pool = torch.tensor(list(b''.join(api.sign_batch(sg, api.BASIC, ks, [b''] * POOL)[0])), dtype=torch.uint8, device=dev).view(POOL, osz)
        gen = torch.tensor(list(api.sign_batch(sg, api.BASIC, [1], [b''])[0][0]), dtype=torch.uint8, device=dev)
        h = ops.elgamal_message_generator(sg)
        for n in [int(x) for x in a.sizes.split(',')]:
            gsel = torch.Generator(device=dev).manual_seed(7 * n + sg)
            pick = lambda k: pool[torch.randint(0, POOL, (k,), device=dev, generator=gsel)].reshape(-1).contiguous()
            scal = lambda k: torch.randint(0, 256, (k, 32), dtype=torch.uint8, device=dev, generator=gsel)
            c1s, c2s, pks = pick(n), pick(n), pick(n)
            mps, bps, chs = scal(n), scal(n), scal(n)
            for t in (mps, bps, chs):
                t[:, 31] &= 0x3f
                t[:, 0] |= 1
            for shared in (False, True):
                pk_t, n_pks = (pks[:osz], 1) if shared else (pks, n)
                run = lambda: ops.elgamal_proof_verify_batch(sg, pk_t, n_pks, None, c1s, c2s, mps, bps, chs, n)
                wall = timed(run)
                assert run().eq(api.CHALLENGE_MISMATCH).all().item()
                prof = profiled(run)
                joint = prof.get('k_elgamal_prep', 0) + prof.get('k_elgamal_ladder', 0)
                # the composition: r1 = (-c) c1 + bp G (2 n terms), r2 = (-c) c2 + mp H + bp pk (3 n terms).  The scalar -c costs the
                # same ladder as c, so the challenges stand in for their negations.
                pk_all = pks if not shared else pks[:osz].repeat(n)
                bases = torch.cat([c1s.view(n, osz), gen.repeat(n, 1), c2s.view(n, osz), h.repeat(n, 1), pk_all.view(n, osz)]).reshape(-1).contiguous()
                # term order: proof-major inside each of the two output families, so that a sum's terms are adjacent
                order = torch.cat([torch.stack([torch.arange(n), n + torch.arange(n)], 1).reshape(-1),
                                   torch.stack([2 * n + torch.arange(n), 3 * n + torch.arange(n), 4 * n + torch.arange(n)], 1).reshape(-1)]).to(dev)
                svec = torch.cat([chs, bps, chs, mps, bps])[order].reshape(-1).contiguous()
                idx = order.to(torch.int32).contiguous()
                offs = torch.cat([torch.arange(0, 2 * n, 2), 2 * n + torch.arange(0, 3 * n + 1, 3)]).to(torch.int64).to(dev)
                keyset = api.KeySet.create_device(sg, bases.data_ptr(), 5 * n, api.FMT_RAW_PROJ, tables=False)
                prod = ops.empty(5 * n * osz)

                def compose():
                    api._check(ops.lib.blsgpu_keyset_mul(keyset.handle, ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(svec.data_ptr()), 5 * n,
                                                         ctypes.c_void_p(prod.data_ptr())))
                    return ops.sum_batch(kgroup, prod, offs, 2 * n)
                base_wall = timed(compose)
                bprof = profiled(compose)
                keyset.close()
                row = {'impl': 'Bls12381G%dImpl' % sg, 'key_group': 'G%d' % kgroup, 'n': n, 'pk': 'shared' if shared else 'per proof',
                       'verify_wall_ms': round(wall * 1e3, 3), 'proofs_per_s': round(n / wall, 1), 'kernel_ms': prof,
                       'joint_ladder_ms': round(joint, 3), 'composition_wall_ms': round(base_wall * 1e3, 3), 'composition_kernel_ms': bprof,
                       'composition_ms': round(sum(bprof.values()), 3), 'composition_over_joint': round(sum(bprof.values()) / joint, 2) if joint else None,
                       'reps': a.reps}
                print(json.dumps(row), flush=True)
                rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
