#!/usr/bin/env python3
"""Timestamp proofs of knowledge: what deriving the challenge on the device costs and saves.

usage: python tools/bench_pok_timestamp.py [--reps 5] [--sizes 4096,65536] [--out profiles/pok_timestamp_bench.json]
Per orientation and size, on valid proofs that live on the device (TensorOps):
  (a) blsgpu_sig_proof_timestamp_verify_batch                       the one call
  (b) blsgpu_sig_proof_verify_batch, challenges already computed    the entry point a caller had before, and the floor of (a)
  (c) blsgpu_sig_proof_challenge_batch alone
  (d) per-kernel device times of (a) from blsgpu_profile_*
  (e) one host thread deriving the same challenges in the tool's own C++ (tools/pok_host_derive.cpp: affine, compress, HKDF,
      reduce) -- what a caller of (b) did before
The proofs are a pool of 4,096 distinct (U, V, pk, t, msg) made with blsgpu_sign_batch (U = x H(m), V = -(x + y) sk H(m) with y
from (c)), tiled to the size; every item is valid, so every item runs the whole check.  Prints one JSON line per shape and writes
them all to --out."""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
POOL = 4096
NOW, TIMEOUT = 1_700_000_000_000, 60_000


def host_lib():
    so = os.path.join(tempfile.mkdtemp(prefix='pok_host_'), 'libpok_host.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tools', 'pok_host_derive.cpp')])
    lb = ctypes.CDLL(so)
    lb.pok_host_derive.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    return lb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='4096,65536')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pok_timestamp_bench.json'))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    host = host_lib()
    rng = random.Random(2026)
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

    def dev_bytes(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    for sg in (1, 2):
        ssz, psz = 144 * sg, 144 * (3 - sg)
        scheme = api.POP
        sks = [rng.randrange(1, R) for _ in range(POOL)]
        xs = [rng.randrange(1, R) for _ in range(POOL)]
        msgs = [b'pok-bench-%05d' % i for i in range(POOL)]
        tms = [NOW - rng.randrange(TIMEOUT) for _ in range(POOL)]
        pks, _ = api.sign_batch(sg, scheme, sks, msgs)
        _, us = api.sign_batch(sg, scheme, xs, msgs)                                       # U = x H(m)
        ys = api.sig_proof_challenge_batch(sg, us, tms)
        _, vs = api.sign_batch(sg, scheme, [(R - (x + y) * sk % R) % R for x, y, sk in zip(xs, ys, sks)], msgs)     # V = -(x + y) sk H(m)
        for n in [int(x) for x in a.sizes.split(',')]:
            rep = (n + POOL - 1) // POOL
            tile = lambda col: (b''.join(col) * rep)[:len(col[0]) * n]
            u_h = tile(us)
            u_t, v_t, pk_t = dev_bytes(u_h), dev_bytes(tile(vs)), dev_bytes(tile(pks))
            t_list = (tms * rep)[:n]
            t_t = torch.tensor(t_list, dtype=torch.int64, device=dev)
            y_t = dev_bytes((b''.join(y.to_bytes(32, 'little') for y in ys) * rep)[:32 * n])
            m_t = dev_bytes(tile(msgs))
            offs = torch.arange(0, (n + 1) * len(msgs[0]), len(msgs[0]), dtype=torch.int64, device=dev)
            one = lambda: ops.sig_proof_timestamp_verify_batch(sg, scheme, u_t, v_t, pk_t, t_t, m_t, offs, n, NOW, TIMEOUT)
            two = lambda: ops.sig_proof_verify_batch(sg, scheme, u_t, v_t, pk_t, y_t, m_t, offs, n)
            chal = lambda: ops.sig_proof_challenge_batch(sg, u_t, t_t, n)
            assert one().eq(0).all().item() and two().eq(0).all().item()
            assert bytes(chal().cpu().tolist()) == bytes(y_t.cpu().tolist())
            wall_a, wall_b, wall_c = timed(one), timed(two), timed(chal)
            prof = profiled(one)
            # (e): one host thread, once (it is serial work: seconds at the large size)
            out = ctypes.create_string_buffer(32 * n)
            t_h = (ctypes.c_uint64 * n)(*t_list)
            t0 = time.perf_counter()
            host.pok_host_derive(sg, u_h, ctypes.cast(t_h, ctypes.c_void_p), n, out)
            wall_e = time.perf_counter() - t0
            assert out.raw == bytes(y_t.cpu().tolist())
            row = {'impl': 'Bls12381G%dImpl' % sg, 'n': n, 'timestamp_verify_wall_ms': round(wall_a * 1e3, 3),
                   'verify_given_challenges_wall_ms': round(wall_b * 1e3, 3), 'a_minus_b_ms': round((wall_a - wall_b) * 1e3, 3),
                   'challenge_batch_wall_ms': round(wall_c * 1e3, 3), 'kernel_ms': prof,
                   'k_proof_challenge_ms': prof.get('k_proof_challenge'), 'k_prepare_ms': prof.get('k_prepare'),
                   'host_thread_derive_ms': round(wall_e * 1e3, 1), 'host_over_device_challenge': round(wall_e / wall_c, 1),
                   'proofs_per_s': round(n / wall_a, 1), 'reps': a.reps}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
