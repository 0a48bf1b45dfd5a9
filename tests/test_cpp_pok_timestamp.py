"""The proof-of-knowledge types of the C++ host mirror (include/blsful_hip.hpp: ProofCommitmentChallenge, ProofOfKnowledge,
ProofOfKnowledgeTimestamp) and their test program tests/cpp/pok_timestamp_test.cpp, built with g++ against the C ABI only, as
tests/test_cpp_mirror.py builds its program.  The proofs come from tests/pok_timestamp_cases.py (the oracle) as "key hex" lines.

CPU: the program compiles, links against libblsgpu.so and FAILS LOUDLY without a device (no CPU path).
GPU: one valid and one timed-out proof per orientation pass through the types."""
import os
import random
import subprocess

import pytest

import pok_timestamp_cases as pc
import util
from oracle.py import blsful_ref as ref

ROOT = util.ROOT
LIBDIR = os.path.join(ROOT, 'agora-blsful_amd')


def build(tmp_path, with_proofs):
    exe = str(tmp_path / 'pok_timestamp_test')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'cpp', 'pok_timestamp_test.cpp'), '-L', LIBDIR, '-lblsgpu', '-Wl,-rpath,' + LIBDIR, '-o', exe])
    seed = b'proof commitment challenge seed'
    lines = ['now %d' % pc.NOW, 'timeout %d' % pc.TIMEOUT, 'seed ' + seed.hex(),
             'seed_scalar ' + pc.hash_to_scalar(seed, pc.KEYGEN_SALT).to_bytes(32, 'little').hex()]
    rng = random.Random(9)
    for sg in ((1, 2) if with_proofs else ()):
        scheme = (ref.POP, ref.AUG)[sg - 1]
        u, v, pk, t, msg = pc.items(sg, scheme)['valid']
        pre = 'g%d_' % sg
        lines += [pre + 'scheme %d' % scheme, pre + 't %d' % t, pre + 'msg ' + msg.hex(),
                  pre + 'u ' + pc.render_point(sg, u, pc.RAW_PROJ, rng).hex(), pre + 'v ' + pc.render_point(sg, v, pc.RAW_PROJ, rng).hex(),
                  pre + 'pk ' + pc.render_point(3 - sg, pk, pc.RAW_PROJ, rng).hex(),
                  pre + 'y ' + pc.compute_y(pc.IMPLS[sg], u, t).to_bytes(32, 'little').hex()]
    kat = str(tmp_path / 'pok_kats.txt')
    open(kat, 'w').write('\n'.join(lines) + '\n')
    return exe, kat


def test_cpp_pok_builds_and_needs_a_device(pkg, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by test_cpp_pok_on_gpu')
    exe, kat = build(tmp_path, False)
    p = subprocess.run([exe, kat], capture_output=True, text=True, timeout=120)
    assert p.returncode == 3 and 'no CPU fallback' in p.stdout, (p.returncode, p.stdout, p.stderr)


@pytest.mark.gpu
def test_cpp_pok_on_gpu(pkg, tmp_path):
    exe, kat = build(tmp_path, True)
    p = subprocess.run([exe, kat], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and ' 0 failed' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-2000:])
