"""The strip plan of the batched multi verify (csrc/multi_batch.cuh: multi_strip_len, multi_strip_plan, multi_strip_of) and the
fold predicate its strips go through (csrc/shares.cuh share_fold_adds) on the host, with integers mod 2^61 - 1 in place of points:
every key is read by exactly one strip of its own set, strip_sid and strip_offs agree, and after the fold levels
part[strip_offs[s]] is the set's sum -- for every strip length the knob can force and for the default rule."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util

PRIME = 2 ** 61 - 1
UNTOUCHED = 2 ** 64 - 1


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_multi_batch', 'multi_batch_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='multi_batch_hostsim_')
    so = os.path.join(d, 'libmulti_batch_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    lb.hs_multi_strip_len.restype = ctypes.c_uint64
    lb.hs_multi_strip_len.argtypes = [ctypes.c_uint64] * 3
    vp = ctypes.c_void_p
    lb.hs_multi_run.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp]
    return lb


def accumulate_lanes(n, cap=57344):
    """blsgpu.hip accumulate_lanes: a quarter of the points, at least 64, capped, in whole workgroups of 64."""
    return (min(max(n // 4, 64), cap) + 63) // 64 * 64


def random_sizes(rng):
    return [rng.choice([0, 0, 1, 1, 2, 3, 5, 17, 63, 64, 65, 100, 129, 300]) for _ in range(rng.randrange(1, 24))]


SIZE_SETS = [
    [0, 1, 0, 2, 3, 1, 0],
    [1] * 70,                                # one-key sets across a workgroup boundary
    [60, 9, 0, 130, 1, 63, 64, 65, 0],       # sets that cross one and two boundaries of 64 lanes
    [5, 0, 0, 0, 7],
    [200],
] + [random_sizes(random.Random(seed)) for seed in range(8)]
# forced strip lengths (BLSGPU_MULTI_STRIP), and the default rule (None) with the library's lane count and with very few lanes
STRIPS = [1, 3, 4, 64, 10 ** 9, None, 'few-lanes']


def test_strip_length_rule(lib):
    f = lib.hs_multi_strip_len
    assert f(0, 64, 0) == 4 and f(200, 64, 0) == 4 and f(257, 64, 0) == 5
    assert f(524288, accumulate_lanes(524288), 0) == 10         # 1,024 sets x 512 keys: ceil(524,288 / 57,344)
    assert f(131072, accumulate_lanes(131072), 0) == 4
    assert f(10 ** 6, 57344, 1) == 1 and f(5, 64, 2 ** 32) == 2 ** 32


@pytest.mark.parametrize('L', STRIPS, ids=lambda v: 'L=%s' % v)
@pytest.mark.parametrize('sizes', SIZE_SETS, ids=lambda s: 'x'.join(map(str, s))[:24])
def test_strips_cover_every_key_once_and_fold_to_the_sum(lib, sizes, L):
    rng = random.Random(str(sizes))
    offs = [0]
    for t in sizes:
        offs.append(offs[-1] + t)
    N, n_sets = offs[-1], len(sizes)
    if L is None:
        L = lib.hs_multi_strip_len(N, accumulate_lanes(N), 0)
        assert L == max(4, -(-N // accumulate_lanes(N)))
    elif L == 'few-lanes':
        L = lib.hs_multi_strip_len(N, 7, 0)
        assert L == max(4, -(-N // 7))
    else:
        assert lib.hs_multi_strip_len(N, accumulate_lanes(N), L) == L
    vals = [rng.randrange(1, PRIME) for _ in range(N)]
    u64 = lambda v: (ctypes.c_uint64 * max(len(v), 1))(*v)
    key_offs, cvals = u64(offs), u64(vals)
    soffs, sid = (ctypes.c_uint64 * (n_sets + 1))(), (ctypes.c_uint32 * max(N, 1))()
    reads = (ctypes.c_uint32 * max(N, 1))()
    sums = u64([UNTOUCHED] * n_sets)
    Q, qmax = ctypes.c_uint64(0), ctypes.c_uint64(0)
    levels = lib.hs_multi_run(key_offs, n_sets, L, cvals, soffs, sid, max(N, 1), reads, sums, ctypes.byref(Q), ctypes.byref(qmax))
    assert levels >= 0, levels
    q = [-(-t // L) for t in sizes]
    assert list(soffs) == [sum(q[:s]) for s in range(n_sets + 1)]          # an empty set gets no strip
    assert Q.value == sum(q) and list(sid)[:Q.value] == [s for s in range(n_sets) for _ in range(q[s])]
    assert qmax.value == max(q) and levels == (max(max(q), 1) - 1).bit_length()     # launches depend on the widest set only
    assert list(reads)[:N] == [1] * N
    for s, t in enumerate(sizes):
        assert sums[s] == (sum(vals[offs[s]:offs[s + 1]]) % PRIME if t else UNTOUCHED), (sizes, L, s)
