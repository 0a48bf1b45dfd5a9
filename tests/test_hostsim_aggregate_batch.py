"""The first-occurrence search of the batched secure aggregation (csrc/secure.cuh secure_first_tile, the body of k_secure_first)
on the host: for every key of every set, the flat index of the first key OF ITS SET with the same bytes -- the reference's
`position` search (src/secure_aggregation.rs:138-147) -- against Python's list.index per set, for 48- and 96-byte keys, one and
several tile slices (gridDim.y), and sets the kernel skips."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_aggregate_batch', 'aggregate_batch_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='aggregate_batch_hostsim_')
    so = os.path.join(d, 'libaggregate_batch_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lb.hs_secure_first.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp]
    return lb


def fresh(rng, width, t):
    keys = set()
    while len(keys) < t:
        keys.add(bytes([rng.randrange(256) for _ in range(4)]) * (width // 4 - 1) + rng.randbytes(4))   # keys that differ late, too
    out = list(keys)
    rng.shuffle(out)
    return out


def make_sets(rng, width):
    """the shapes of the issue; every entry is one set's key list"""
    sets = [[], fresh(rng, width, 1), fresh(rng, width, 2)]
    k = fresh(rng, width, 1)
    sets.append(k * 2)                                            # two keys, equal
    for t in (63, 64, 65):                                        # duplicates on both sides of the 64-key tile boundary
        k = fresh(rng, width, t)
        k[t - 1] = k[0]
        if t > 2:
            k[t // 2] = k[1]
        if t == 65:
            k[64] = k[63]                                         # neighbours across the boundary
            k[62] = k[5]
        sets.append(k)
    k = fresh(rng, width, 130)
    k[129] = k[3]                                                 # two tiles later
    sets.append(k)
    k = fresh(rng, width, 70)
    k[20] = k[40] = k[7]                                          # triplicates, one of them across the boundary
    k[69] = k[66] = k[64]
    sets.append(k)
    shared = fresh(rng, width, 3)                                 # the same bytes in two different sets: no match across sets
    sets.append(shared + fresh(rng, width, 4))
    sets.append(fresh(rng, width, 2) + shared[::-1])
    sets.append([shared[0]])
    sets.append([])
    sets.append(fresh(rng, width, 1) * 100)                       # all keys equal
    return sets


def run(lib, sets, width, S=1, large=()):
    offs = [0]
    for k in sets:
        offs.append(offs[-1] + len(k))
    n = offs[-1]
    blob = b''.join(x for k in sets for x in k)
    first = (ctypes.c_uint32 * max(n, 1))()
    lg = bytes(1 if s in large else 0 for s in range(len(sets)))
    rc = lib.hs_secure_first(blob, width // 4, (ctypes.c_uint64 * len(offs))(*offs), len(sets), lg, S, first)
    assert rc == 0, rc
    return offs, list(first)[:n]


def expect(sets, offs, large=()):
    return [0xffffffff if s in large else offs[s] + k.index(x) for s, k in enumerate(sets) for x in k]


@pytest.mark.parametrize('S', [1, 2, 3])
@pytest.mark.parametrize('width', [48, 96])
def test_first_occurrence_per_set(lib, width, S):
    rng = random.Random(1000 * width + S)
    sets = make_sets(rng, width)
    offs, got = run(lib, sets, width, S)
    assert got == expect(sets, offs)
    # the cases the list is there for, spelled out
    s130 = next(s for s, k in enumerate(sets) if len(k) == 130)
    assert got[offs[s130] + 129] == offs[s130] + 3
    assert got[offs[-1] - 100:] == [offs[-1] - 100] * 100
    # rotated, so that every set meets the workgroup and tile boundaries somewhere else
    for r in (1, 5):
        rs = sets[r:] + sets[:r]
        offs, got = run(lib, rs, width, S)
        assert got == expect(rs, offs)


@pytest.mark.parametrize('width', [48, 96])
def test_sizes_0_1_2_alone(lib, width):
    rng = random.Random(width)
    for sets in ([[]], [fresh(rng, width, 1)], [fresh(rng, width, 2)], [fresh(rng, width, 1) * 2], [[], [], []]):
        offs, got = run(lib, sets, width)
        assert got == expect(sets, offs)


def test_skipped_sets_stay_untouched_and_are_never_matched(lib):
    """a set the kernel skips (SECURE_F_LARGE: it runs through the single call's steps) between two small ones that hold its bytes"""
    rng = random.Random(7)
    k = fresh(rng, 48, 70)
    sets = [k[:10] + k[:1], k + k[:5], [k[69], k[0], k[69]]]
    offs, got = run(lib, sets, 48, 2, large={1})
    assert got == expect(sets, offs, large={1})


def test_random_batches(lib):
    rng = random.Random(99)
    for _ in range(30):
        width = rng.choice([48, 96])
        pool = fresh(rng, width, 12)
        sets = [[rng.choice(pool) if rng.random() < 0.5 else fresh(rng, width, 1)[0] for _ in range(rng.choice([0, 1, 2, 5, 64, 65, 129, 200]))]
                for _ in range(rng.randrange(1, 9))]
        offs, got = run(lib, sets, width, rng.choice([1, 2, 4]))
        assert got == expect(sets, offs)
