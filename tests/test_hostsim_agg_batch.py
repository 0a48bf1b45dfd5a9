"""The per-item functions of the batched aggregate verify (csrc/agg_batch.cuh) on the host, against Python models on random ragged
inputs: the segmented duplicate rule against a dict per set, the segmented first-identity reduction against min(), the
segmented product's index arithmetic against a product per set, the precedence against the reference's order."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util

NONE = 0xffffffff
PRIME = 2 ** 61 - 1


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_agg_batch', 'agg_batch_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='agg_batch_hostsim_')
    so = os.path.join(d, 'libagg_batch_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    lb.hs_agg_hash.restype = ctypes.c_uint64
    lb.hs_agg_hash.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
    lb.hs_agg_fold.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p]
    return lb


def u32(v):
    return (ctypes.c_uint32 * max(len(v), 1))(*v)


def u64(v):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def ragged(rng, sizes):
    """boffs, sid of the flat list; plus a scattered src map (the caller's pair index of every item), as a call with large sets
    between the batched ones has."""
    boffs = [0]
    for t in sizes:
        boffs.append(boffs[-1] + t)
    sid = [b for b, t in enumerate(sizes) for _ in range(t)]
    src, at = [], 0
    for t in sizes:
        at += rng.choice([0, 0, 3, 70])
        src += list(range(at, at + t))
        at += t
    return boffs, sid, src, at


def random_sizes(rng):
    """A ragged list of set sizes: empty and one-pair sets, sizes at and around a workgroup of 64 lanes, a few larger ones."""
    return [rng.choice([0, 0, 1, 1, 2, 3, 5, 17, 63, 64, 65, 100, 129, 300]) for _ in range(rng.randrange(1, 24))]


SIZE_SETS = [
    [0, 1, 0, 2, 3, 1, 0],
    [1] * 70,                                # one-pair sets across a workgroup boundary
    [60, 9, 0, 130, 1, 63, 64, 65, 0],       # sets that cross one and two boundaries of 64 lanes
    [5, 0, 0, 0, 7],
    [200],
]


@pytest.mark.parametrize('sizes', SIZE_SETS + [None], ids=lambda s: 'random' if s is None else 'x'.join(map(str, s))[:24])
@pytest.mark.parametrize('tight', [False, True], ids=['cap2n', 'cap-tight'])
def test_segmented_duplicate_rule(lib, sizes, tight):
    rng = random.Random(str(sizes) + str(tight))
    for trial in range(6):
        sz = sizes if sizes is not None else random_sizes(rng)
        boffs, sid, src, n_src = ragged(rng, sz)
        T = boffs[-1]
        # few distinct messages, so that sets repeat them within and across sets: empty ones, prefixes of one another
        pool = [b'', b'a', b'ab', b'abc', b'abcd', b'\x00', b'\x00\x00', b'm' * 40, b'm' * 41] + [bytes([rng.randrange(256)]) * rng.randrange(1, 9) for _ in range(rng.randrange(1, 60))]
        all_msgs = [b'unused %d' % i for i in range(n_src + 1)]
        for i in range(T):
            all_msgs[src[i]] = rng.choice(pool)
        moffs = [0]
        for m in all_msgs:
            moffs.append(moffs[-1] + len(m))
        blob = b''.join(all_msgs)
        cap = 2
        while cap <= (T if tight else max(2 * T, 63)):      # tight: the smallest table that still has a free slot, so chains collide
            cap *= 2
        order = list(range(T))
        if trial % 2:
            rng.shuffle(order)                           # any interleaving of the lanes gives the same pairs
        out = (ctypes.c_uint32 * (2 * max(len(sz), 1)))()
        lib.hs_agg_dup(T, len(sz), blob, u64(moffs), u32(sid), u32(src), u64(boffs), cap, u32(order), out)
        for b, t in enumerate(sz):
            seen, want = {}, (NONE, NONE)
            for l in range(t):
                m = all_msgs[src[boffs[b] + l]]
                if m in seen:
                    want = (seen[m], l)
                    break
                seen[m] = l
            assert (out[2 * b], out[2 * b + 1]) == want, (sz, b, trial)


def test_hash_separates_sets_lengths_and_prefixes(lib):
    h = lib.hs_agg_hash
    assert h(0, b'', 0) != h(1, b'', 0)
    assert h(3, b'abc', 3) != h(3, b'abc', 2) and h(3, b'ab', 2) == h(3, b'abc', 2)
    assert h(0, b'\x00', 1) != h(0, b'', 0)


@pytest.mark.parametrize('fixed', SIZE_SETS + [None], ids=lambda s: 'random' if s is None else 'x'.join(map(str, s))[:24])
def test_segmented_first_identity(lib, fixed):
    rng = random.Random(str(fixed))
    for trial in range(8):
        sizes = fixed if fixed is not None else random_sizes(rng)
        boffs, sid, _, _ = ragged(rng, sizes)
        T, n_b = boffs[-1], len(sizes)
        p = rng.choice([0.0, 0.02, 0.3, 1.0])
        bad = [1 if rng.random() < p else 0 for _ in range(T + n_b)]
        order = list(range(T + n_b))
        rng.shuffle(order)
        first, sig_id = (ctypes.c_uint32 * n_b)(), (ctypes.c_uint32 * n_b)()
        lib.hs_agg_first_bad(T, n_b, u32(sid), u64(boffs), (ctypes.c_int32 * (T + n_b))(*bad), u32(order), first, sig_id)
        for b, t in enumerate(sizes):
            idx = [l for l in range(t) if bad[boffs[b] + l]]
            assert first[b] == (min(idx) if idx else NONE), (sizes, b)
            assert sig_id[b] == bad[T + b]


@pytest.mark.parametrize('sizes', SIZE_SETS + [[4095], [1, 4095, 1]] + [random_sizes(random.Random(seed)) for seed in range(12)],
                         ids=lambda s: 'x'.join(map(str, s))[:24])
def test_segmented_product_indices(lib, sizes):
    rng = random.Random(str(sizes))
    boffs, sid, _, _ = ragged(rng, sizes)
    T, n_b = boffs[-1], len(sizes)
    vals = [rng.randrange(1, PRIME) for _ in range(T + n_b)]
    f, rec, products = u64(vals), (ctypes.c_uint64 * n_b)(), ctypes.c_uint64(0)
    tmax = max(sizes)
    nr = lib.hs_agg_fold(T, n_b, u32(sid), u64(boffs), tmax, f, rec, ctypes.byref(products))
    assert nr == (max(tmax, 1) - 1).bit_length()         # launches depend on the largest set only
    assert products.value == sum(t - 1 for t in sizes if t)   # work proportional to T: every item enters exactly one product
    for b, t in enumerate(sizes):
        want = vals[T + b]
        for l in range(t):
            want = want * vals[boffs[b] + l] % PRIME
        assert rec[b] == want, (sizes, b)


def test_precedence(lib):
    aux = (ctypes.c_uint64 * 2)()
    d = lib.hs_agg_decide
    assert d(1, 3, 1, 0, aux) == 4 and list(aux) == [1, 3]          # duplicate first, whatever else holds
    assert d(NONE, NONE, 1, 0, aux) == 2 and list(aux) == [0, 0]    # then the identity signature
    assert d(NONE, NONE, 0, 0, aux) == 3 and list(aux) == [1, 0]    # then the first identity key, 1-based
    assert d(NONE, NONE, 0, 6, aux) == 3 and list(aux) == [7, 0]
    assert d(NONE, NONE, 0, NONE, aux) == 0 and list(aux) == [0, 0]  # the pairing product decides
