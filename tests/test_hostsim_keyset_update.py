"""The position rule of blsgpu_keyset_update and blsgpu_keyset_append (csrc/keyset.cuh keyset_positions_check) on the host: which
lists of positions an update accepts -- every position below the set's size, none twice, the range decided first -- and how far an
append may grow a set (2^32 - 2 entries, as at creation).  A Python restatement gives the expected outputs.  The same driver runs
once more as a stand-alone program under the address and undefined-behaviour sanitizers (a host build, nothing preloaded)."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util

SRC = os.path.join(util.ROOT, 'tests', 'hostsim_keyset_update', 'keyset_update_hostsim.cpp')
OK, RANGE, DUP, FULL = 0, 1, 2, 3
TOP = 2 ** 32 - 2


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='keyset_update_hostsim_'), 'libkeyset_update_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_update_rule.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    lb.hs_append_rule.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return lb


def update_rule(pos, n_keys):
    """the rule restated: a position outside the set first, then a position named twice"""
    if any(p >= n_keys for p in pos):
        return RANGE
    return DUP if len(set(pos)) != len(pos) else OK


def append_rule(n_keys, count):
    return OK if n_keys + count <= TOP else FULL


def got(lib, pos, n_keys):
    arr = (ctypes.c_uint32 * max(len(pos), 1))(*pos)
    return lib.hs_update_rule(ctypes.cast(arr, ctypes.c_void_p), len(pos), n_keys)


N = 320
CASES = [
    ('empty list', [], N, OK),
    ('empty list, empty set', [], 0, OK),
    ('one position', [0], N, OK),
    ('one position, empty set', [0], 0, RANGE),
    ('n - 1', [N - 1], N, OK),
    ('n', [N], N, RANGE),
    ('2^32 - 1', [2 ** 32 - 1], N, RANGE),
    ('sorted', [1, 2, 3, 63, 64, 65], N, OK),
    ('unsorted', [65, 0, N - 1, 64, 5, 63], N, OK),
    ('reversed', list(range(9, -1, -1)), N, OK),
    ('duplicate at distance 1', [1, 7, 7, 9], N, DUP),
    ('duplicate, nothing else', [4, 4], N, DUP),
    ('duplicate at the two ends', [7, 1, 2, 3, 7], N, DUP),
    ('range before duplicates', [7, 1, 2, 3, 7, N], N, RANGE),
    ('n - 1 and n', [N - 1, N], N, RANGE),
    ('a whole table reversed', list(range(4099, -1, -1)), 4100, OK),
    ('... over a set one entry shorter', list(range(4099, -1, -1)), 4099, RANGE),
    ('... with its ends equal', list(range(4099, 0, -1)) + [4099], 4100, DUP),
]


@pytest.mark.parametrize('name,pos,n_keys,want', CASES, ids=[c[0] for c in CASES])
def test_update_rule(lib, name, pos, n_keys, want):
    assert update_rule(pos, n_keys) == want
    assert got(lib, pos, n_keys) == want


def test_update_rule_on_random_lists(lib):
    rng = random.Random(8)
    seen = set()
    for _ in range(300):
        n_keys = rng.choice([1, 2, 64, 65, N])
        pos = [rng.randrange(n_keys + (rng.random() < 0.2)) for _ in range(rng.randrange(0, min(2 * n_keys, 40)))]
        if rng.random() < 0.5:
            pos = list(dict.fromkeys(pos))
        want = update_rule(pos, n_keys)
        seen.add(want)
        assert got(lib, pos, n_keys) == want, (pos, n_keys)
    assert seen == {OK, RANGE, DUP}


def test_append_rule(lib):
    """a set may grow to exactly 2^32 - 2 entries and not one further; no sum wraps around"""
    for n_keys, count in ((0, 0), (0, 1), (0, TOP), (0, TOP + 1), (N, 65), (N, TOP - N), (N, TOP - N + 1), (TOP, 0), (TOP, 1), (TOP - 1, 1), (TOP - 1, 2),
                          (N, 2 ** 64 - 1), (1, 2 ** 64 - 1), (TOP, 2 ** 64 - 1)):
        assert lib.hs_append_rule(n_keys, count) == append_rule(n_keys, count), (n_keys, count)
    assert append_rule(N, TOP - N) == OK and append_rule(N, TOP - N + 1) == FULL


def test_standalone_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix='keyset_update_hostsim_san_'), 'keyset_update_hostsim')
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DKEYSET_UPDATE_HOSTSIM_MAIN', '-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert p.stdout.strip().endswith(' 0 bad')
