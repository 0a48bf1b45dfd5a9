"""The recoding header of the registered key sets (csrc/keyset.cuh) on the host: the signed 4-bit digits of every endomorphism
sub-scalar reconstruct it, stay inside the table's rows, and fill exactly the table's windows, the carry window included; the
precedence key orders an out-of-range index before the first invalid entry in input order.  The same driver runs once more as a
stand-alone program under the address and undefined-behaviour sanitizers (a host build, nothing preloaded).  Also the host helper
indices_from_bits of the Python layer."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util
from util import c

SRC = os.path.join(util.ROOT, 'tests', 'hostsim_keyset', 'keyset_hostsim.cpp')
Z = c.X_ABS
R = c.R


@pytest.fixture(scope='module')
def lib():
    d = tempfile.mkdtemp(prefix='keyset_hostsim_')
    so = os.path.join(d, 'libkeyset_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_keyset_pre_key.restype = ctypes.c_uint64
    lb.hs_keyset_pre_key.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int32]
    lb.hs_keyset_pre_status.restype = ctypes.c_int32
    lb.hs_keyset_pre_status.argtypes = [ctypes.c_uint64]
    return lb


def shape(lib, G):
    out = (ctypes.c_int * 7)()
    lib.hs_keyset_shape(G, out)
    return dict(zip(('E', 'WORDS', 'FULL', 'WINDOWS', 'POINTS', 'W', 'ROW'), out))


def recode(lib, G, a):
    s = shape(lib, G)
    words = (ctypes.c_uint64 * s['WORDS'])(*[(a >> (64 * k)) & (2 ** 64 - 1) for k in range(s['WORDS'])])
    digits, recs = (ctypes.c_int32 * s['WINDOWS'])(), (ctypes.c_uint32 * s['WINDOWS'])()
    carry = lib.hs_keyset_recode(G, words, digits, recs)
    return list(digits), list(recs), carry


def decompose(lib, G, k):
    kw = (ctypes.c_uint32 * 8)(*[(k >> (32 * j)) & 0xffffffff for j in range(8)])
    a = (ctypes.c_uint64 * 4)()
    lib.hs_keyset_decompose(G, kw, a)
    return [a[0] | a[1] << 64, a[2] | a[3] << 64] if G == 1 else list(a)


@pytest.mark.parametrize('G', [1, 2])
def test_shape(lib, G):
    s = shape(lib, G)
    bits = 128 if G == 1 else 64                          # one endomorphism sub-scalar: G1 keys split in two, G2 keys in four
    assert 3 <= s['W'] <= 5 and s['ROW'] == 2 ** (s['W'] - 1)
    assert s['E'] * bits == 256 and s['WORDS'] * 64 == bits
    assert s['FULL'] * s['W'] == bits and s['WINDOWS'] == s['FULL'] + 1           # the carry of the top window has a window of its own
    assert s['POINTS'] == s['FULL'] * s['ROW'] + 1                                # ... which holds the digit 1 alone


@pytest.mark.parametrize('G', [1, 2])
def test_digits_reconstruct_every_sub_scalar(lib, G):
    s = shape(lib, G)
    w, bits = s['W'], s['WORDS'] * 64
    rng = random.Random(G)
    top = 2 ** bits - 1
    carries = [sum(d << (w * j) for j in range(s['FULL'])) for d in (2 ** w - 1, 2 ** (w - 1) + 1, 9, 12)]      # every window carries
    # the largest magnitudes msm2_decompose_* returns: base-z digits below z (G2); a0 < z^2, a1 <= r / z^2 (G1)
    largest = [Z - 1, Z - 2] if G == 2 else [Z * Z - 1, R // (Z * Z), (Z - 1) * Z + Z - 1]
    vals = [0, 1, 2 ** w - 1, 2 ** (w - 1), 2 ** (w - 1) + 1, top, top - 1, 2 ** (bits - 1), 2 ** (bits - 1) - 1] + carries + largest
    vals += [rng.randrange(2 ** bits) for _ in range(2000)]
    for k in [R - 1, R, R + 1, 2 ** 256 - 1, 2 ** 255, Z, Z * Z, R - Z * Z] + [rng.randrange(2 ** 256) for _ in range(300)]:
        subs = decompose(lib, G, k)
        assert all(0 <= a < 2 ** bits for a in subs) and all(a <= max(largest) for a in subs), hex(k)
        if G == 1:
            assert (subs[0] + subs[1] * Z * Z - k) % R == 0
        else:
            assert (sum(a * Z ** j for j, a in enumerate(subs)) - k) % R == 0
        vals += subs
    nonzero = 0
    for a in vals:
        digits, recs, carry = recode(lib, G, a)
        assert carry == 0 and len(digits) == s['WINDOWS']                      # as many windows as the table has
        assert sum(d << (w * j) if d >= 0 else -((-d) << (w * j)) for j, d in enumerate(digits)) == a, hex(a)
        assert all(-s['ROW'] < d <= s['ROW'] for d in digits) and digits[s['FULL']] in (0, 1)
        for j, (d, r) in enumerate(zip(digits, recs)):
            if d:
                assert r == j * s['ROW'] + abs(d) - 1 and r < s['POINTS']      # one contiguous record per (window, digit)
        nonzero += sum(1 for d in digits if d)
    assert recode(lib, G, top)[0][s['FULL']] == 1 and recode(lib, G, 0)[0] == [0] * s['WINDOWS']
    assert nonzero / len(vals) < s['WINDOWS']


def test_precedence_key(lib):
    key, status = lib.hs_keyset_pre_key, lib.hs_keyset_pre_status
    none = 2 ** 64 - 1
    assert key(0, 17, 0) == none
    oob, bad_at_3, legacy_at_2, bad_at_0 = key(1, 9, 0), key(0, 3, 7), key(0, 2, 8), key(0, 0, 7)
    assert status(min(oob, bad_at_3, none)) == -3                        # out of range wins wherever it stands
    assert status(min(bad_at_3, legacy_at_2, none)) == 8                 # else the first invalid entry in input order
    assert status(min(bad_at_3, bad_at_0)) == 7 and bad_at_0 < legacy_at_2
    assert key(0, 2 ** 32 - 2, 8) < none and status(key(0, 2 ** 32 - 2, 8)) == 8


def test_standalone_under_sanitizers():
    d = tempfile.mkdtemp(prefix='keyset_hostsim_san_')
    exe = os.path.join(d, 'keyset_hostsim')
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DKEYSET_HOSTSIM_MAIN', '-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert p.stdout.strip().endswith(' 0 bad')


def test_indices_from_bits(pkg):
    f = pkg.api.indices_from_bits
    assert f(b'') == [] and f(bytes(4)) == []
    assert f(b'\x01') == [0] and f(b'\x80') == [7] and f(b'\x00\x01') == [8]             # little-endian bit order, byte boundary
    assert f(b'\x80\x01') == [7, 8] and f(b'\xff\xff') == list(range(16))
    assert f(b'\x05\x00\x00') == [0, 2] == f(b'\x05') == f(bytearray(b'\x05\x00'))        # trailing zeros name nobody
    assert f(bytes([0, 0, 0, 0x10])) == [28]
    rng = random.Random(3)
    for _ in range(50):
        want = sorted(rng.sample(range(400), rng.randrange(0, 60)))
        bits = bytearray(50)
        for i in want:
            bits[i // 8] |= 1 << (i % 8)
        assert f(bits) == want
