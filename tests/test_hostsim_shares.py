"""The threshold-recovery device functions (csrc/fr.cuh, csrc/shares.cuh) on the host, bound tracker on, against Python integers
and the oracle's point multiplication: Fr arithmetic at its edges, the canonical check, the per-share Lagrange function (with
zeros and duplicates), the NAF recoding and the per-share ladder."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util
from util import c

R = c.R
RINV = pow(2 ** 256, -1, R)


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_shares', 'shares_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='shares_hostsim_')
    so = os.path.join(d, 'libshares_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    lb.hs_lagrange.restype = ctypes.c_uint32
    return lb


def w(v):
    return (ctypes.c_uint32 * 8)(*[(v >> (32 * j)) & 0xffffffff for j in range(8)])


def val(a):
    return sum(int(a[j]) << (32 * j) for j in range(8))


EDGE = [0, 1, 2, R - 1, R - 2, (2 ** 255 - 1) % R, 2 ** 255 % R, 2 ** 256 % R, (2 ** 256 - 1) % R, R // 2, R // 2 + 1, 2 ** 32, 2 ** 224 - 1]


def test_fr_arithmetic(lib):
    rng = random.Random(1)
    vals = EDGE + [rng.randrange(R) for _ in range(300)]
    out = (ctypes.c_uint32 * 8)()
    pairs = [(a, b) for a in EDGE for b in EDGE] + [(rng.choice(vals), rng.choice(vals)) for _ in range(400)]
    for a, b in pairs:
        lib.hs_fr_op(0, w(a), w(b), out)
        assert val(out) == a * b % R, (a, b)
        lib.hs_fr_op(1, w(a), w(b), out)
        assert val(out) == (a - b) % R, (a, b)
    for a in vals:
        lib.hs_fr_op(2, w(a), w(0), out)
        assert val(out) == (pow(a, R - 2, R)), a
    # non-canonical 256-bit inputs reduce; the raw Montgomery product at its bounds (a up to 2^256 - 1, b up to r - 1)
    for a in [R, R + 1, 2 ** 256 - 1, 2 ** 255, 2 * R - 1] + [rng.randrange(2 ** 256) for _ in range(100)]:
        lib.hs_fr_op(3, w(a), w(0), out)
        assert val(out) == a % R
        for b in (0, 1, R - 1, R - 2, rng.randrange(R)):
            lib.hs_fr_mont_mul(w(a), w(b), out)
            assert val(out) == a * b * RINV % R, (a, b)


def test_fr_canonical(lib):
    for v, want in ((0, 1), (R - 1, 1), (R, 0), (R + 1, 0), (2 ** 256 - 1, 0), (2 ** 255, 0), (R - 2 ** 200, 1)):
        assert lib.hs_fr_canonical(w(v)) == want, hex(v)


def lagrange_py(xs, i):
    num = den = 1
    for j, xj in enumerate(xs):
        if j != i:
            num = num * xj % R
            den = den * (xj - xs[i]) % R
    return num * pow(den, R - 2, R) % R


def test_lagrange_per_share(lib):
    rng = random.Random(2)
    lam = (ctypes.c_uint32 * 8)()
    for t in (2, 3, 5, 17, 64, 65):
        for kind in ('random', 'small', 'dup', 'zero'):
            xs = [rng.randrange(1, R) for _ in range(t)] if kind != 'small' else rng.sample(range(1, 256), t)
            if kind == 'dup':
                xs[rng.randrange(1, t)] = xs[0]
            if kind == 'zero':
                xs[rng.randrange(t)] = 0
            ids = (ctypes.c_uint32 * (8 * t))(*[(x >> (32 * j)) & 0xffffffff for x in xs for j in range(8)])
            for i in range(t):
                f = lib.hs_lagrange(ids, t, i, lam)
                bad = xs[i] == 0 or xs.count(xs[i]) > 1
                assert (f != 0) == bad, (t, kind, i)
                if kind in ('random', 'small') or (kind == 'zero' and not bad):
                    assert val(lam) == lagrange_py(xs, i), (t, kind, i)
            if kind in ('random', 'small'):       # the coefficients interpolate: sum lambda_i f(x_i) = f(0)
                coeffs = [rng.randrange(R) for _ in range(t)]
                fx = [sum(cf * pow(x, e, R) for e, cf in enumerate(coeffs)) % R for x in xs]
                tot = 0
                for i in range(t):
                    lib.hs_lagrange(ids, t, i, lam)
                    tot += val(lam) * fx[i]
                assert tot % R == coeffs[0]


def test_naf(lib):
    rng = random.Random(3)
    pos, neg = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
    for words, top in ((1, 64), (2, 128)):
        for k in [0, 1, 3, 2 ** top - 1, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa] + [rng.randrange(2 ** top) for _ in range(200)]:
            kw = (ctypes.c_uint64 * 2)(k & (2 ** 64 - 1), k >> 64)
            lib.hs_naf(kw, words, pos, neg)
            p = sum(int(pos[j]) << (64 * j) for j in range(3))
            n = sum(int(neg[j]) << (64 * j) for j in range(3))
            assert p - n == k and p & n == 0 and (p | n) & ((p | n) >> 1) == 0      # non-adjacent
            assert (p | n) < 2 ** (top + 1)


def test_share_ladder(lib):
    rng = random.Random(4)
    out = ctypes.create_string_buffer(96)
    z = 0xd201000000010000
    lams = [0, 1, 2, R - 1, R - 2, z, z * z, z ** 3 % R, 2 ** 254] + [rng.randrange(R) for _ in range(6)]
    for group, E, gen, raw, comp in ((1, c.E1, c.G1_GEN, util.g1_raw, c.g1_compress), (2, c.E2, c.G2_GEN, util.g2_raw, c.g2_compress)):
        for P in [E.mul(gen, rng.randrange(1, R)) for _ in range(3)] + [None]:
            for lam in lams:
                lib.hs_share_ladder(group, raw(P, rng), w(lam), out)
                assert out.raw[:48 * group] == comp(E.mul(P, lam) if P is not None else None), (group, hex(lam))
