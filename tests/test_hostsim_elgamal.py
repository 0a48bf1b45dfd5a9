"""The ElGamal device functions (csrc/elgamal.cuh, csrc/fr.cuh) on the host, bound tracker on: STROBE / Merlin against
tests/merlin_ref.py, the 512-bit reduction against Python integers, the multi-term joint ladder on the related-base cases against
the oracle's scalar multiplication."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import elgamal_cases as ec
import merlin_ref
import util
from util import c

R = c.R


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_elgamal', 'elgamal_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='elgamal_hostsim_')
    so = os.path.join(d, 'libelgamal_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    lb.hs_keccak_f0.restype = ctypes.c_uint64
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    lb.hs_merlin.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.c_char_p, vp, ctypes.c_char_p, sz, vp, sz]
    lb.hs_elgamal_transcript.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, sz, vp]
    return lb


def merlin(lib, label, items, clabel, n):
    flat = b''.join(l + m for l, m in items) or b'\0'
    lens = (ctypes.c_uint64 * (2 * max(len(items), 1)))(*[x for l, m in items for x in (len(l), len(m))])
    out = ctypes.create_string_buffer(n)
    lib.hs_merlin(label, len(label), len(items), flat, ctypes.cast(lens, ctypes.c_void_p), clabel, len(clabel), ctypes.cast(out, ctypes.c_void_p), n)
    return out.raw


def merlin_py(label, items, clabel, n):
    t = merlin_ref.Transcript(label)
    for l, m in items:
        t.append_message(l, m)
    return t.challenge_bytes(clabel, n)


def test_keccak_and_merlin_vector(lib):
    assert lib.hs_keccak_f0() == 0xF1258F7940E1DDE7
    got = merlin(lib, b'test protocol', [(b'some label', b'some data')], b'challenge', 32)
    assert got.hex() == 'd5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615'


def test_merlin_random_transcripts(lib):
    """Message lengths 0 .. 400: an absorb crosses one and two block boundaries (rate 166) at every offset; the squeeze crosses too."""
    rng = random.Random(21)
    for ln in range(0, 401):
        items = [(b'x' * rng.randrange(1, 12), bytes(rng.randrange(256) for _ in range(ln)))]
        if ln % 7 == 0:
            items.append((b'second', bytes(rng.randrange(256) for _ in range(rng.randrange(0, 401)))))
        n = 64 if ln % 50 else 400
        assert merlin(lib, b'proto', items, b'challenge', n) == merlin_py(b'proto', items, b'challenge', n), ln
    # begin_op's two bytes land on the block boundary itself: total position before the operation 164, 165
    for pad in range(100, 180):
        items = [(b'a', bytes(pad)), (b'bb', b'payload')]
        assert merlin(lib, b'p', items, b'c', 64) == merlin_py(b'p', items, b'c', 64), pad


@pytest.mark.parametrize('sg', [1, 2])
def test_proof_transcript_from_prefix(lib, sg):
    g = ec.kg(sg)
    rng = random.Random(22 + sg)
    pts = [g.mul(g.gen, rng.randrange(1, R)) for _ in range(5)] + [None]
    out = ctypes.create_string_buffer(64)
    for _ in range(3):
        rng.shuffle(pts)
        b = [g.to_bytes(p) for p in pts]
        lib.hs_elgamal_transcript(g.to_bytes(g.gen), b''.join(b[:4]), b''.join(b[4:]), g.K, ctypes.cast(out, ctypes.c_void_p))
        assert ec.scalar_from_bytes_wide(out.raw) == ec.challenge(g, *pts)


def w16(v):
    return (ctypes.c_uint32 * 16)(*[(v >> (32 * j)) & 0xffffffff for j in range(16)])


def w8(v):
    return (ctypes.c_uint32 * 8)(*[(v >> (32 * j)) & 0xffffffff for j in range(8)])


def val(a):
    return sum(int(a[j]) << (32 * j) for j in range(8))


def test_reduction_of_512_bits(lib):
    rng = random.Random(23)
    out = (ctypes.c_uint32 * 8)()
    vals = [0, 1, R - 1, R, R + 1, 2 ** 256 - 1, 2 ** 256, 2 ** 512 - 1, 2 ** 511, (2 ** 256 - 1) << 256]
    vals += [R * k for k in (2, 3, 2 ** 255, 2 ** 256 - 1, rng.randrange(2 ** 256))]
    vals += [(2 ** 256 * k) % 2 ** 512 for k in (1, 2, R - 1, R, 2 ** 256 - 1, rng.randrange(2 ** 256))]
    vals += [rng.randrange(2 ** 512) for _ in range(500)]
    for v in vals:
        assert v < 2 ** 512
        lib.hs_fr_from_wide(w16(v), out)
        assert val(out) == v % R, hex(v)
    for v in (1, 2, R - 1, R // 2, rng.randrange(1, R)):
        lib.hs_fr_neg(w8(v), out)
        assert val(out) == R - v


@pytest.mark.parametrize('group', [1, 2])
def test_window_recoding(lib, group):
    """The signed 4-bit windows of a sub-scalar (128 bits in G1, 64 in G2): digits in [-7, 8] that sum back to the value."""
    rng = random.Random(26 + group)
    top = 128 if group == 1 else 64
    dig = (ctypes.c_int8 * 40)()
    vals = [0, 1, 7, 8, 9, 15, 16, 2 ** top - 1, 2 ** (top - 1), int('8' * (top // 4), 16), int('9' * (top // 4), 16), int('7' * (top // 4), 16),
            int('f8' * (top // 8), 16), int('8f' * (top // 8), 16)] + [rng.randrange(2 ** top) for _ in range(300)]
    for k in vals:
        nw = lib.hs_elgamal_recode(group, (ctypes.c_uint64 * 2)(k & (2 ** 64 - 1), k >> 64), dig)
        assert nw == top // 4 + 1
        assert all(-7 <= dig[w] <= 8 for w in range(nw))
        assert sum(dig[w] << (4 * w) for w in range(nw)) == k, hex(k)


@pytest.mark.parametrize('group', [1, 2])
def test_joint_ladder_related_bases(lib, group):
    g = ec.kg(3 - group)
    rng = random.Random(24 + group)
    G, H = g.gen, g.message_generator()
    nG = g.E.neg(G)
    P, Q = g.mul(G, rng.randrange(1, R)), g.mul(G, rng.randrange(1, R))
    k, k2 = rng.randrange(1, R), rng.randrange(1, R)
    z = 0xd201000000010000
    sets = [
        [(P, k), (G, k2)], [(P, k), (H, k2), (Q, rng.randrange(1, R))],                     # general position
        [(G, k), (G, k)], [(G, k), (G, -k % R)], [(nG, k), (G, k)], [(nG, k), (G, -k % R)],        # P + P, P - P at every digit
        [(G, 1), (G, 1)], [(G, 1), (G, R - 1)], [(G, R - 1), (G, R - 1)], [(P, 1), (Q, 1)],
        [(P, k), (H, k2), (H, -k2 % R)], [(P, k), (H, k2), (H, k2)], [(H, k), (H, -k % R), (P, 1)], [(H, k), (H, k), (H, k)],
        [(H, k), (H, k), (H, -2 * k % R)], [(P, 0), (Q, 0)], [(P, 0), (Q, k)], [(P, z), (Q, z * z)], [(P, z ** 3 % R), (P, R - z), (G, 2 ** 254)],
        [(P, k), (g.mul(P, 2), k)], [(P, 2), (g.mul(P, 2), R - 1)],
        [(P, int('8' * 63, 16) % R), (Q, int('7' * 63, 16)), (G, (2 ** 255 - 1) % R)], [(P, 8), (P, R - 8)], [(P, 9), (g.mul(P, 3), R - 3)],
        [(P, 5), (g.mul(P, 5), 1)], [(P, 8), (g.mul(P, 8), R - 1), (Q, 16)],            # a table entry meets the accumulator
    ]
    out = ctypes.create_string_buffer(96)
    for terms in sets:
        pts = b''.join(g.raw(p, rng) for p, _ in terms)
        ks = (ctypes.c_uint32 * (8 * len(terms)))(*[(s >> (32 * j)) & 0xffffffff for _, s in terms for j in range(8)])
        lib.hs_elgamal_ladder(group, len(terms), pts, ks, out)
        want = None
        for p, s in terms:
            want = g.add(want, g.mul(p, s))
        assert out.raw[:g.K] == g.to_bytes(want), [(p == G, hex(s)) for p, s in terms]
