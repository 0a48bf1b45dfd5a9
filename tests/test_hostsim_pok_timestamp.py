"""HashToScalar and the fixed-shape challenge hash (agora-blsful_amd/csrc/hkdf.cuh) on the host, bound tracker on, against hmac /
hashlib and Python integers (tests/pok_timestamp_cases.py): the general form at every block and padding edge and every salt rule,
the 48-byte reduction at its edges, the two register paths of compute_y against the general form and the oracle's compressed
encoding, the constant key-block states against the salt -- and the same source once more as a program of its own under
AddressSanitizer and UBSan."""
import ctypes
import hashlib
import os
import random
import subprocess
import tempfile

import pytest

import pok_timestamp_cases as pc
import util
from util import c

R = c.R
SRC = os.path.join(util.ROOT, 'tests', 'hostsim_pok', 'pok_hostsim.cpp')


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='pok_hostsim_'), 'libpok_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_challenge_bytes.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    lb.hs_challenge_point.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p]
    lb.hs_hkdf_scalar.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    lb.hs_timeout_status.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64]
    return lb


def hkdf(lib, msg, salt):
    out = ctypes.create_string_buffer(32)
    lib.hs_hkdf_scalar(msg, len(msg), salt, len(salt), out)
    return int.from_bytes(out.raw, 'little')


def test_general_form_every_length_and_salt(lib):
    rng = random.Random(1)
    for sl in (0, 1, 36, 63, 64, 65, 130):
        salt = pc.POK_SALT if sl == 36 else rng.randbytes(sl)
        for n in range(201):
            msg = rng.randbytes(n)
            assert hkdf(lib, msg, salt) == pc.hash_to_scalar(msg, salt), (sl, n)
    seed = hashlib.sha256(b'x').digest()
    assert hkdf(lib, seed, pc.KEYGEN_SALT) == util.ref.keygen_from_hash(seed)


def test_reduction(lib):
    rng = random.Random(2)
    out = ctypes.create_string_buffer(32)
    for v in [0, 1, R - 1, R, R + 1, 3 * R, 2 ** 384 - 1, 2 ** 256, 2 ** 256 - 1, 2 ** 383] + [rng.getrandbits(384) for _ in range(300)]:
        lib.hs_okm_to_scalar(v.to_bytes(48, 'big'), out)
        assert int.from_bytes(out.raw, 'little') == v % R, hex(v)
    for v in (R, 3 * R):                       # zero is returned, not looped on
        lib.hs_okm_to_scalar(v.to_bytes(48, 'big'), out)
        assert out.raw == bytes(32)


TS = (0, 1, 2 ** 32, 2 ** 64 - 1)


@pytest.mark.parametrize('sg', (1, 2))
def test_fixed_shapes_against_the_general_form(lib, sg):
    """200 random points, the identity and x coordinates with a zero top word, through the lane's path (affine conversion from a
    fresh projective scaling, words, nine compressions) and through the byte entry, against the general form in Python"""
    C = pc.IMPLS[sg]
    E, gen, raw = (c.E1, c.G1_GEN, util.g1_raw) if sg == 1 else (c.E2, c.G2_GEN, util.g2_raw)
    rng = random.Random(10 + sg)
    out, comp = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    # a chain of additions is cheap for the oracle: 200 distinct points
    step = E.mul(gen, rng.randrange(1, R))
    pts, p = [None], E.mul(gen, rng.randrange(1, R))
    for _ in range(200):
        pts.append(p)
        p = E.add(p, step)
    for i, u in enumerate(pts):
        t = TS[i % 4] if i < 8 else rng.getrandbits(64)
        want = pc.compute_y(C, u, t)
        lib.hs_challenge_point(sg, raw(u, rng), t, out, comp)
        assert comp.raw[:48 * sg] == C.sig_to_bytes(u), i
        assert int.from_bytes(out.raw, 'little') == want, i
        lib.hs_challenge_bytes(sg, C.sig_to_bytes(u), t, out)
        assert int.from_bytes(out.raw, 'little') == want, i
    # the hash does not care whether the bytes are a point: x coordinates whose top word (after the flag bits) is zero, every t
    for k in range(8):
        b = bytearray(rng.randbytes(48 * sg))
        b[0], b[1], b[2], b[3] = (0x80, 0xa0)[k & 1], 0, 0, 0
        for t in TS:
            lib.hs_challenge_bytes(sg, bytes(b), t, out)
            assert int.from_bytes(out.raw, 'little') == pc.hash_to_scalar(bytes(b) + t.to_bytes(8, 'little'), pc.POK_SALT), (k, t)


def test_midstates_are_the_salts(lib):
    out = (ctypes.c_uint32 * 32)()
    lib.hs_midstates(out)
    assert list(out[:16]) == list(out[16:]) and list(out[:8]) != list(out[8:16])


def test_timeout_rule(lib):
    for t, now, timeout in ((5, 4, None), (pc.NOW - pc.TIMEOUT, pc.NOW, pc.TIMEOUT), (pc.NOW - pc.TIMEOUT - 1, pc.NOW, pc.TIMEOUT),
                            (pc.NOW + 1, pc.NOW, pc.TIMEOUT), (pc.NOW, pc.NOW, 0), (0, 2 ** 64 - 1, 2 ** 63 - 1), (2 ** 64 - 1, 0, 0),
                            (0, 2 ** 64 - 1, None), (0, 2 ** 63, 2 ** 63 - 1)):
        want = pc.timeout_status(t, now, timeout)
        assert lib.hs_timeout_status(t, now, -1 if timeout is None else timeout) == (0 if want is None else want), (t, now, timeout)


def test_standalone_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix='pok_hostsim_san_'), 'pok_hostsim')
    subprocess.check_call(['g++', '-O1', '-g', '-DBLS_TRACK_BOUNDS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-DPOK_HOSTSIM_MAIN', '-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert p.stdout.strip().endswith(' 0 bad')
