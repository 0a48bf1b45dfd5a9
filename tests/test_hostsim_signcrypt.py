"""The signcryption device functions (csrc/keccak.cuh, csrc/signcrypt.cuh) on the host: the SHAKE128 keystream against
hashlib.shake_128 for 48- and 96-byte inputs and every output length 0 - 512 (plus 1,000 and 4,097), at every alignment of the
frame (the 8-byte word path and the byte path), with guard bytes around the output; and the frame parser against the Python
model of tests/signcrypt_cases.py on the crafted frames and on 2,000 random ones."""
import ctypes
import hashlib
import os
import random
import subprocess
import tempfile

import pytest

import signcrypt_cases as sc
import util


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_signcrypt', 'signcrypt_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='signcrypt_hostsim_')
    so = os.path.join(d, 'libsigncrypt_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    lb.hs_keystream_xor.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int]
    lb.hs_keystream_xor.restype = None
    lb.hs_parse_frame.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    return lb


GUARD = 16


def xor_at(lib, g, v, out_mis, v_mis):
    """The keystream xor with the output at address = out_mis mod 8 and v at v_mis mod 8; checks the guard bytes."""
    n = len(v)
    size = n + 2 * GUARD + 16
    obuf = ctypes.create_string_buffer(b'\xa5' * size, size)
    vbuf = ctypes.create_string_buffer(n + 32)
    oa = ctypes.addressof(obuf) + GUARD
    oa += (out_mis - oa) % 8
    va = ctypes.addressof(vbuf)
    va += (v_mis - va) % 8
    ctypes.memmove(va, v, n)
    lib.hs_keystream_xor(oa, va, n, g, len(g))
    lo = oa - ctypes.addressof(obuf)
    raw = obuf.raw
    assert raw[:lo] == b'\xa5' * lo and raw[lo + n:] == b'\xa5' * (len(raw) - lo - n), 'wrote outside the frame'
    return raw[lo:lo + n]


def test_keccak_permutation_of_zero(lib):
    s = (ctypes.c_uint64 * 25)()
    lib.hs_keccak_f1600(s)
    assert s[0] == 0xF1258F7940E1DDE7        # the first lane of Keccak-f[1600](0)


@pytest.mark.parametrize('glen', [48, 96])
def test_shake128_every_length(lib, glen):
    rng = random.Random(glen)
    g = bytes(rng.randrange(256) for _ in range(glen))
    ks = hashlib.shake_128(g).digest(4097)
    for n in list(range(513)) + [1000, 4097]:
        v = bytes(rng.randrange(256) for _ in range(n))
        want = bytes(a ^ b for a, b in zip(ks, v))
        mis = n % 8
        assert xor_at(lib, g, v, mis, mis) == want, (n, 'words')
        assert xor_at(lib, g, v, mis, (mis + 3) % 8) == want, (n, 'bytes')
    zero = bytes(600)
    for mis in range(8):                                  # every alignment of the word path, around one and two block boundaries
        for n in (0, 1, 7, 8, 9, 160, 167, 168, 169, 176, 335, 336, 337, 344, 600):
            assert xor_at(lib, g, zero[:n], mis, mis) == ks[:n], (mis, n)
    assert xor_at(lib, bytes([0xc0]) + bytes(glen - 1), zero[:64], 0, 0) == hashlib.shake_128(bytes([0xc0]) + bytes(glen - 1)).digest(64)


def parse(lib, frame):
    off, ln = ctypes.c_uint64(99), ctypes.c_uint64(99)
    ok = lib.hs_parse_frame(frame, len(frame), ctypes.byref(off), ctypes.byref(ln))
    return (off.value, ln.value) if ok else None


def test_parser_matches_the_model(lib):
    for name, frame in sc.crafted_frames():
        assert parse(lib, frame) == sc.parse_frame(frame), name
    rng = random.Random(7)
    hits = 0
    for _ in range(2000):
        n = rng.choice([0, 1, 2, 5, 18, 19, 20, 32, 33, 200, 300])
        kind = rng.randrange(4)
        if kind == 0:
            frame = bytes(rng.randrange(256) for _ in range(n))
        elif kind == 1:                                  # a well-formed prefix with a length near what remains
            body = rng.randrange(0, n + 3)
            frame = (sc.varint(body) + bytes(rng.randrange(256) for _ in range(n)))[:max(n, 1)]
        elif kind == 2:                                  # long runs of continuation bytes
            k = rng.randrange(0, 22)
            frame = (bytes(0x80 | rng.randrange(128) for _ in range(k)) + bytes([rng.randrange(128)]) + bytes(n))[:n + k]
        else:
            frame = (sc.varint(rng.randrange(2 ** 63)) + bytes(n))[:n]
        got = parse(lib, frame)
        assert got == sc.parse_frame(frame), frame.hex()
        hits += got is not None
    assert 200 < hits < 1800
