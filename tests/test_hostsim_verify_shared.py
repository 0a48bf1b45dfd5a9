"""The per-item functions of the shared-message verify calls (csrc/verify_shared.cuh) on the host with the bound tracker on: the group
lookup against a linear scan over offset arrays with runs of empty groups; the byte gather of the MessageAugmentation path; the
per-group line-table routine, which must reproduce the generated tables G2NEG_LINES_N / G2NEGC_LINES_N row for row when it is given
-g2 and -[c] g2, canonical words included; a Miller loop fed from a BUILT table against the general two-pair loop, for the oracle's
hash points, on valid and tampered pairs; the flag for the identity and for h = 0; and Bls12381G1Impl's record against
prepare_hashed_item's.  The same driver runs once more as a stand-alone program under the address and undefined-behaviour
sanitizers (a host build, nothing preloaded)."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util
from util import c, ref

SRC = os.path.join(util.ROOT, 'tests', 'hostsim_verify_shared', 'verify_shared_hostsim.cpp')
TABLE_WORDS = 68 * 4 * 14


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='verify_shared_hostsim_'), 'libverify_shared_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_group_of.restype = ctypes.c_uint64
    lb.hs_group_of.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    lb.hs_expand_src.restype = ctypes.c_uint64
    lb.hs_expand_src.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    return lb


def u64s(v):
    return (ctypes.c_uint64 * len(v))(*v)


def offsets(sizes):
    o = [0]
    for s in sizes:
        o.append(o[-1] + s)
    return o


def test_group_lookup_against_a_linear_scan(lib):
    rng = random.Random(1)
    shapes = [[3], [0, 0, 0, 2], [2, 0, 0, 0], [1, 0, 0, 0, 1], [0, 1, 0], [1] * 9, [0, 0, 5, 0, 0, 0, 7, 0], [1, 0, 31, 33, 0, 65]]
    shapes += [[rng.choice([0, 0, 0, 1, 2, 9]) for _ in range(rng.randrange(1, 70))] for _ in range(60)]
    seen = 0
    for sizes in shapes:
        offs = offsets(sizes)
        arr = u64s(offs)
        for i in range(offs[-1]):
            want = max(g for g in range(len(sizes)) if offs[g] <= i)               # the last group that starts at or before i ...
            assert offs[want] <= i < offs[want + 1]                                 # ... is the one that owns i
            assert lib.hs_group_of(arr, len(sizes), i) == want, (sizes, i)
            seen += 1
    assert seen > 2000


def test_expand_src(lib):
    """the per-item message buffer of the MessageAugmentation path: item j's bytes are its group's message"""
    rng = random.Random(2)
    for _ in range(40):
        ng = rng.randrange(1, 9)
        sizes = [rng.choice([0, 1, 2, 5]) for _ in range(ng)]
        lens = [rng.choice([0, 0, 1, 3, 8]) for _ in range(ng)]
        ioffs, moffs = offsets(sizes), offsets(lens)
        n = ioffs[-1]
        if n == 0:
            continue
        item_group = [g for g in range(ng) for _ in range(sizes[g])]
        xoffs = offsets([lens[g] for g in item_group])
        want = [moffs[g] + k for g in item_group for k in range(lens[g])]
        got = [lib.hs_expand_src(u64s(xoffs), n, u64s(ioffs), ng, u64s(moffs), b) for b in range(xoffs[-1])]
        assert got == want, (sizes, lens)


@pytest.mark.parametrize('which', [1, 2], ids=['-g2', '-[c]g2'])
def test_table_of_a_constant_is_the_generated_table(lib, which):
    assert lib.hs_table_of_constant(which) == 0


def test_flag(lib):
    table = (ctypes.c_uint32 * TABLE_WORDS)()
    assert lib.hs_build_table(bytes(192), table) == 0                                        # the identity
    h = c.hash_to_g2(b'flag', ref.G2Impl.DST[ref.BASIC])
    assert lib.hs_build_table(util.g2_aff_raw(h), table) == 1
    assert lib.hs_build_table(util.fp2_raw(h[0]) + util.fp2_raw((0, 0)), table) == 0         # y = 0: the first tangent has h = 2 Y Z = 0


def test_table_fed_loop_agrees_with_the_general_loop(lib):
    """random H(m), keys and signatures: the table form and the general form give the oracle's verdict"""
    C = ref.G2Impl
    rng = random.Random(3)
    out = (ctypes.c_int * 2)()
    for t in range(3):
        m = b'shared message %d' % t
        h = c.hash_to_g2(m, C.DST[ref.BASIC])
        for j in range(2):
            k = rng.randrange(1, c.R)
            pk = C.pk_curve.mul(C.pk_gen, k)
            for signer, want in ((k, 0), (k + 1, 1)):
                sig = C.sig_curve.mul(h, signer % c.R)
                try:
                    ref.verify(C, ref.BASIC, pk, sig, m)
                    oracle = 0
                except ref.BlsError:
                    oracle = 1
                assert oracle == want
                lib.hs_verdicts(util.g1_raw(pk, rng), util.g2_raw(sig, rng), util.g2_aff_raw(h), out)
                assert list(out) == [want, want], (t, j, signer == k)
    lib.hs_verdicts(util.g1_raw(pk, rng), util.g2_raw(None), util.g2_aff_raw(h), out)
    assert list(out) == [2, 2]
    lib.hs_verdicts(util.g1_raw(None, rng), util.g2_raw(None), util.g2_aff_raw(h), out)
    assert list(out) == [2, 2]                                                              # the signature wins
    lib.hs_verdicts(util.g1_raw(None, rng), util.g2_raw(sig, rng), util.g2_aff_raw(h), out)
    assert list(out) == [3, 3]


def test_g1impl_record_is_prepare_hashed_items(lib):
    C = ref.G1Impl
    rng = random.Random(4)
    h = c.hash_to_g1(b'm', C.DST[ref.POP])
    k = rng.randrange(1, c.R)
    pk, sig = C.pk_curve.mul(C.pk_gen, k), C.sig_curve.mul(h, k)
    assert lib.hs_prepare_g1impl(util.g2_raw(pk, rng), util.g1_raw(sig, rng), util.g1_aff_raw(h)) == 0
    assert lib.hs_prepare_g1impl(util.g2_raw(pk, rng), util.g1_raw(None, rng), util.g1_aff_raw(h)) == 2
    assert lib.hs_prepare_g1impl(util.g2_raw(None), util.g1_raw(None, rng), util.g1_aff_raw(h)) == 2
    assert lib.hs_prepare_g1impl(util.g2_raw(None), util.g1_raw(sig, rng), util.g1_aff_raw(h)) == 3


def test_standalone_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix='verify_shared_hostsim_san_'), 'verify_shared_hostsim')
    subprocess.check_call(['g++', '-O1', '-g', '-DBLS_TRACK_BOUNDS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-DVERIFY_SHARED_HOSTSIM_MAIN', '-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert p.stdout.strip().endswith(' 0 bad')
