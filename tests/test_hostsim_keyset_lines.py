"""The host side of the per-key line tables of the registered key sets (BLSGPU_KEYSET_LINES; csrc/keyset.cuh, csrc/tower.cuh
lines_merge_yy, csrc/pairing.cuh miller_loop_tables_merged) with the bound tracker on, on the host emulation of the lane-split tower:
lines_merge_yy against lines_merge coefficient by coefficient, random slots and the edges 0, 1, p - 1 in every slot; the rows of
-[c] g2 built through the key-set build path against the generated table G2NEGC_LINES_N, canonical words included; a Miller loop fed
from TWO tables (a key's built rows at the uncleared message point, G2NEGC_LINES_N at the signature) against the general two-pair
loop, on the oracle's valid and tampered tuples; the flag for entries without usable rows; and the size rule.  A violated bound
aborts the process, so a test that returns has seen the tracker silent.  The same driver runs once more as a stand-alone program
under the address and undefined-behaviour sanitizers (a host build, nothing preloaded)."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util
from util import c, ref

SRC = os.path.join(util.ROOT, 'tests', 'hostsim_keyset_lines', 'keyset_lines_hostsim.cpp')
TABLE_WORDS = 68 * 4 * 14
KEY_BYTES = TABLE_WORDS * 4


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='keyset_lines_hostsim_'), 'libkeyset_lines_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_lines_fit.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    return lb


def test_merge_yy_is_merge_with_both_w3_coefficients_in_fp(lib):
    """slots: a0, a2, b0, b2 (two Fp each), ya, yb; both tower instantiations; 0 = every coefficient equal after canonical reduction"""
    rng = random.Random(1)
    P = c.P

    def call(vals):
        return lib.hs_merge_yy_differs(b''.join(util.fp_raw(v) for v in vals))
    for _ in range(40):
        assert call([rng.randrange(P) for _ in range(10)]) == 0
    for edge in (0, 1, P - 1):
        assert call([edge] * 10) == 0, edge
        for slot in range(10):
            vals = [rng.randrange(P) for _ in range(10)]
            vals[slot] = edge
            assert call(vals) == 0, (edge, slot)
        for slots in ((8, 9), (0, 1, 4, 5), (2, 3, 6, 7)):                 # both y, both constant terms, both w^2 terms
            vals = [rng.randrange(P) for _ in range(10)]
            for s in slots:
                vals[s] = edge
            assert call(vals) == 0, (edge, slots)


def negc():
    return c.E2.neg(c.E2.mul(c.G2_GEN, pow(c.H_EFF_G1, -1, c.R)))


def test_built_rows_of_the_constant_are_the_generated_table(lib):
    assert lib.hs_rows_of_negc(util.g2_aff_raw(negc())) == 0


def test_flag(lib):
    table = (ctypes.c_uint32 * TABLE_WORDS)()
    assert lib.hs_build_rows(bytes(192), table) == 1                                         # the identity / an invalid entry
    pk = c.E2.mul(c.G2_GEN, 12345)
    assert lib.hs_build_rows(util.g2_aff_raw(pk), table) == 0
    assert lib.hs_build_rows(util.fp2_raw(pk[0]) + util.fp2_raw((0, 0)), table) == 2         # finite, y = 0: the first tangent has h = 2 Y Z = 0


def uncleared_hash(msg, dst):
    """the message point the Bls12381G1Impl kernels pair with: the sum of the two mapped points, before the cofactor is cleared"""
    u0, u1 = c.hash_to_field(msg, dst, 2, 1)
    q = c.E1.add(c.map_to_curve_g1(u0), c.map_to_curve_g1(u1))
    assert c.E1.mul(q, c.H_EFF_G1) == c.hash_to_g1(msg, dst)
    return q


def test_two_table_loop_agrees_with_the_general_loop(lib):
    """three keys, two messages each, signed by the oracle and tampered: the two-table form and the general form give the oracle's
    verdict on prepare_shared_item's record (the uncleared hash; the second pair is (sig, -[c] g2))"""
    C = ref.G1Impl
    rng = random.Random(3)
    out = (ctypes.c_int * 2)()
    for t in range(3):
        sk = rng.randrange(1, c.R)
        pk = C.pk_curve.mul(C.pk_gen, sk)
        rec = util.g2_aff_raw(pk)
        for j in range(2):
            m = b'keyed message %d %d' % (t, j)
            h = uncleared_hash(m, C.DST[ref.BASIC])
            for signer, want in ((sk, 0), (sk + 1, 1)):
                sig = C.sig_curve.mul(c.hash_to_g1(m, C.DST[ref.BASIC]), signer % c.R)
                try:
                    ref.verify(C, ref.BASIC, pk, sig, m)
                    oracle = 0
                except ref.BlsError:
                    oracle = 1
                assert oracle == want
                lib.hs_verdicts(util.g2_raw(pk, rng), rec, util.g1_raw(sig, rng), util.g1_aff_raw(h), out)
                assert list(out) == [want, want], (t, j, signer == sk)
                if signer == sk:
                    good = sig
            other = uncleared_hash(m + b'!', C.DST[ref.BASIC])                               # a wrong message
            lib.hs_verdicts(util.g2_raw(pk, rng), rec, util.g1_raw(good, rng), util.g1_aff_raw(other), out)
            assert list(out) == [1, 1]
    lib.hs_verdicts(util.g2_raw(pk, rng), rec, util.g1_raw(None, rng), util.g1_aff_raw(h), out)
    assert list(out) == [2, 2]
    lib.hs_verdicts(util.g2_raw(None), rec, util.g1_raw(None, rng), util.g1_aff_raw(h), out)
    assert list(out) == [2, 2]                                                               # the signature wins
    lib.hs_verdicts(util.g2_raw(None), rec, util.g1_raw(sig, rng), util.g1_aff_raw(h), out)
    assert list(out) == [3, 3]


def test_size_rule(lib):
    """the 32-bit byte offset of the line kernel (15,232 bytes per key: 281,970 keys stay below 2^32) and the MiB cap, which the
    fixed-base tables share"""
    assert 281970 * KEY_BYTES < 2 ** 32 <= 281971 * KEY_BYTES
    assert lib.hs_lines_fit(281970, 0, 4096) == 1
    assert lib.hs_lines_fit(281971, 0, 4096) == 0 and lib.hs_lines_fit(281971, 0, 1 << 20) == 0
    assert lib.hs_lines_fit(0, 0, 4096) == 0
    assert lib.hs_lines_fit(320, 0, 5) == 1 and lib.hs_lines_fit(320, 0, 1) == 0             # 4.65 MiB of rows
    assert lib.hs_lines_fit(320, 1 << 20, 5) == 0                                            # ... with 1 MiB of fixed-base tables
    assert lib.hs_lines_fit(68, 0, 1) == 1 and lib.hs_lines_fit(69, 0, 1) == 0               # 1 MiB = 68.8 keys' rows


def test_standalone_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix='keyset_lines_hostsim_san_'), 'keyset_lines_hostsim')
    subprocess.check_call(['g++', '-O1', '-g', '-DBLS_TRACK_BOUNDS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-DKEYSET_LINES_HOSTSIM_MAIN', '-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert p.stdout.strip().endswith(' 0 bad')
