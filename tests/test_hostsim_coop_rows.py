"""The Miller loop of one TABLED and one WALKED pair of the wave-cooperative engine (csrc/coop_rows.cuh coop_miller2_rows, what
k_pairing_coop_rows runs for a Bls12381G2Impl verification under a registered message) on the host: tests/hostsim_coop_rows compiles
the round functions the device compiles, one thread per lane pair, with the bound tracker on and strict -- a read of an LDS slot
nobody wrote aborts, and every element's bounds are carried through its slot.  Pair 0's rows are built from the case's Q0 by
group_lines_build; the record's own Q0 is not read.  On every two-general-pair case of the list the easy-part value must equal the
oracle's exactly (the Fp2 factors of the normalisation die there), the verdict must be the oracle's, and the tracker stays silent,
which proves the placement of the reductions in the new rounds."""
import ctypes
import os
import subprocess

import pytest

import field_cases as fc
import util

HERE = os.path.join(util.ROOT, 'tests', 'hostsim_coop_rows')


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(HERE, 'coop_rows_hostsim.cpp')
    so = os.path.join(HERE, 'libcoop_rows_hostsim.so')
    csrc = os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc')
    deps = [src, os.path.join(util.ROOT, 'tests', 'hostsim_coop', 'coop_hostsim.cpp')] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.cuh', '.h'))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(['g++', '-O2', '-fwrapv', '-pthread', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])
    return ctypes.CDLL(so)


GENERAL = [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == 0]


def test_the_case_list_is_what_the_tests_below_rely_on():
    assert len(GENERAL) >= 14 and {fc.pairing_expected(cs)[2] for cs in GENERAL} == {fc.BLS_OK, fc.BLS_INVALID}
    names = ' | '.join(cs['name'] for cs in GENERAL)
    assert 'outside the subgroups' in names and 'largest canonical' in names and 'negative representative' in names


@pytest.mark.parametrize('cs', GENERAL, ids=[cs['name'] for cs in GENERAL])
def test_rows_miller_loop_and_final_exponentiation_on_the_host(lib, cs):
    """coop_miller2_rows, then coop_final_easy -- the exact Fp12 value against the oracle -- and coop_final_verdict"""
    (qx, qy) = cs['pairs'][0][1]
    rec = util.fp2_raw(qx) + util.fp2_raw(qy)
    assert len(rec) == 192
    vecs = [list(v) for v in cs['vecs']]
    for k in range(2, 6):                    # pair 0's Q in the record: not read, so garbage must not matter
        vecs[k] = [0x0badbad] * len(vecs[k])
    flat = (ctypes.c_int32 * 168)(*[x for v in vecs for x in v])
    out = (ctypes.c_int32 * 168)()
    assert lib.hs_coop_pairing_rows(0, flat, rec, out) == 0
    o = list(out)
    fc.check_easy(cs, [o[14 * k:14 * (k + 1)] for k in range(12)])
    assert lib.hs_coop_pairing_rows(1, flat, rec, out) == fc.pairing_expected(cs)[2], cs['name']
