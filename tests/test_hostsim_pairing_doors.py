"""The per-item bodies of k_prepare_proof, k_prepare_hashed and k_pairs2_to_affine (csrc/verify.cuh) on the host with the bound
tracker on, then the host Miller loop -- over G2NEG_LINES on the one-lane tower and over the merged G2NEG_LINES_N on the lane-split
tower where the door passes fixed_g2 = 1 -- and the final verdict: every kind of tests/pairing_door_cases.py, both orientations, must
get the case list's result.  This extends DESIGN section 4's one-pass proof of the limb bounds to hash -> jac_mul_scalar -> jac_add
with a caller's point -> g1g2_to_aff, to fp_inv3 on three caller-supplied Z values and to the two-pair conversion, and it is where
the H = identity and U = y H(m) kinds can be debugged without a GPU."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import pairing_door_cases as d
import util


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_pairing_doors', 'pairing_doors_hostsim.cpp')
    so = os.path.join(tempfile.mkdtemp(prefix='pairing_doors_hostsim_'), 'libpairing_doors_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])
    return ctypes.CDLL(so)


def run_kinds(door, sg, scheme, call):
    """every (kind, base item) of the pool through `call(rendered RAW_PROJ columns)`: the case list's result"""
    rng = random.Random(17 * sg + scheme)
    bad = []
    for (kind, j), (item, want) in d.cases(door, sg, scheme).items():
        got = call(d.render(door, sg, item, d.RAW_PROJ, rng))
        if door in d.BOOL_DOORS:
            got = {0: True, 1: False}.get(got, got)
        if got != want or type(got) is not type(want):
            bad.append((kind, j, got, want))
    assert not bad, bad


@pytest.mark.parametrize('sg', [1, 2])
def test_hashed(lib, sg):
    run_kinds('hashed', sg, 0, lambda r: lib.hs_door_hashed(sg, r[0], r[1], r[2]))


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('scheme', d.SCHEMES)
def test_sig_proof(lib, sg, scheme):
    dst = d.IMPLS[sg].DST[scheme]
    run_kinds('sig_proof', sg, scheme,
              lambda r: lib.hs_door_proof(sg, r[0], r[1], r[2], int(r[3]).to_bytes(32, 'little'), r[4], len(r[4]), dst, len(dst)))


def test_pairing2(lib):
    run_kinds('pairing2', 0, 0, lambda r: lib.hs_door_pairs2(r[0], r[1], r[2], r[3]))
