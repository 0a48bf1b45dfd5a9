"""The pairing-value functions of csrc/timecrypt.cuh on the host: tests/hostsim_timecrypt compiles coop_miller1, coop_final_value and
coop_gt_bytes -- the source text the device compiles -- with the bound tracker of fp.cuh on, a wave as 32 threads (the model of
tests/hostsim_coop).  Their 576 bytes must be those of tests/timecrypt_ref.py on the pairs of tests/timecrypt_cases.py; a tracked-bound
violation aborts the process."""
import ctypes
import os
import random
import subprocess

import pytest

import timecrypt_cases as tc
import timecrypt_ref as tr
import util
from util import c


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_timecrypt', 'timecrypt_hostsim.cpp')
    so = os.path.join(util.ROOT, 'tests', 'hostsim_timecrypt', 'libtimecrypt_hostsim.so')
    csrc = os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc')
    deps = [src, os.path.join(util.ROOT, 'tests', 'hostsim_coop', 'coop_hostsim.cpp')] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.cuh', '.h'))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the flags of util.build_hostsim_coop: -fwrapv because the engine multiplies job slots whose values nobody uses
        subprocess.check_call(['g++', '-O2', '-fwrapv', '-pthread', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])
    return ctypes.CDLL(so)


def run_pair(lib, a, b):
    flat = [x for v in tc.pair_limbs(a, b) for x in v]
    out = (ctypes.c_uint8 * tr.GT_BYTES)()
    assert lib.hs_pairing_value((ctypes.c_int32 * len(flat))(*flat), out) == 0
    return bytes(out)


@pytest.mark.parametrize('k', range(len(tc.SCALARS)))
def test_pairing_value_on_the_host(lib, k):
    """coop_miller1 + coop_final_value + coop_gt_bytes against the oracle's value, byte for byte, with no bound violation"""
    a, b = tc.SCALARS[k]
    assert run_pair(lib, a, b) == tc.expected(a, b)


def test_gt_bytes_of_chosen_elements(lib):
    """coop_gt_bytes alone: one, coefficients 0, 1, p - 1, random ones, from the reduced internal form"""
    rng = random.Random(9)
    elems = [c.F12_ONE, tuple((c.P - 1, c.P - 1) for _ in range(6)), tuple((k, c.P - 1 - k) for k in range(6))]
    elems += [tuple((rng.randrange(c.P), rng.randrange(c.P)) for _ in range(6)) for _ in range(4)]
    for f in elems:
        flat = [x for co in f for v in co for x in util.limbs_of_elem(v)]
        out = (ctypes.c_uint8 * tr.GT_BYTES)()
        assert lib.hs_gt_bytes((ctypes.c_int32 * len(flat))(*flat), out) == 0
        assert bytes(out) == tr.gt_bytes(f)
    assert tr.gt_bytes(c.F12_ONE) == bytes(47) + b'\x01' + bytes(528)


@pytest.mark.parametrize('sg', [1, 2])
def test_time_lock_tail_on_the_host(lib, sg):
    """timecrypt_open_frame and timecrypt_check -- the lane body of k_timecrypt_open -- on every case whose pairing is formed (scheme
    tags equal, no identity), fed the oracle's K: status, range and the opened message against tests/timecrypt_ref.py"""
    C = tr.IMPLS[sg]
    lib.hs_timecrypt_open.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p,
                                      ctypes.POINTER(ctypes.c_uint64)]
    seen = set()
    for g in tc.timelock_groups(sg):
        for it in g['items']:
            if it['scheme'] != g['scheme'] or g['sig'] is None or it['u'] is None:
                continue
            gt = tr.gt_bytes(tr.pairing_of(C, g['sig'], it['u']))
            u_raw = util.g2_raw(it['u']) if sg == 1 else util.g1_raw(it['u'])
            frame = ctypes.create_string_buffer(max(len(it['w']), 1))
            rng = (ctypes.c_uint64 * 2)()
            st = lib.hs_timecrypt_open(sg, gt, it['v'], it['w'], len(it['w']), u_raw, frame, rng)
            want_st, want_msg = it['want']
            assert st == want_st, it['name']
            if st == tc.OK:
                assert frame.raw[rng[0]:rng[0] + rng[1]] == want_msg, it['name']
                assert len(want_msg) == 0 or tr.peek(frame.raw[:len(it['w'])]) == (rng[0], rng[1]), it['name']
            else:
                assert (rng[0], rng[1]) == (0, 0), it['name']
            seen.add(st)
    assert seen == {tc.OK, tc.INVALID_SIGNATURE, tc.BAD_FRAME}
