"""The pairing values of the lane-split kernels on the host, as far as the host build can run them (tests/hostsim_value_split, with the
bound tracker of fp.cuh on; a tracked-bound violation aborts the process):
  * the value ending and the byte export of k_finalexp2s_value -- final_exp_parts on the lane-split Fp2, the kernel's ending t f^2 f,
    and every tower slot placed through gt_tower_wpow / gt_part_offset / coop_gt_put -- against tests/timecrypt_ref.py
    gt_bytes(c.final_exponentiation(f)) on the Miller values of pairs of tests/timecrypt_cases.py;
  * the per-entry loop of k_millerf_rows1 against the rows and the walk restated in tests/miller_cases.py: conj(f) coefficient for
    coefficient, and its value against the oracle's pairing.
The packed LDS accumulator and the functions that stream through it (fx_load / fx_store / fx_mul, f12_sh_mul_line3) exist on the
device only; tests/test_gpu_value_split.py runs them."""
import ctypes
import os
import subprocess

import pytest

import field_cases as fc
import miller_cases as mc
import timecrypt_cases as tc
import timecrypt_ref as tr
import util
from util import c

PAIRS = [0, 1, 2, 4, 7, 11]           # of tc.SCALARS: the generators, small multiples, the negated generators, two random pairs


@pytest.fixture(scope='module')
def lib():
    here = os.path.join(util.ROOT, 'tests', 'hostsim_value_split')
    src, so = os.path.join(here, 'value_split_hostsim.cpp'), os.path.join(here, 'libvalue_split_hostsim.so')
    csrc = os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc')
    deps = [src, os.path.join(util.ROOT, 'tests', 'hostsim_coop', 'coop_hostsim.cpp')] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.cuh', '.h'))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(['g++', '-O2', '-fwrapv', '-pthread', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])      # the flags of tests/test_hostsim_timecrypt.py
    return ctypes.CDLL(so)


def tower_limbs(f):
    """the twelve limb vectors of an oracle Fp12 (w-power order) in tower order: c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5)"""
    return [x for k in (0, 2, 4, 1, 3, 5) for v in f[k] for x in util.limbs_of_elem(v)]


@pytest.mark.parametrize('k', PAIRS)
def test_value_ending_and_export(lib, k):
    a, b = tc.SCALARS[k]
    f = c.miller_loop([(tc.g1_mul(a), tc.g2_mul(b))])
    for fin in (f, c.f12_conj(f)):
        flat = tower_limbs(fin)
        out = (ctypes.c_uint8 * tr.GT_BYTES)()
        assert lib.hs_finalexp_value((ctypes.c_int32 * len(flat))(*flat), out) == 0
        assert bytes(out) == tr.gt_bytes(c.final_exponentiation(fin))
    assert tr.gt_bytes(c.final_exponentiation(f)) == tc.expected(a, b)


def test_value_of_an_element_of_fp6_is_one(lib):
    """the easy part maps Fp6* to 1: the compressed chain declines and the plain chain answers; the bytes are Gt one's"""
    v = ((3, 5), (0, 0), (7, 11), (0, 0), (c.P - 1, 2), (0, 0))
    flat = tower_limbs(v)
    out = (ctypes.c_uint8 * tr.GT_BYTES)()
    assert lib.hs_finalexp_value((ctypes.c_int32 * len(flat))(*flat), out) == 0
    assert bytes(out) == tr.GT_ONE == bytes(47) + b'\x01' + bytes(528)


def rows_of(Q):
    """(the 68 normalised rows as Fp2 pairs, their words in the *_LINES_N layout: canonical Montgomery limbs)"""
    rows = [mc.norm_row(l) for l in mc.walk(Q)[0]]
    words = [x for n0, cc in rows for v in (n0[0], n0[1], cc[0], cc[1]) for x in util.limbs_of(v % c.P * util.R392 % c.P)]
    assert all(0 <= x <= util.LIMB_MASK for x in words)
    return rows, words


@pytest.mark.parametrize('k', PAIRS)
def test_rows1_loop(lib, k):
    a, b = tc.SCALARS[k]
    P, Q = tc.g1_mul(a), tc.g2_mul(b)
    rows, words = rows_of(Q)
    f = c.F12_ONE
    for e, (n0, cc) in enumerate(rows):
        if e > 0 and e not in mc.ADD_ENTRIES:
            f = c.f12_mul(f, f)
        f = c.f12_mul(f, fc.line3_f12(*mc.line3_row(n0, cc, P[0], P[1])))
    xy = [x for v in P for x in util.limbs_of_elem(v)]
    out_f, out_v = (ctypes.c_uint8 * tr.GT_BYTES)(), (ctypes.c_uint8 * tr.GT_BYTES)()
    assert lib.hs_rows1((ctypes.c_int32 * len(xy))(*xy), (ctypes.c_uint32 * len(words))(*words), out_f, out_v) == 0
    assert bytes(out_f) == tr.gt_bytes(c.f12_conj(f))
    assert bytes(out_v) == tc.expected(a, b)
