"""The body of k_pairing_value_rows on the host: tests/hostsim_sigset compiles coop_miller1_rows (csrc/coop_row1.cuh, the Miller loop
of ONE TABLED pair that a registered signature's rows feed), coop_final_value and coop_gt_bytes -- the source text the device
compiles -- one thread per lane pair, with the bound tracker on and strict: a read of an LDS slot nobody wrote aborts, and every
element's bounds are carried through its slot.  The rows are built from the pair's Q by group_lines_build.  On every general pair of
field_cases.pairing_cases() (each of its two pairs alone) and on the dozen pairs of timecrypt_cases.SCALARS the 576 bytes must be
those of tests/timecrypt_ref.py exactly, and those of the walked path (coop_miller1) on the same pair; the tracker stays silent,
which proves the placement of the reductions in the new rounds.  A build that skips the first row's staging must abort: the harness
is strict in fact, not in name."""
import ctypes
import os
import subprocess
import sys

import pytest

import field_cases as fc
import timecrypt_cases as tc
import timecrypt_ref as tr
import util

HERE = os.path.join(util.ROOT, 'tests', 'hostsim_sigset')
FLAGS = ['g++', '-O2', '-fwrapv', '-pthread', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC']      # the flags of tests/test_hostsim_coop_rows.py


def build(name, extra=()):
    src = os.path.join(HERE, 'sigset_hostsim.cpp')
    so = os.path.join(HERE, name)
    csrc = os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc')
    deps = [src, os.path.join(util.ROOT, 'tests', 'hostsim_coop', 'coop_hostsim.cpp'),
            os.path.join(util.ROOT, 'tests', 'hostsim_coop_rows', 'coop_rows_hostsim.cpp')] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.cuh', '.h'))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(FLAGS + list(extra) + ['-o', so, src])
    return so


@pytest.fixture(scope='module')
def lib():
    return ctypes.CDLL(build('libsigset_hostsim.so'))


def pairs():
    """(name, P, Q, the six limb vectors): each pair of every general case alone (the case's own limb vectors, so that the negative
    representatives come along; equal pairs once), then the SCALARS pairs"""
    out, seen = [], set()
    for cs in fc.pairing_cases():
        if cs['fixed_g2'] != 0:
            continue
        for k in range(2):
            P, Q = cs['pairs'][k]
            vecs = [list(v) for v in cs['vecs'][6 * k:6 * k + 6]]
            key = (P, Q, tuple(tuple(v) for v in vecs))
            if key not in seen:
                seen.add(key)
                out.append(('%s, pair %d' % (cs['name'], k), P, Q, vecs))
    for a, b in tc.SCALARS:
        out.append(('(%d g1, %d g2)' % (a % 1000, b % 1000), tc.g1_mul(a), tc.g2_mul(b), tc.pair_limbs(a, b)))
    return out


PAIRS = pairs()


def test_the_pair_list_is_what_the_tests_below_rely_on():
    names = ' | '.join(p[0] for p in PAIRS)
    assert len(PAIRS) >= 12 + 14 and 'outside the subgroups' in names and 'largest canonical' in names and 'negative representative' in names
    for _, P, Q, vecs in PAIRS[:4]:            # the limb vectors are the pair's: P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1
        assert [util.elem_of(v) for v in vecs] == [P[0], P[1], Q[0][0], Q[0][1], Q[1][0], Q[1][1]]


def rec_of(Q):
    rec = util.fp2_raw(Q[0]) + util.fp2_raw(Q[1])
    assert len(rec) == 192
    return rec


@pytest.mark.parametrize('pr', PAIRS, ids=[p[0] for p in PAIRS])
def test_rows_pairing_value_on_the_host(lib, pr):
    """coop_miller1_rows + coop_final_value + coop_gt_bytes: the oracle's bytes and the walked path's, with no bound violation and no
    unstaged slot"""
    _, P, Q, vecs = pr
    flat = (ctypes.c_int32 * (6 * len(vecs[0])))(*[x for v in vecs for x in v])
    out = (ctypes.c_uint8 * tr.GT_BYTES)()
    assert lib.hs_pairing_value_rows(flat, rec_of(Q), out) == 0
    want = tr.gt_bytes(tr.pairing_value(P, Q))
    assert bytes(out) == want
    walked = (ctypes.c_uint8 * tr.GT_BYTES)()
    assert lib.hs_pairing_value_walked(flat, walked) == 0
    assert bytes(walked) == bytes(out)


def test_the_harness_aborts_on_a_slot_nobody_staged():
    """the same source with -DCOOP_ROW1_TEST_SKIP_ROW0, which leaves row 0's n0 out of its line slot: the first line round reads it
    and the strict tracker must abort the process"""
    so = build('libsigset_hostsim_skip.so', ['-DCOOP_ROW1_TEST_SKIP_ROW0'])
    a, b = tc.SCALARS[1]
    flat = [x for v in tc.pair_limbs(a, b) for x in v]
    code = ('import ctypes, sys\n'
            'lib = ctypes.CDLL(%r)\n'
            'flat = (ctypes.c_int32 * %d)(*%r)\n'
            'out = (ctypes.c_uint8 * 576)()\n'
            'print("rc", lib.hs_pairing_value_rows(flat, %r, out))\n') % (so, len(flat), flat, rec_of(tc.g2_mul(b)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == -6, (r.returncode, r.stdout, r.stderr[-500:])         # SIGABRT
    assert 'which nobody wrote' in r.stderr and 'rc' not in r.stdout
