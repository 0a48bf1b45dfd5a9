"""The G1 map with the 11-isogeny at an affine x (csrc/h2c.cuh sswu_g1_inv + iso_map_g1), on the 96 inputs of
tests/h2c_affine_cases.py: the facts the inverse rests on, the Python restatement of the device's sequence against the oracle, and
the compiled headers (tests/hostsim_h2c_affine, bound tracker on) against both.  Every comparison is exact."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import h2c_affine_cases as ac
import h2c_cases as hc
import util
from oracle.py import bls381 as c
from oracle.py import iso_consts as iso

P = c.P
SRC = os.path.join(util.ROOT, 'tests', 'hostsim_h2c_affine', 'h2c_affine_hostsim.cpp')


def test_inputs_are_what_they_claim():
    ins = ac.inputs()
    assert ins is ac.inputs() and len(ins) == 96
    kinds = {}
    for d in ins:
        kinds.setdefault(d['kind'], []).append(d)
    assert {k: len(v) for k, v in kinds.items()} == {'pole': 16, 'tv2': 2, 'small': 3, 'square': 32, 'nonsquare': 32, 'random': 11}
    assert [d['u'] for d in kinds['small']] == [0, 1, P - 1]
    assert all(c.map_to_curve_g1(d['u']) is None for d in kinds['pole'])
    assert all(hc.classify(1, d['u']) is None for d in kinds['tv2'])
    assert all(ac.model_sswu(d['u'])['is_qr'] for d in kinds['square'])
    assert not any(ac.model_sswu(d['u'])['is_qr'] for d in kinds['nonsquare'])
    # liftings u + k p: most blocks are not the canonical writing
    assert sum(int.from_bytes(d['block'], 'big') >= P for d in ins) > 80
    assert [e is None for e in ac.expected()] == [d['kind'] == 'pole' for d in ins]


def test_e1_iso_has_no_point_of_order_two():
    """x^3 + A'x + B' has no root in Fp: gx1 = 0 would be a point (x1, 0) of order 2 on E1', so w = gx1 gxd^3 is never zero"""
    assert hc.fp_roots([iso.G1_B, iso.G1_A, 0, 1], random.Random(3)) == []
    h = (c.X - 1) ** 2 // 3                                          # #E1(Fp) = h r is odd, and an isogeny keeps the order
    assert (c.X - 1) ** 2 % 3 == 0 and h * c.R % 2 == 1 and (P + 1 - h * c.R) ** 2 <= 4 * P


def test_inverse_out_of_the_square_root_chain():
    """chi c^2 gx1 xd^8 xd = 1 with c = w^((p-3)/4), w = gx1 gxd^3 and chi = +1 / -1 as is_qr says, on every input"""
    signs = set()
    for d in ac.inputs():
        s = ac.model_sswu(d['u'])
        assert s['w'] != 0 and s['xd'] != 0 and s['gx1'] != 0, d['name']
        assert s['w'] == s['gx1'] * pow(s['xd'], 9, P) % P
        chi = 1 if s['is_qr'] else P - 1
        assert pow(s['w'], (P - 1) // 2, P) == chi, d['name']          # is_qr is the quadratic character of w
        assert chi * s['c'] * s['c'] % P * s['gx1'] % P * pow(s['xd'], 8, P) % P * s['xd'] % P == 1, d['name']
        assert s['xinv'] * s['xd'] % P == 1, d['name']
        signs.add(s['is_qr'])
        # and the model's SSWU point is the oracle's
        assert (s['xn'] * s['xinv'] % P, s['y']) == c._sswu(c.E1_ISO, iso.G1_Z, d['u'], c.fp_is_square, c.fp_sqrt, c._sgn0_fp, 1), d['name']
    assert signs == {True, False}


def test_affine_horner_and_jacobian_assembly():
    """the four plain Horner chains (monic denominators start with an addition) and (XN XD YD^2, y YN XD^3 YD^2, XD YD) give
    map_to_curve_g1(u): the identity (Z = 0) at the 16 poles and nowhere else"""
    assert iso.G1_ISO[1][-1] == 1 and iso.G1_ISO[3][-1] == 1
    assert [len(t) - 1 for t in iso.G1_ISO] == [11, 10, 15, 15]
    for d, want in zip(ac.inputs(), ac.expected()):
        s = ac.model_sswu(d['u'])
        jac = ac.model_iso(s['xn'] * s['xinv'] % P, s['y'])
        assert ac.jac_to_affine(jac) == want, d['name']
        assert (jac[2] == 0) == (d['kind'] == 'pole'), d['name']
        if want is not None:
            assert c.E1.on_curve(want)


# ---------------------------------------------------------------- the compiled headers, bound tracker on
@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='h2c_affine_hostsim_'), 'libh2c_affine_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_affine_map.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    lb.hs_affine_map.restype = None
    lb.hs_sswu_plain.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    lb.hs_sswu_plain.restype = None
    lb.hs_affine_hash_map.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    lb.hs_affine_hash_map.restype = None
    return lb


def _fps(raw, n):
    return [hc._fp(raw[48 * k:48 * k + 48]) for k in range(n)]


def test_host_build_sswu_and_isogeny(lib):
    """sswu_g1_inv and iso_map_g1 as compiled: every output of the square-root function equals the model's (the root's sign
    included: the model takes the device's root), the inverse is the inverse, and the Jacobian point normalises to the oracle's"""
    for d, want in zip(ac.inputs(), ac.expected()):
        out = ctypes.create_string_buffer(8 * 48)
        lib.hs_affine_map(d['block'], out)
        xn, xd, y, xinv, x, X, Y, Zc = _fps(out.raw, 8)
        s = ac.model_sswu(d['u'])
        assert (xn, xd, y, xinv) == (s['xn'], s['xd'], s['y'], s['xinv']), d['name']
        assert xinv * xd % P == 1 and x == xn * xinv % P, d['name']
        assert (X, Y, Zc) == ac.model_iso(x, y), d['name']
        assert ac.jac_to_affine((X, Y, Zc)) == want, d['name']
        assert (Zc == 0) == (d['kind'] == 'pole'), d['name']


def test_host_build_form_without_the_inverse_is_unchanged(lib):
    """sswu_g1 as the row-wide engine's callers see it (here on fp): xn, xd, y as before"""
    for d in ac.inputs():
        out = ctypes.create_string_buffer(3 * 48)
        lib.hs_sswu_plain(d['block'], out)
        s = ac.model_sswu(d['u'])
        assert tuple(_fps(out.raw, 3)) == (s['xn'], s['xd'], s['y']), d['name']


@pytest.mark.parametrize('uncleared', (0, 1))
def test_host_build_hash_to_g1_map(lib, uncleared):
    """hash_to_g1_map (the one-lane form; what hash_to_g1 and the door blsgpu_debug_map_to_curve run) on the inputs in pairs"""
    for cs in ac.pairs():
        out = ctypes.create_string_buffer(144)
        lib.hs_affine_hash_map(cs['uniform'], uncleared, out)
        hc.check(cs, out.raw, uncleared, 'host build, affine isogeny,')
