"""Inputs and the Python model of the G1 map with an affine isogeny (csrc/h2c.cuh: sswu_g1 hands out 1 / xd from its square-root
chain, iso_map_g1 runs four plain Horner chains at x = xn / xd), shared by tests/test_h2c_affine_iso.py and
tests/test_gpu_h2c_affine_iso.py.  Everything is built from oracle/py and tests/h2c_cases.py, deterministic (seeded), once per process.

INPUTS: 96 field elements u, each with a 64-byte writing u + k p (h2c_cases.lift):
  16  the pole preimages (SSWU lands on a root of the isogeny's x-denominator: the map is the identity)
   2  the inputs with tv2 = 0 (xd takes its exceptional value Z A)
   3  u = 0, 1, p - 1
  32  random u with g(x1) a square        chi = +1
  32  random u with g(x1) a non-square    chi = -1
  11  random u, unclassified

model_sswu / model_iso restate the device's straight-line sequence on Python integers: the same intermediate values, so the identity
that the inverse rests on is checked on exactly what the device multiplies together."""
import functools
import random

import h2c_cases as hc
from oracle.py import bls381 as c
from oracle.py import iso_consts as iso

P = c.P
A, B, Z = iso.G1_A % P, iso.G1_B % P, iso.G1_Z % P
XNUM, XDEN, YNUM, YDEN = iso.G1_ISO


def model_sswu(u):
    """sswu_g1 of csrc/h2c.cuh, value by value: {'xn', 'xd', 'y', 'gx1' (numerator of g(x1) over xd^3), 'w', 'c', 'is_qr', 'xinv'}"""
    tv1 = Z * u * u % P
    tv2 = (tv1 * tv1 + tv1) % P
    tv3 = B * (tv2 + 1) % P
    tv4 = A * (Z if tv2 == 0 else -tv2) % P                  # xd
    xd2 = tv4 * tv4 % P
    gx1 = ((tv3 * tv3 + A * xd2) * tv3 + B * xd2 * tv4) % P
    gxd = xd2 * tv4 % P
    s1 = gxd * gxd % P                                       # xd^6
    s2 = gx1 * gxd % P
    m = s1 * xd2 % P * gx1 % P                               # gx1 xd^8, formed before the chain
    w = s1 * s2 % P                                          # gx1 gxd^3
    cc = pow(w, (P - 3) // 4, P)
    y1 = cc * s2 % P
    is_qr = y1 * y1 % P * gxd % P == gx1
    xinv = m * cc % P * cc % P
    if not is_qr:
        xinv = -xinv % P
    y2 = y1 * pow(-Z % P, (P + 1) // 4, P) % P
    xn = tv3 if is_qr else tv1 * tv3 % P
    y = y1 if is_qr else tv1 * u % P * y2 % P
    if (u & 1) != (y & 1):
        y = -y % P
    return {'xn': xn, 'xd': tv4, 'y': y, 'gx1': gx1, 'w': w, 'c': cc, 'is_qr': is_qr, 'xinv': xinv}


def horner(k, x, monic):
    """acc <- acc x + k[i] from the top; a monic polynomial starts with the ADDITION x + k[D - 1]"""
    if monic:
        assert k[-1] == 1
        acc = (x + k[-2]) % P
        rest = k[:-2]
    else:
        acc = k[-1] % P
        rest = k[:-1]
    for kk in reversed(rest):
        acc = (acc * x + kk) % P
    return acc


def model_iso(x, y):
    """iso_map_g1 of csrc/h2c.cuh at an affine x: the Jacobian (X, Y, Z) = (XN XD YD^2, y YN XD^3 YD^2, XD YD)"""
    xn, xd, yn, yd = horner(XNUM, x, False), horner(XDEN, x, True), horner(YNUM, x, False), horner(YDEN, x, True)
    yd2 = yd * yd % P
    return (xn * xd % P * yd2 % P, y * yn % P * pow(xd, 3, P) % P * yd2 % P, xd * yd % P)


def jac_to_affine(pt):
    X, Y, Zc = pt
    if Zc == 0:
        return None
    zi = pow(Zc, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def model_map(u):
    s = model_sswu(u)
    return jac_to_affine(model_iso(s['xn'] * s['xinv'] % P, s['y']))


@functools.lru_cache(maxsize=None)
def inputs():
    """[{'name', 'u', 'block' (64 bytes), 'kind'}] x 96, the same list on every call"""
    rng = random.Random(0x61666669)
    out = []

    def put(kind, name, u):
        out.append({'kind': kind, 'name': name, 'u': u, 'block': hc.lift(u, rng)})

    for i, u in enumerate(hc.g1_pole_preimages(rng)):
        put('pole', 'pole %d' % i, u)
    for nm, u in zip(('+s', '-s'), hc.g1_tv2_zero_inputs()):
        put('tv2', 'tv2 = 0: u = %s' % nm, u)
    for nm, u in (('0', 0), ('1', 1), ('p-1', P - 1)):
        put('small', 'u = %s' % nm, u)
    poles = {d['u'] for d in out if d['kind'] == 'pole'}
    want = {True: 32, False: 32}
    while want[True] or want[False]:
        u = rng.randrange(1, P)
        cl = hc.classify(1, u)
        if cl is None or u in poles or not want[cl[0]]:
            continue
        want[cl[0]] -= 1
        put('square' if cl[0] else 'nonsquare', 'random %s %d' % ('square' if cl[0] else 'non-square', 32 - want[cl[0]] - 1), u)
    while len(out) < 96:
        put('random', 'random %d' % len(out), rng.randrange(P))
    assert len(out) == 96 and len({d['u'] for d in out}) == 96
    assert all(int.from_bytes(d['block'], 'big') % P == d['u'] for d in out)
    assert any(int.from_bytes(d['block'], 'big') >= P for d in out)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """the oracle's map_to_curve_g1 of every input (None at the poles), in the order of inputs()"""
    return tuple(c.map_to_curve_g1(d['u']) for d in inputs())


@functools.lru_cache(maxsize=None)
def pairs():
    """the 96 inputs as 96 items of 128 uniform bytes: input i in position 0 beside input (i + 37) mod 96 in position 1 (37 is
    coprime to 96: every input sits once in each position, every pole beside a regular element), with Q = the sum of the two maps and
    H = [1 - x] Q as tests/h2c_cases.py defines them; cases in h2c_cases' format (h2c_cases.check takes them)"""
    ins, ex = inputs(), expected()
    out = []
    for i in range(96):
        j = (i + 37) % 96
        q = c.E1.add(ex[i], ex[j])
        out.append({'name': '%s | %s' % (ins[i]['name'], ins[j]['name']), 'group': 1, 'uniform': ins[i]['block'] + ins[j]['block'],
                    'u': (ins[i]['u'], ins[j]['u']), 'Q': q, 'H': c.E1.mul(q, c.H_EFF_G1)})
    return out
