"""The Miller loop of two TABLED pairs of the wave-cooperative engine (csrc/coop.cuh coop_miller2_tables, what k_pairing_coop_keyed
runs) on the host: tests/hostsim_coop_keyed compiles the round functions the device compiles, one thread per lane pair, with the
bound tracker on and every element's bounds carried through its LDS slot.  Pair 0's rows are built from the case's Q0 by the
key-set build path (keyset_lines_entry), pair 1's are G2NEGC_LINES_N.  The easy-part value must equal the oracle's exactly (the
Fp2 factors of the normalisation die there), the verdict must be the oracle's, and the tracker stays silent, which proves the
placement of the reductions in the new rounds.  The new reduction mode and the merge round are also run on their own against Python
integers, on operands at the bounds the tracker assumes for them."""
import ctypes
import os
import random
import subprocess

import pytest

import field_cases as fc
import util
from util import P, limbs_of, val

HERE = os.path.join(util.ROOT, 'tests', 'hostsim_coop_keyed')
LB = float(1 << 28)


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(HERE, 'coop_keyed_hostsim.cpp')
    so = os.path.join(HERE, 'libcoop_keyed_hostsim.so')
    csrc = os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc')
    deps = [src, os.path.join(util.ROOT, 'tests', 'hostsim_coop', 'coop_hostsim.cpp')] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.cuh', '.h'))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(['g++', '-O2', '-fwrapv', '-pthread', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, src])
    return ctypes.CDLL(so)


KEYED = [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == 2]


def test_the_case_list_is_what_the_tests_below_rely_on():
    assert len(KEYED) >= 12 and {fc.pairing_expected(cs)[2] for cs in KEYED} == {fc.BLS_OK, fc.BLS_INVALID}
    assert all(cs['pairs'][1][1] == fc.g2_negc() for cs in KEYED)
    names = ' | '.join(cs['name'] for cs in KEYED)
    assert 'outside the subgroups' in names and 'largest canonical' in names and 'negative representative' in names


@pytest.mark.parametrize('cs', KEYED, ids=[cs['name'] for cs in KEYED])
def test_tabled_miller_loop_and_final_exponentiation_on_the_host(lib, cs):
    """coop_miller2_tables, then coop_final_easy -- the exact Fp12 value against the oracle -- and coop_final_verdict"""
    (qx, qy) = cs['pairs'][0][1]
    rec = util.fp2_raw(qx) + util.fp2_raw(qy)
    assert len(rec) == 192
    flat = (ctypes.c_int32 * 168)(*[x for v in cs['vecs'] for x in v])
    out = (ctypes.c_int32 * 168)()
    assert lib.hs_coop_pairing_keyed(0, flat, rec, out) == 0
    o = list(out)
    fc.check_easy(cs, [o[14 * k:14 * (k + 1)] for k in range(12)])
    assert lib.hs_coop_pairing_keyed(1, flat, rec, out) == fc.pairing_expected(cs)[2], cs['name']


# ---- the two new rounds on their own.  Operands are limb vectors with exact limbs whose VALUES sit at the bounds the tracker holds
# for them: a staged product or a loaded row word is within 1.125 p in magnitude (fp.cuh: REDC output, fp_load)
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


XI = (1, 1)
TOP = 9 * P // 8                     # the largest value of a staged product or a loaded word
EDGE = (TOP, -TOP, P - 1, -(P // 8), 0, 1, -1, P // 2, -(P // 2))


def operand_sets(n, count=6):
    """lists of n residues (integers in the internal form's range): each edge value in every slot, mixed edges, random values"""
    rng = random.Random(n)
    out = [[e] * n for e in EDGE]
    out += [[rng.choice(EDGE) for _ in range(n)] for _ in range(count)]
    out += [[rng.randrange(-TOP, TOP + 1) for _ in range(n)] for _ in range(count)]
    return out


def run(fn, residues, n_out):
    flat = [x for v in residues for x in limbs_of(v)]
    n = len(residues)
    out = (ctypes.c_int32 * (14 * n_out))()
    fn((ctypes.c_int32 * len(flat))(*flat), (ctypes.c_double * n)(*([LB] * n)), (ctypes.c_double * n)(*([1.125] * n)), out)
    o = list(out)
    vecs = [o[14 * k:14 * (k + 1)] for k in range(n_out)]
    for v in vecs:                   # every coefficient leaves reduced, or (c4) as the product it is
        assert all(0 <= x < (1 << 28) for x in v[:13]) and abs(val(v)) * 1000 <= 1125 * P
    return [(util.elem_of(vecs[2 * k]), util.elem_of(vecs[2 * k + 1])) for k in range(n_out // 2)]


def elems(residues):
    e = [v * util.R392_INV % P for v in residues]
    return [(e[2 * k], e[2 * k + 1]) for k in range(len(e) // 2)]


def test_reduction_of_thirty_products(lib):
    """coop_reduce_line5: coefficient k = sum_{i + j = k} P_ij + xi sum_{i + j = k + 6} P_ij over j in {0, 2, 3, 4, 5}; all thirty
    products at +-1.125 p put five like terms of the largest magnitude on every anti-diagonal"""
    lib.hs_coop_reduce_line5.restype = None
    jw = (0, 2, 3, 4, 5)
    for res in operand_sets(60):
        prod = elems(res)
        want = [(0, 0)] * 6
        for i in range(6):
            for c, j in enumerate(jw):
                t = prod[5 * i + c]
                k = (i + j) % 6
                want[k] = f2_add(want[k], f2_mul(XI, t) if i + j >= 6 else t)
        assert run(lib.hs_coop_reduce_line5, res, 12) == want


def test_merge_round(lib):
    """the seven products and their combination: (a0 + a2 w^2 + ya w^3)(b0 + b2 w^2 + yb w^3) = c0 + c2 w^2 + c3 w^3 + c4 w^4 + c5 w^5
    with w^6 = xi; a0 + a2 and b0 + b2 enter their product unnormalised (limbs up to 2^29, values up to 2.25 p)"""
    lib.hs_coop_merge_round.restype = None
    for res in operand_sets(10):
        e = [v * util.R392_INV % P for v in res]
        a0, a2, b0, b2 = ((e[2 * k], e[2 * k + 1]) for k in range(4))
        ya, yb = (e[8], 0), (e[9], 0)
        want = [f2_add(f2_mul(a0, b0), f2_mul(XI, f2_mul(ya, yb))), f2_add(f2_mul(a0, b2), f2_mul(a2, b0)), f2_add(f2_mul(a0, yb), f2_mul(b0, ya)),
                f2_mul(a2, b2), f2_add(f2_mul(a2, yb), f2_mul(b2, ya))]
        assert run(lib.hs_coop_merge_round, res, 10) == want
