"""The crafted inputs of tests/test_gpu_finalexp.py have the properties their families claim, under the oracle: a wrong generator
must not let the GPU test pass vacuously (say, an 'Fp6' element with odd coefficients, or a 'y^r' that is not one after the
final exponentiation)."""
import random

import pytest

import finalexp_cases as fc
from util import c

ODD = (1, 3, 5)      # the w^1, w^3, w^5 coefficients: zero exactly for the elements of Fp6


@pytest.fixture(scope='module')
def pool():
    return fc.family_pool()


def test_families_have_their_properties(pool):
    fams = {}
    for name, fam, v in pool:
        fams.setdefault(fam, []).append(name)
        if fam == 'Z':
            assert v is None and fc.record(v) == bytes(576)
            with pytest.raises(ValueError):           # 0 is not in Fp12*: the oracle cannot even invert it
                c.final_exponentiation((c.F2_ZERO,) * 6)
            assert fc.verdict(v) == fc.INVALID
            continue
        e = fc.easy_part(v)
        if fam == 'S':
            assert all(v[k] == c.F2_ZERO for k in ODD) and v != (c.F2_ZERO,) * 6, name
            assert e == c.F12_ONE, name               # every a^x of the hard part then has a = 1: z2 = 0, the compressed chain declines
            assert fc.verdict(v) == fc.OK, name
        elif fam == 'K':
            assert e != c.F12_ONE, name               # a nontrivial cyclotomic element: the compressed chain runs
            assert fc.verdict(v) == fc.OK, name
        elif fam == 'N':
            assert fc.verdict(v) == fc.INVALID, name
        else:
            assert fam == 'M'
            assert fc.verdict(v) == (fc.OK if 'valid_' in name and 'invalid' not in name else fc.INVALID), name
        assert fc.record(v) == fc.util.f12_record(v) and fc.util.f12_from_record(fc.record(v)) == v
    assert sorted(fams) == ['K', 'M', 'N', 'S', 'Z']
    assert {'one', 'minus_one'} <= set(fams['S'])
    assert any(n.startswith('y^r_') for n in fams['K']) and any(n.startswith('y^r*s_') for n in fams['K'])
    # y^r itself is one after the final exponentiation (not merely 'OK' through some other factor)
    yr = [v for name, _, v in pool if name.startswith('y^r_')]
    assert all(c.final_exponentiation(v) == c.F12_ONE for v in yr)


@pytest.mark.parametrize('k', [1, 2, 3, 17])
def test_product_sets_have_their_properties(k):
    sets = fc.product_sets(k, random.Random(100 + k))
    assert fc.product(sets['one'][0]) == c.F12_ONE and sets['one'][1] == fc.OK
    vals, v = sets['fp6']
    assert len(vals) == k and all(all(x[j] == c.F2_ZERO for j in ODD) for x in vals) and v == fc.OK
    assert all(x[j] == c.F2_ZERO for x in [fc.product(vals)] for j in ODD)
    names = sorted(sets)
    assert len(names) == 6
    for name in names:
        vals, v = sets[name]
        assert len(vals) == k
        if '_zero' in name:
            assert vals.count(None) == 1 and v == fc.INVALID
        elif '_y' in name:
            base = sets[name.split('_y')[0]][0]
            assert sum(a is not b for a, b in zip(vals, base)) == 1 and v == fc.INVALID
        else:
            assert None not in vals and v == fc.OK
