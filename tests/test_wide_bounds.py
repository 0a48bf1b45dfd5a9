"""Static magnitude check of the row-wide engine's tables (tools/gen_wide_tables.py OPS and OPS_PT; no GPU): every product row and every
linear row of both sets against the bounds that csrc/wide.cuh and csrc/wide_engine.cuh are written for.  The figures are read from the
device source (the comments that state each function's contract, the constants of w_finish), not repeated here.

Product row  A = sum ca V[a], B = sum cb V[b], every limb of a value at most L = 2^28 + 8 after a carry pass (w_norm):
  * each coefficient fits the signed byte it is packed into;
  * sum|c| L < 2^31: the operand sum is cast to 32 bits;
  * 14 (sum|ca| L)(sum|cb| L) < 2^62: the column sums of w_mul_cols.
Linear row  V[out] = reduce(sum k term):
  * at most WIDE_MAX_TERMS terms, each coefficient a signed 16-bit field;
  * the column sums that enter w_redc_cols -- a product term is a column of w_mul_cols (below 2^29.6), a plain term a limb L at
    columns 14.. -- stay below 2^62;
  * what leaves w_redc_cols fits w_finish's first carry pass, and the value is inside w_finish's range.

The range of w_finish, from its code.  Its input is one 64-bit limb sum per lane, value V = sum acc_j 2^(28 j).
  1. c1 = acc >> 28 goes through a 32-bit word: |acc| < 2^59.  A reduced column is the row's own column plus sum_s q_s p_(14+j-s) with
     q_s < 2^28: at most (2^28 - 1) (p_1 + ... + p_13) = 2^58.906 for limb 0, so the row's own columns may reach 2^59 - 2^58.906 = 2^54.9
     (they stay below 2^36.6).  The limb with its neighbour's carry on top, up to 2^28 + 2^30.91 = 2^31.09, does NOT fit a signed 32-bit
     word: the sum is formed on 64 bits (it was not before this check existed: a row whose quotient digits are all near 2^28, such as a
     product congruent to a small multiple of p modulo 2^392, wrapped limb 1 by 2^32).
  2. After that pass limbs 0..12 lie in [-C, 2^28 - 1 + C], C < 2^31 the largest carry, so V = top 2^364 + low with
     low / 2^364 inside (-8.01, 9.01), and top -- lane 13's limb plus lane 12's carry -- must fit 32 bits: |V| / 2^364 + 9.01 < 2^31,
     |V| < 20,161 p (2^364 is p / u, u = 106,513.12).
  3. k = rint(fl(fl(top) cf)), cf the float 1.0f / 106513.57f: two roundings of relative size 2^-24 each, so
     |k - V / p| <= 0.5 + |top| (|cf - 1 / u| + cf (2^-23 + 2^-48)) + 9.01 / u, which is below 0.6 while |top| < 2.47e9, |V| < 23,221 p:
     beyond what 32 bits hold.  V - k p is then inside (-0.6 p, 0.6 p), and k p is subtracted on 64 bits.
So w_finish is exact for |V| < 20,161 p, the 32-bit top limb being the binding condition.  The largest value a row of today's tables can
hand it is 2.21 p: the rows with the largest sum|k| (110, 120) sum PRODUCTS, and a product a b / R of operands below 1.2 p is below
1.44 p (p / R) = p / 1,760; only plain terms count 0.6 p each (a row holds at most two), and the reduction adds less than p."""
import math
import os
import re
from fractions import Fraction as F

import numpy as np

import util
import wide_tables_check as chk

g = chk.g
P = g.P
CSRC = os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc')
WIDE = open(os.path.join(CSRC, 'wide.cuh')).read()
ENGINE = open(os.path.join(CSRC, 'wide_engine.cuh')).read()
TMP, CONST = g.TMP, g.CONST
PL = [(P >> (28 * i)) & (2**28 - 1) for i in range(13)] + [P >> 364]


def stated(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return m


def pow2(m, k=1):
    return 2**float(m.group(k))


# what the device source states
L = 2**28 + int(stated(WIDE, r'one parallel carry pass.*?come back below 2\^28 \+ (\d+)').group(1))
NORM_IN = pow2(stated(WIDE, r'one parallel carry pass.*?limbs with magnitude below 2\^(\d+)'))
MULCOLS_IN = pow2(stated(WIDE, r'a \* b / R mod p; operand limbs:.*?must stay below 2\^(\d+)'))
MULCOLS_OUT = pow2(stated(WIDE, r'w_mul_cols: the 27 columns.*?\(below\s*//\s*2\^([0-9.]+)\)'))
REDC_IN = pow2(stated(WIDE, r'w_redc_cols: Montgomery reduction of 28 columns.*?magnitudes below 2\^(\d+)'))
REDC_OUT = pow2(stated(WIDE, r'w_redc_cols: Montgomery reduction.*?lane j: limb j, below 2\^(\d+)'))
FINISH_IN = pow2(stated(ENGINE, r'limb sums of a linear phase \(magnitude below 2\^(\d+)'))
FINISH_DIV = stated(ENGINE, r'w_finish\(int64_t acc.*?__float2int_rn\(\(float\)top \* \(1\.0f / ([0-9.]+)f\)\)').group(1)
MAX_TERMS = int(stated(ENGINE, r'#define WIDE_MAX_TERMS (\d+)').group(1))
VALUE = F(3, 5)                 # every value of the store: |value| < 0.6 p (the engine's output contract); constants are canonical, below p


def finish_range():
    """(|V| / p for which the 32-bit top limb is exact, |V| / p for which the float estimate lands within 0.6): the docstring's 2 and 3"""
    u = F(P, 2**364)
    slack = F(901, 100)
    top_fit = (2**31 - 1 - slack) / u
    cf = np.float32(1.0) / np.float32(float(FINISH_DIV))
    assert cf.dtype == np.float32
    cf = F(float(cf))
    per_top = abs(cf - 1 / u) + cf * (F(1, 2**23) + F(1, 2**48))
    top_float = (F(6, 10) - F(1, 2) - slack / u) / per_top
    return top_fit, top_float / u


def redc_growth():
    """the most a Montgomery reduction adds to a column that survives it: sum_s q_s p_(14+j-s), q_s < 2^28, largest for limb 0"""
    return (2**28 - 1) * sum(PL[1:])


def row_figures(op):
    prods, lins = [], []
    by_out = {o: (a, b) for a, b, o in op.prods}
    for a, b, o in op.prods:
        sa, sb = sum(abs(k) for k, _ in a), sum(abs(k) for k, _ in b)
        prods.append({'op': op.name, 'shape': (sa, sb), 'coefs': [k for k, _ in a + b], 'cast': max(sa, sb) * L, 'cols': 14 * (sa * L) * (sb * L)})
    for terms, o in op.lins:
        cols, value, has_prod = 0, F(0), False
        for k, i in terms:
            if (i >> 12) == TMP:
                a, b = by_out[i]
                has_prod = True
                cols += abs(k) * math.ceil(MULCOLS_OUT)
                value += abs(k) * sum(abs(x) for x, _ in a) * sum(abs(x) for x, _ in b) * F(P, 2**392)       # |a b / R| < sa sb p (p / R)
            else:
                assert (i >> 12) == g.SA, 'a linear row reads products and plain values of A only'
                cols += abs(k) * L
                value += abs(k) * VALUE
        acc = cols
        if has_prod:                    # through w_redc_cols: q p / R < p on the value, the reduction's growth and its last carry on the limb sums
            value += 1
            acc = cols + redc_growth() + (cols + 14 * 2**56) // (2**28 - 1) + 1
        lins.append({'op': op.name, 'terms': len(terms), 'coefs': [k for k, _ in terms], 'sumk': sum(abs(k) for k, _ in terms), 'cols': cols, 'acc': acc,
                     'value': value, 'reduced': has_prod})
    return prods, lins


def all_rows(ops):
    prods, lins = [], []
    for op in ops:
        p, l = row_figures(op)
        prods += p
        lins += l
    return prods, lins


SETS = (('F12', g.OPS), ('PT', g.OPS_PT))


def test_the_stated_contracts_chain():
    """each function's stated output is a legal input of the next one, on the figures the source states"""
    assert L == 2**28 + 8 and NORM_IN == 2**31 and MULCOLS_IN == 2**62 and REDC_IN == 2**62
    # w_mul_cols: a column of magnitude below 2^63 leaves three fields; the busiest column takes its own low field, two middle fields and
    # two high ones (at most 2^63 / 2^56 each)
    assert 3 * 2**28 + 2 * 2**7 < MULCOLS_OUT < 2**31
    # w_redc_cols -> w_finish: the first carry goes through a 32-bit word
    assert redc_growth() < REDC_OUT <= FINISH_IN <= 2**59
    assert abs(math.log2(redc_growth()) - 58.906) < 1e-3
    # ... and a limb with that carry on top does not fit 32 bits, which is why w_finish forms it on 64
    assert 2**28 + (redc_growth() >> 28) > 2**31
    assert re.search(r'const int64_t v1 = \(acc & keep64\) \+ \(int64_t\)w_shr<1>\(c1m\);', ENGINE)
    fit, flt = finish_range()
    print('w_finish: top limb exact for |V| < %.1f p, float estimate within 0.6 for |V| < %.1f p' % (float(fit), float(flt)))
    assert 20161 < fit < 20162 < flt and 23221 < flt < 23222
    assert g.FINISH_MAX_P <= fit and g.LIMB_MAX == L and g.COL_MAX >= MULCOLS_OUT and g.REDC_COL_MAX == REDC_IN and g.MAXLIN == MAX_TERMS
    for k, v in (('w_finish', '20,161 p'), ('fp_reduce', '20,000 p')):
        assert v in (ENGINE if k == 'w_finish' else WIDE)


def test_every_product_row():
    for name, ops in SETS:
        prods, _ = all_rows(ops)
        assert prods
        for r in prods:
            assert all(-128 <= k < 128 for k in r['coefs']), r
            assert r['cast'] < 2**31, r
            assert r['cols'] < MULCOLS_IN, r
        w = max(prods, key=lambda r: r['cols'])
        shapes = {}
        for r in prods:
            shapes[r['shape']] = shapes.get(r['shape'], 0) + 1
        print('set %s: %d product rows, shapes %s; worst %s row of %s: columns 2^%.3f, margin to 2^62: %.3f bits; operand sum 2^%.3f of 2^31' % (
            name, len(prods), sorted(shapes.items()), w['shape'], w['op'], math.log2(w['cols']), 62 - math.log2(w['cols']), math.log2(w['cast'])))
        assert set(shapes) == {(1, 1), (2, 2)} and max(abs(k) for r in prods for k in r['coefs']) <= 2
        assert shapes == ({(1, 1): 445, (2, 2): 145} if name == 'F12' else {(1, 1): 624, (2, 2): 256})
        assert abs(math.log2(w['cols']) - 61.81) < 0.005


def test_every_linear_row():
    fit, flt = finish_range()
    limit = min(fit, flt)
    for name, ops in SETS:
        _, lins = all_rows(ops)
        assert lins
        for r in lins:
            assert r['terms'] <= MAX_TERMS, r
            assert all(-32768 <= k < 32768 for k in r['coefs']), r
            assert r['cols'] < REDC_IN, r
            assert r['acc'] < FINISH_IN and (r['acc'] >> 28) < 2**31, r
            assert r['value'] < limit, r
        wk = max(lins, key=lambda r: r['sumk'])
        wv = max(lins, key=lambda r: r['value'])
        wc_ = max(lins, key=lambda r: r['cols'])
        print('set %s: %d linear rows; most terms %d; max |k| %d; max sum|k| %d (%s); largest value into w_finish %.2f p (%s), range %.0f p: '
              'margin x%.0f; largest column sum into w_redc_cols 2^%.2f (%s) of 2^62; largest limb sum into w_finish 2^%.3f of 2^59' % (
                  name, len(lins), max(r['terms'] for r in lins), max(abs(k) for r in lins for k in r['coefs']), wk['sumk'], wk['op'], float(wv['value']),
                  wv['op'], float(limit), float(limit / wv['value']), math.log2(wc_['cols']), wc_['op'], math.log2(max(r['acc'] for r in lins))))
        assert max(abs(k) for r in lins for k in r['coefs']) == 72
        assert (wk['sumk'], max(r['terms'] for r in lins)) == ((110, 18) if name == 'F12' else (120, 16))
        assert (wk['op'] == 'PDBL1') if name == 'F12' else (wk['op'] == 'C2ADD1X4')


def test_the_generator_refuses_rows_past_the_bounds():
    """the same conditions are assertions of the generator: a table change that breaks one fails when the header is generated"""
    import pytest
    op = g.Op('T')
    a, b = g.idx(g.SA, 0), g.idx(g.SA, 1)
    with pytest.raises(AssertionError):
        op.prod([(2, a), (1, b)], [(2, a), (1, b)])             # (3,3): 14 (3 L)^2 > 2^62
    with pytest.raises(AssertionError):
        op.prod([(128, a)], [(1, b)])                           # not a signed byte
    t = op.prod([(1, a), (1, b)], [(1, a), (-1, b)])
    with pytest.raises(AssertionError):
        op.lin([(40000, t)], g.idx(g.DST, 0))                   # not a signed 16-bit field
    with pytest.raises(AssertionError):
        op.lin([(k + 1, g.idx(g.SA, k)) for k in range(g.MAXLIN + 1)], g.idx(g.DST, 0))
    with pytest.raises(AssertionError):
        op.lin([(32767, a), (32767, b)], g.idx(g.DST, 0))       # 39,320 p: past w_finish's range
    op.lin([(16000, a), (16000, b)], g.idx(g.DST, 0))           # 19,200 p: inside
