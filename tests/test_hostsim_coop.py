"""The wave-cooperative pairing engine (csrc/coop.cuh) on the host: tests/hostsim_coop compiles the very round functions the device
compiles, runs a wave as 32 threads (one per lane pair) and keeps the bound tracker of fp.cuh on, with every element's tracked bounds
carried through its LDS slot.  tests/test_field_cases.py runs the whole case list of every COOP_* row through it; here are the
alias modes, the fills, the properties the case lists claim for themselves, and coop_miller2 + coop_final_easy / coop_final_verdict
on the crafted pairs of field_cases.pairing_cases -- the cases tests/test_gpu_coop_ops.py gives to the shipped kernels.  Every
expected value is from Python integers and the oracle's tower."""
import ctypes

import pytest

import field_cases as fc
import util
from util import c, P, val

COOP_OPS = sorted(op for op in fc.build() if op.startswith('COOP_'))


@pytest.fixture(scope='module')
def lib():
    return util.build_hostsim_coop()


@pytest.fixture(scope='module')
def table(pkg):
    return pkg.api.field_op_table()


def run_op(lib, table, op, cs, reps=1):
    opid, lanes, n_in, n_out, n_par, _ = table[op]
    assert lanes == 64 and len(cs['vecs']) == n_in and len(cs['par']) == n_par, (op, cs['name'])
    flat = [x for v in cs['vecs'] for x in v]
    out = (ctypes.c_int32 * (14 * n_out))()
    rc = lib.hs_coop_op(opid, (ctypes.c_int32 * len(flat))(*flat), (ctypes.c_double * n_in)(*cs['lb']), (ctypes.c_double * n_in)(*cs['vb']),
                        (ctypes.c_int32 * n_in)(*cs['nn']), (ctypes.c_int32 * n_par)(*cs['par']), reps, out)
    assert rc == 0, op
    o = list(out)
    return [o[14 * k:14 * (k + 1)] for k in range(n_out)]


def test_rows_are_the_cooperative_ones(table):
    assert set(COOP_OPS) == {op for op, row in table.items() if row[1] == 64} and len(COOP_OPS) == 13
    for op in COOP_OPS:
        assert table[op][4] >= 1, op          # the last parameter is the fill


@pytest.mark.parametrize('op', sorted(fc.COOP_ALIASES))
def test_every_alias_mode(lib, table, op):
    """dst apart, dst = a and (coop_mul) dst = b, as coop_final_verdict and coop_pow_x call them: every case of the list in every
    mode, and the chains at 2 and 17 repetitions"""
    lst = fc.build()[op]
    for alias in fc.COOP_ALIASES[op]:
        for cs in lst:
            fc.check(op, fc.with_pars(cs, first=alias), run_op(lib, table, op, fc.with_pars(cs, first=alias)))
        for reps, stride in fc.CHAIN_REPS[:2]:
            for cs in fc.chain_cases(op, stride)[:8]:
                v = fc.with_pars(cs, first=alias)
                fc.check(op, v, run_op(lib, table, op, v, reps), reps)


@pytest.mark.parametrize('op', COOP_OPS)
def test_fills_change_nothing(lib, table, op):
    """the first cases of every row with each fill word: right, and (but for the slots coop_jobs leaves alone) the same limbs"""
    for cs in fc.build()[op][:6]:
        outs = []
        for fill in fc.FILLS:
            v = fc.with_pars(cs, fill=fill)
            outs.append(run_op(lib, table, op, v))
            fc.check(op, v, outs[-1])
        if op != 'COOP_JOBS':
            assert outs[0] == outs[1] == outs[2], (op, cs['name'])


def test_same_sign_cases_are_what_they_say():
    """the operands named "same-sign products": every one of the 36 products a_i b_j (21 for the squaring, 18 for the line) has the named
    part of the named sign, as integers -- so the anti-diagonal sums of six like terms are reached"""
    part = lambda a, b, im: a[0] * b[1] + a[1] * b[0] if im else a[0] * b[0] - a[1] * b[1]
    seen = 0
    for op, nb in (('COOP_MUL', 6), ('COOP_SQR', 0), ('COOP_MUL_LINE', 3)):
        for cs in fc.build()[op]:
            if not cs['name'].startswith('same-sign') or 'negated' in cs['name'].split(',')[-1]:
                continue
            v = [val(l) for l in cs['vecs']]
            a = [(v[2 * k], v[2 * k + 1]) for k in range(6)]
            b = [(v[12 + 2 * k], v[13 + 2 * k]) for k in range(nb)] if nb else a
            im = 'imaginary' in cs['name']
            want = -1 if 'all negative' in cs['name'] else 1
            for x in a:
                for y in b:
                    assert part(x, y, im) * want > 0, (op, cs['name'])
            seen += 1
    assert seen == 2 * 4 + 2 * 5 + 2 * 4


def test_pow_x_restated_is_the_power_in_the_cyclotomic_subgroup():
    """what fixes "right" for COOP_POW_X (squarings by the Granger-Scott formulas, defined for any input) is conj(f^|x|) where it must be"""
    import random
    for nm, g in fc.cyclotomic_elements(random.Random(5)):
        assert fc.coop_pow_x(g) == c.f12_conj(c.f12_pow(g, c.X_ABS)), nm


def test_final_exponentiation_cases_have_both_verdicts():
    """r-th powers, elements of Fp6 and Fp2 (times a power of w: the single components), one and minus one give OK; random elements and zero (fp12_inv(0) = 0) INVALID"""
    got = {cs['name']: fc.final_verdict(fc.f12_of_vecs(cs['vecs'])) for cs in fc.build()['COOP_FINAL_VERDICT']}
    for nm, st in got.items():
        one = nm.startswith(('r-th power', 'element of', 'one', 'minus one', 'single component'))
        assert st == (fc.BLS_OK if one else fc.BLS_INVALID), nm
    assert got['zero'] == fc.BLS_INVALID and sum(st == fc.BLS_OK for st in got.values()) >= 8 and sum(st != fc.BLS_OK for st in got.values()) >= 8


# ---- the crafted pairs
def test_pair_cases_are_regular():
    """every point on its curve, no exceptional step in the 63-iteration walk of either Q, the oracle's Miller value invertible; both
    verdicts under every fixed_g2; points outside the subgroups present; the two representatives of a coordinate congruent"""
    cases = fc.pairing_cases()
    for a, b in zip(cases, cases[1:] + cases[:1]):
        assert a['vecs'] != b['vecs'] or a['fixed_g2'] != b['fixed_g2']
    fixed_q = {1: c.E2.neg(c.G2_GEN), 2: fc.g2_negc()}
    for cs in cases:
        for p, q in cs['pairs']:
            assert p is not None and q is not None and c.E1.on_curve(p) and c.E2.on_curve(q), cs['name']
            assert fc.miller_walk_is_regular(q), cs['name']
        if cs['fixed_g2']:
            assert cs['pairs'][1][1] == fixed_q[cs['fixed_g2']], cs['name']
        m, easy, st = fc.pairing_expected(cs)
        assert m != fc.F12_ZERO and c.f12_mul(m, c.f12_inv(m)) == fc.F12_ONE, cs['name']
        assert st == (fc.BLS_OK if 'product one' in cs['name'] else fc.BLS_INVALID), cs['name']
        got = [util.elem_of(v) for v in cs['vecs']]
        want = [z for (px, py), ((a0, a1), (b0, b1)) in cs['pairs'] for z in (px, py, a0, a1, b0, b1)]
        assert got == want and all(abs(val(v)) * 100 <= 52 * P for v in cs['vecs']), cs['name']
    for fx in (0, 1, 2):
        sub = [cs for cs in cases if cs['fixed_g2'] == fx]
        assert {fc.pairing_expected(cs)[2] for cs in sub} == {fc.BLS_OK, fc.BLS_INVALID}
        assert any(not c.g1_in_subgroup(cs['pairs'][0][0]) and not c.g2_in_subgroup(cs['pairs'][0][1]) for cs in sub if 'outside' in cs['name'])
        pos = [cs for cs in sub if 'positive representative' in cs['name']]
        neg = [cs for cs in sub if 'negative representative' in cs['name']]
        assert len(pos) == len(neg) >= 3
        for x, y in zip(pos, neg):
            assert x['pairs'] == y['pairs'] and sum(u != w for u, w in zip(x['vecs'], y['vecs'])) == 1
            assert [val(w) - val(u) for u, w in zip(x['vecs'], y['vecs']) if u != w] == [-P]
    big_p, big_q = fc.largest_g1(), fc.largest_g2()
    assert big_p[0] > P - 64 and big_q[0][0] == P - 1 and big_q[0][1] > P - 64


@pytest.mark.parametrize('fixed_g2', (0, 1, 2))
def test_miller_loop_and_final_exponentiation_on_the_host(lib, fixed_g2):
    """coop_miller2 (its point-step glue under the tracker), then coop_final_easy -- the exact Fp12 value against the oracle -- and
    coop_final_verdict, on every pair case of this fixed_g2"""
    for cs in fc.pairing_cases():
        if cs['fixed_g2'] != fixed_g2:
            continue
        flat = (ctypes.c_int32 * 168)(*[x for v in cs['vecs'] for x in v])
        out = (ctypes.c_int32 * 168)()
        assert lib.hs_coop_pairing(0, fixed_g2, flat, out) == 0
        o = list(out)
        fc.check_easy(cs, [o[14 * k:14 * (k + 1)] for k in range(12)])
        assert lib.hs_coop_pairing(1, fixed_g2, flat, out) == fc.pairing_expected(cs)[2], cs['name']
