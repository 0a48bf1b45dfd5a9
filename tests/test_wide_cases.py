"""tests/wide_cases.py without a GPU: the inputs it builds are legal operands of the row-wide engine, the aligned item of every
operation drives its widest product row to the column sums the table allows (2^61.7 of 2^62 for a (2,2) row), every operation of both
table sets is exercised, and the checker that judges the device's answers fails on a limb off by one, on a stray write and on an output
outside (-0.6 p, 0.6 p)."""
import math
import random

import pytest

import wide_cases as wc
from util import P, val, limbs_of, limbs_of_elem, NL

SA, SB, CONST = wc.SA, wc.SB, wc.CONST


@pytest.fixture(scope='module')
def runs():
    return wc.all_runs()


_cache = {}


def perfect_store(run, item, fill=0):
    """what a correct device returns: the expected elements in reduced form where the steps write, the initial words elsewhere"""
    key = (run['name'], item, fill)
    if key not in _cache:
        store = wc.initial_store(run, item, fill)
        want = wc.expected_store(run, item)
        for v in wc.written(run):
            store[v] = wc.vec16(limbs_of_elem(want[v]))
        _cache[key] = (store, want)
    store, want = _cache[key]
    return [list(v) for v in store]


def check(run, item, store, fill=0):
    perfect_store(run, item, fill)
    return wc.check(run, item, store, fill, expected=_cache[(run['name'], item, fill)][1])


def test_every_operation_is_exercised(runs):
    want = {('F12', o.name) for o in wc.g.OPS} | {('PT', o.name) for o in wc.g.OPS_PT} | {('F12', 'FPINV')}
    assert set(wc.ALL_OPS) == want and len(want) == 37 + 42 + 1
    assert wc.exercised(runs) == want
    per_op = {(r['set'], r['ops'][0]) for r in runs if len(r['steps']) == 1 and r['reps'] == 1}
    assert per_op == want, 'every operation has a run of its own'
    assert not any(st[0] in wc.HANDOVER for r in runs for st in r['steps'])


def test_every_shape_of_the_programs_is_run():
    for ts in wc.SETS.values():
        sh = wc.shapes(ts)
        used = {st[0] for prog in ts.programs.values() for st in prog} - set(wc.HANDOVER)
        assert used <= set(sh) == set(ts.by) | ({'FPINV'} if ts.name == 'F12' else set())
        for n, steps in sh.items():
            assert len(wc.op_runs(ts.name, n)) == len(steps) >= 1


def test_every_input_satisfies_the_input_contract(runs):
    for r in runs:
        fpinv = r['ops'] == ['FPINV']
        assert len(r['items']) >= 1 and len(set(r['in_idx'])) == len(r['in_idx'])
        for it in r['items']:
            assert len(it) == len(r['in_idx'])
            for v in it:
                if fpinv:           # fp_inv_var canonicalises first: limbs of up to two carries, a value of a few p (field_cases FP_INV_VAR)
                    assert v[14] == 0 and v[15] == 0 and all(abs(x) < 2**30 for x in v[:NL]) and abs(val(v[:NL])) < 3 * P
                else:
                    assert wc.in_contract(v), r['name']


def test_extremes_sit_at_the_limit():
    assert len(wc.EXTREMES) == 16
    for nm, v in wc.EXTREMES:
        assert wc.in_contract(v) and 5 * (abs(val(v[:NL])) + 2**364) >= 3 * P, nm
    lows = {x for _, v in wc.EXTREMES for x in v[:NL - 1]}
    assert lows == {wc.LIMB_HI, -wc.LIMB_HI, 8, -8} and wc.LIMB_LO == -8
    assert all(x == wc.LIMB_HI for x in wc.BIG[:NL - 1])


def test_the_aligned_item_attains_the_widest_product_row():
    """column sums on integers: the aligned item takes the chosen row to thirteen full limb products per column -- the limbs 0..12 of
    both operand sums at sum|c| (2^28 + 7), all of one sign -- which for a (2,2) row is 2^61.7; and no row of any operation passes 2^62"""
    worst = {}
    for set_name, op_name in wc.ALL_OPS:
        if op_name == 'FPINV':
            continue
        ts = wc.SETS[set_name]
        op = ts.by[op_name]
        rng = random.Random('%s %s %d' % (set_name, op_name, 1))
        for step in wc.shapes(ts)[op_name]:
            need, items = wc.op_items(ts, step, rng)
            named = dict(items)
            _, prow, _ = wc.aligned_signs(op, random.Random(0))
            for nm in ('aligned', 'aligned, negated'):
                for row in op.prods:
                    top = max(abs(x) for x in wc.product_columns(ts, step, named[nm], row))
                    assert top < 2**62, (op_name, nm)
                    worst[set_name] = max(worst.get(set_name, 0), top)
            if prow is None:
                continue
            sa, sb = (sum(abs(k) for k, _ in side) for side in prow[:2])
            apart = ts.lay.ref(step[2]) != ts.lay.ref(step[3]) or not wc.reads(op)[1]
            steerable = all((i >> 12) != CONST for side in prow[:2] for _, i in side)
            if apart and steerable:
                cols = wc.product_columns(ts, step, named['aligned'], prow)
                assert max(abs(x) for x in cols) >= 13 * sa * sb * wc.LIMB_HI**2, (op_name, step)
                if (sa, sb) == (2, 2):
                    assert 2**61 < max(abs(x) for x in cols) < 2**62, (op_name, step)
    for s, w in sorted(worst.items()):
        print('set %s: largest product column sum of the aligned items 2^%.3f' % (s, math.log2(w)))
    assert all(w > 2**61 for w in worst.values())


def test_every_set_has_a_steerable_2_2_row():
    """the 2^61.7 case exists in both sets, and in every operation that has a (2,2) row over plain operands with distinct values"""
    for ts in wc.SETS.values():
        hit = 0
        for op in ts.ops:
            _, prow, _ = wc.aligned_signs(op, random.Random(0))
            if prow and tuple(sum(abs(k) for k, _ in side) for side in prow[:2]) == (2, 2):
                hit += 1
        assert hit >= 10, ts.name


PICKS = ('MUL ', 'PDBL1 ', 'C2ADD1X4 ', 'C1ISOK ', 'FPINV ', 'Miller doubling', 'sixteen-point sum G1_JJ', 'MUL chain x2')


def picked(runs):
    out = [r for r in runs if r['name'].startswith(PICKS)]
    assert len(out) >= len(PICKS)
    return out


def test_the_checker_accepts_a_correct_store(runs):
    for r in picked(runs):
        for fill in wc.FILLS:
            for item in range(0, len(r['items']), 7):
                assert check(r, item, perfect_store(r, item, fill), fill)


def test_the_checker_fails_on_a_limb_off_by_one(runs):
    for r in picked(runs):
        for v in sorted(wc.written(r))[::5]:
            for limb in (0, 6, 13):
                for d in (1, -1):
                    store = perfect_store(r, 0)
                    store[v][limb] += d
                    with pytest.raises(AssertionError):
                        check(r, 0, store)


def test_the_checker_fails_on_a_stray_write(runs):
    for r in picked(runs):
        ts = wc.SETS[r['set']]
        wr = wc.written(r)
        outside = [v for v in range(ts.nv) if v not in wr and v not in ts.tmp]
        for v in (outside[0], outside[len(outside) // 2], outside[-1], r['in_idx'][0] if r['in_idx'][0] not in wr else outside[1], min(ts.consts)):
            for word in (0, 13, 15):
                store = perfect_store(r, 0, -1)
                store[v][word] ^= 1
                with pytest.raises(AssertionError):
                    check(r, 0, store, -1)
        store = perfect_store(r, 0)
        store[ts.tmp[0]][3] ^= 1                    # the product scratch is the engine's own
        assert check(r, 0, store)


def test_the_checker_fails_on_an_output_outside_the_range(runs):
    for r in picked(runs):
        inv = wc.last_writer_is_inv(r)
        for v in sorted(wc.written(r))[::5]:
            for k in (1, 2):
                store = perfect_store(r, 0)
                x = val(store[v][:NL])
                x += k * P if x >= 0 else -k * P        # congruent, |value| > 0.6 p
                store[v] = wc.vec16(limbs_of(x))
                with pytest.raises(AssertionError, match="0.6 p|fp_reduce"):
                    check(r, 0, store)
            store = perfect_store(r, 0)
            store[v][14] = 1
            with pytest.raises(AssertionError, match='words 14 and 15'):
                check(r, 0, store)
            if v not in inv:
                store = perfect_store(r, 0)
                store[v][3] += 9 << 28                  # the same value on a limb that no carry pass leaves
                store[v][4] -= 9
                with pytest.raises(AssertionError, match='carry-pass'):
                    check(r, 0, store)


def test_the_whole_pairing_program_ends_in_the_verdict():
    run, want_one = wc.pairing_run()
    ts = wc.SETS['F12']
    t = ts.lay.base['T']
    for item, one in enumerate(want_one):
        V = wc.expected_store(run, item)
        assert (wc.chk.unflat(V[t:t + 12]) == wc.c.F12_ONE) == one


def test_the_maximal_quotient_items_need_the_64_bit_carry_pass(runs):
    """the device's integer arithmetic of a linear row on Python integers: for the items built from QUOTIENT_PAIRS every quotient digit
    but the lowest is 2^28 - 1, the limb sums stay below 2^59 (their carry fits 32 bits) and a limb with its neighbour's carry passes 2^31
    -- w_finish must form it on 64 bits.  Both table sets have such rows."""
    seen = set()
    for r in runs:
        if len(r['steps']) != 1 or r['reps'] != 1 or r['ops'] == ['FPINV']:
            continue
        ts = wc.SETS[r['set']]
        step = r['steps'][0]
        op = ts.by[step[0]]
        for nm, it in zip(r['item_names'], r['items']):
            if not nm.startswith(('every quotient digit maximal', 'aligned')):
                continue
            m = dict(zip(r['in_idx'], it))
            worst = 0
            for row in op.lins:
                acc, qs = wc.limb_sums(ts, step, m, row)
                assert all(abs(x) < 2**59 for x in acc), (r['name'], nm)
                top = max(wc.first_pass(acc))
                if top >= 2**31:
                    assert all(q == 2**28 - 1 for q in qs[2:])
                worst = max(worst, top)
            if nm.startswith('every quotient'):
                assert worst >= 2**31, (r['name'], nm)
                seen.add(r['set'])
    assert seen == {'F12', 'PT'}
    assert len(wc.QUOTIENT_PAIRS) == 4 and all(wc.in_contract(wc.vec16(limbs_of(x))) for pr in wc.QUOTIENT_PAIRS for x in pr)
