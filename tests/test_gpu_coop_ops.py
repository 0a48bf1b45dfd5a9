"""The wave-cooperative pairing engine (csrc/coop.cuh) ON THE DEVICE: its round functions one at a time through the COOP_* rows of
csrc/debug_ops.h (blsgpu_debug_field_op: one item per 64-lane workgroup on a coop_shared overwritten with a fill word first), and the
shipped kernels k_pairing_coop_easy, k_pairing_coop and k_finalexp_coop on crafted operands (blsgpu_debug_coop_pairing).

The cases are the lists of tests/field_cases.py -- tests/test_field_cases.py and tests/test_hostsim_coop.py prove each of them legal
on the host build of the same source with the bound tracker -- and every expected value comes from Python integers and the oracle's
tower: congruence modulo p plus the output contract of the function (limbs in [0, 2^28) and |value| <= 0.52 p after fp2_reduce).
Shapes: 1, 2, 3, 33 and 65 workgroups with different cases in neighbouring ones, and the whole list in one call."""
import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 33, 65)
PAIR_COUNTS = (1, 2, 33, 65)
OPS = sorted(op for op in fc.build() if op.startswith('COOP_'))
OK = fc.BLS_OK


def run(api, op, cases, reps=1):
    return api.debug_field_op(op, [(cs['vecs'], cs['par']) for cs in cases], reps)


def take(lst, n, start):
    """n consecutive cases from `start` on, cyclically: neighbours hold different operands (field_cases._cycle_pars asserts it)"""
    return [lst[(start + i) % len(lst)] for i in range(n)]


def check_all(op, cases, outs, reps=1):
    assert len(outs) == len(cases)
    for cs, o in zip(cases, outs):
        fc.check(op, cs, o, reps)


@pytest.mark.parametrize('op', OPS)
def test_whole_list(api, op):
    lst = fc.build()[op]
    check_all(op, lst, run(api, op, lst))


@pytest.mark.parametrize('op', OPS)
def test_item_counts(api, op):
    lst = fc.build()[op]
    for k, n in enumerate(COUNTS):
        cases = take(lst, n, 7 * k)
        check_all(op, cases, run(api, op, cases))


@pytest.mark.parametrize('op', [op for op in fc.CHAINS if op.startswith('COOP_')])
def test_chains(api, op):
    """reps = 2, 17, 63: a round's reduced output as its own next operand; coop_cyc_sqr on every cyclotomic element at every length
    (63 squarings are those of one a^x), coop_mul and coop_cyc_sqr feeding each other inside COOP_POW_X and COOP_FINAL_VERDICT"""
    for reps, stride in fc.CHAIN_REPS:
        cases = fc.chain_cases(op, stride)
        check_all(op, cases, run(api, op, cases, reps), reps)


@pytest.mark.parametrize('op', sorted(fc.COOP_ALIASES))
def test_alias_modes(api, op):
    """dst apart, dst = a, and for coop_mul dst = b -- all three occur in coop_final_verdict: the whole list and a chain in each mode"""
    lst = fc.build()[op]
    for alias in fc.COOP_ALIASES[op]:
        cases = [fc.with_pars(cs, first=alias) for cs in lst]
        check_all(op, cases, run(api, op, cases))
        chain = [fc.with_pars(cs, first=alias) for cs in fc.chain_cases(op, 5)]
        check_all(op, chain, run(api, op, chain, 17), 17)


@pytest.mark.parametrize('op', OPS)
def test_fills(api, op):
    """the whole list with coop_shared pre-filled with 0, 0xffffffff and 0x7fffffff: every output right each time, and the same limbs --
    nothing depends on what LDS held.  (COOP_JOBS returns the fill in the slots it must not compute: check() demands exactly that.)"""
    lst = fc.build()[op]
    outs = []
    for fill in fc.FILLS:
        cases = [fc.with_pars(cs, fill=fill) for cs in lst]
        outs.append(run(api, op, cases))
        check_all(op, cases, outs[-1])
    if op != 'COOP_JOBS':
        for cs, a, b, d in zip(lst, *outs):
            assert a == b == d, '%s, case "%s": the result depends on the fill' % (op, cs['name'])


# ---- the shipped kernels on crafted pairs
def pair_cases(fixed_g2):
    return [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == fixed_g2]


@pytest.mark.parametrize('fixed_g2', (0, 1, 2))
def test_easy_part_of_the_shipped_kernel(api, fixed_g2):
    """k_pairing_coop_easy: the exported value is miller_loop(pairs)^((p^6 - 1)(p^2 + 1)) of the oracle, exactly, at 1, 2, 33 and 65
    items (the list cycles) -- subgroup points, the largest coordinates, points outside the subgroups, both representatives"""
    lst = pair_cases(fixed_g2)
    for k, n in enumerate(PAIR_COUNTS):
        cases = take(lst, n, 3 * k)
        outs = api.debug_coop_pairing(0, fixed_g2, [cs['vecs'] for cs in cases])
        assert len(outs) == n
        for cs, o in zip(cases, outs):
            fc.check_easy(cs, o)


@pytest.mark.parametrize('fixed_g2', (0, 1, 2))
def test_verdict_of_the_shipped_kernel(api, fixed_g2):
    """k_pairing_coop: OK exactly where the oracle's pairing product is one"""
    lst = pair_cases(fixed_g2)
    for k, n in enumerate(PAIR_COUNTS):
        cases = take(lst, n, 5 * k + 1)
        got = api.debug_coop_pairing(1, fixed_g2, [cs['vecs'] for cs in cases])
        want = [fc.pairing_expected(cs)[2] for cs in cases]
        assert got == want, [cs['name'] for cs, g, w in zip(cases, got, want) if g != w]


def test_finalexp_coop_on_crafted_values(api):
    """k_finalexp_coop (the single-verdict tail) on the COOP_FINAL_VERDICT operands: r-th powers, Fp6, +-1, zero, random"""
    lst = fc.build()['COOP_FINAL_VERDICT']
    for k, n in enumerate(PAIR_COUNTS):
        cases = take(lst, n, 4 * k)
        got = api.debug_coop_pairing(2, 0, [cs['vecs'] for cs in cases])
        want = [fc.final_verdict(fc.f12_of_vecs(cs['vecs'])) for cs in cases]
        assert got == want, [cs['name'] for cs, g, w in zip(cases, got, want) if g != w]


@pytest.mark.parametrize('fixed_g2', (0, 1, 2))
def test_flagged_items_beside_live_ones(api, fixed_g2):
    """items that are not OK on entry -- the first, one in the middle, the last -- are skipped: their status stays, their easy-part
    slot still holds the sentinel the door pre-filled, and the live items beside them are exact"""
    lst = pair_cases(fixed_g2)
    n = 9
    cases = take(lst, n, 2)
    flagged = {0, 4, n - 1}
    status = [7 if i in flagged else OK for i in range(n)]
    outs = api.debug_coop_pairing(0, fixed_g2, [cs['vecs'] for cs in cases], status)
    for i, (cs, o) in enumerate(zip(cases, outs)):
        if i in flagged:
            assert all(x == api.COOP_SENTINEL for v in o for x in v), 'item %d was flagged and its easy-part slot was written' % i
        else:
            fc.check_easy(cs, o)
    got = api.debug_coop_pairing(1, fixed_g2, [cs['vecs'] for cs in cases], status)
    assert got == [7 if i in flagged else fc.pairing_expected(cs)[2] for i, cs in enumerate(cases)]
    if fixed_g2 == 0:
        vals = take(fc.build()['COOP_FINAL_VERDICT'], n, 1)
        got = api.debug_coop_pairing(2, 0, [cs['vecs'] for cs in vals], status)
        assert got == [7 if i in flagged else fc.final_verdict(fc.f12_of_vecs(cs['vecs'])) for i, cs in enumerate(vals)]
