"""The lane-split tower and the field leaves ON THE DEVICE, one operation at a time (blsgpu_debug_field_op, csrc/debug_ops.h) and
k_millerf2s itself on crafted line tables (blsgpu_debug_millerf), against the integers.

The cases are the shared list of tests/field_cases.py -- tests/test_field_cases.py proves each of them legal on the host build with
the bound tracker -- and every comparison is exact: congruence modulo p against Python integers and the oracle's tower, plus the
output contracts of fp.cuh.  Shapes: 1, 2, 31, 32, 33 and 65 items (a lone lane pair, a full wave, one pair into the second
workgroup, a partly filled last one; twice that for the one-lane operations) and the whole list at once; neighbours always hold
different cases; a subset runs at both positions of a DPP quad; reps = 2, 17, 63 chain an operation onto its own output.

Of the three compiled bodies of the compressed squaring, k_finalexp2s runs CYC_C_SQR_KARA (f12_sh_cyc_c_sqr_kara_body) by default;
CYC_C_SQR is what fp12_pow_x runs (k_finalexps, the pairing-product paths), CYC_C_SQR_UNPACKED the BLS_CYC_KARA = 0 build."""
import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 31, 32, 33, 65)
ELSEWHERE = ('COOP_', 'MILLER', 'LINES_', 'LINE3_')      # the wave-cooperative engine: tests/test_gpu_coop_ops.py; the line producers: tests/test_gpu_miller_ops.py
OPS = sorted(op for op in fc.build() if not op.startswith(ELSEWHERE))

def run(api, op, cases, reps=1):
    return api.debug_field_op(op, [(cs['vecs'], cs['par']) for cs in cases], reps)


def take(lst, n, start):
    """n consecutive cases of the list from `start` on, cyclically: neighbours differ, because consecutive cases of every list do,
    the wrap-around included (tests/test_field_cases.py test_neighbours_always_differ)"""
    return [lst[(start + i) % len(lst)] for i in range(n)]


@pytest.mark.parametrize('op', OPS)
def test_whole_list(api, op):
    """the bulk: every case of the operation in one call (a few hundred items for the field and Fp2 operations)"""
    lst = fc.build()[op]
    outs = run(api, op, lst)
    assert len(outs) == len(lst)
    for cs, o in zip(lst, outs):
        fc.check(op, cs, o)


@pytest.mark.parametrize('op', OPS)
def test_item_counts(api, op):
    """1, 2, 31, 32, 33, 65 items (lane pairs; the one-lane operations also at twice that: 62 .. 130 lanes of 64-lane workgroups)"""
    lst = fc.build()[op]
    lanes = api.field_op_shape(op)[0]
    counts = COUNTS if lanes != 1 else COUNTS + (62, 64, 66, 130)        # (lane pairs and, for G2Q_DBL, quads)
    for k, n in enumerate(counts):
        cases = take(lst, n, 7 * k)
        outs = run(api, op, cases)
        assert len(outs) == n
        for cs, o in zip(cases, outs):
            fc.check(op, cs, o)


@pytest.mark.parametrize('op', [op for op in OPS if op.startswith(('FP2_', 'F12_', 'CYC_', 'G2S_', 'G2Q_')) and not op.startswith('FP2_KARA')])
def test_both_quad_positions(api, op):
    """the same cases at an even and at an odd pair index -- both positions of a DPP quad -- give identical limbs: a quad_perm that
    reaches the wrong partner, or anything leaking between neighbours, shows here (and in check() at either position); for G2Q_DBL the
    two runs put a case at an even and at an odd quad index"""
    lst = fc.build()[op]
    sub = take(lst, min(len(lst), 21), 3)
    even = run(api, op, sub)
    odd = run(api, op, [lst[0]] + sub)[1:]
    for cs, a, b in zip(sub, even, odd):
        fc.check(op, cs, a)
        assert a == b, '%s, case "%s": the result depends on the position in the quad' % (op, cs['name'])


@pytest.mark.parametrize('op', [op for op in fc.CHAINS if not op.startswith(ELSEWHERE)])
def test_chains(api, op):
    """reps = 2, 17, 63: the lazy output of an operation as its own next operand.  The squarings of the cyclotomic subgroup run every
    cyclotomic element of the list at every length: 63 compressed squarings are those of one a^x"""
    for reps, stride in fc.CHAIN_REPS:
        cases = fc.chain_cases(op, stride)
        outs = run(api, op, cases, reps)
        for cs, o in zip(cases, outs):
            fc.check(op, cs, o, reps)


def run_miller(api, picks, status=None):
    tables = fc.miller_tables()
    return api.debug_millerf([fc.miller_table_vecs(tables[i][1]) for i in picks], status)


@pytest.mark.parametrize('n', COUNTS)
def test_millerf_kernel_on_line_tables(api, n):
    """k_millerf2s, the shipped kernel (f12_sh_sqr_fn, f12_sh_mul_line5_fn with line5_ld, the packed accumulator), on line tables no
    signature can produce: all lines 1, one special entry at entries 0, 1, 2, 51, 67, the zero line, single coefficients, random tables.
    Expected value from the oracle's tower with the embedding of tower.cuh fp12_from_line5 (field_cases.line5_f12)."""
    tables = fc.miller_tables()
    picks = [(5 * n + i) % len(tables) for i in range(n)]
    outs = run_miller(api, picks)
    assert len(outs) == n
    for i, o in zip(picks, outs):
        fc.check_miller(tables[i][0], tables[i][1], o)


def test_millerf_every_table(api):
    tables = fc.miller_tables()
    outs = run_miller(api, range(len(tables)))
    for (nm, t), o in zip(tables, outs):
        fc.check_miller(nm, t, o)


def test_millerf_flagged_items_next_to_live_ones(api):
    """items whose status is not OK -- item 0, the last one, and one inside a quad next to a live item -- are skipped; their live
    neighbours are exact (the flagged slots are not compared)"""
    tables = fc.miller_tables()
    n = 33
    picks = [(i + 2) % len(tables) for i in range(n)]
    flagged = {0, 5, 18, n - 1}
    status = [1 if i in flagged else 0 for i in range(n)]
    outs = run_miller(api, picks, status)
    for j, (i, o) in enumerate(zip(picks, outs)):
        if j not in flagged:
            fc.check_miller(tables[i][0] + ' (item %d beside flagged items)' % j, tables[i][1], o)
