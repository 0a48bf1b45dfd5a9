"""The shared case list of tests/field_cases.py on the CPU: every case of every operation runs through the host-compiled headers
(tests/hostsim hs_field_op; the lanes = 64 rows of the wave-cooperative engine through tests/hostsim_coop hs_coop_op, a wave as 32
threads) with the bound tracker on and the case's declared limb and value bounds, so a case that passes lies
inside the documented input contract of the function under test; the results are judged by field_cases.check (exact integers).
tests/test_gpu_field_ops.py then runs the same cases on the device.  No case is skipped: a case the tracker rejects aborts the run
and is removed from the list in the source."""
import ctypes

import pytest

import field_cases as fc
import util
from util import c, P


@pytest.fixture(scope='module')
def ops(pkg):
    return pkg.api.field_ops()


@pytest.fixture(scope='module')
def hs(hs):
    """hs_field_op of tests/hostsim and hs_coop_op of tests/hostsim_coop behind one name: run_host picks by the row's lanes"""
    hs.hs_coop_op = util.build_hostsim_coop().hs_coop_op
    return hs


def run_host(hs, ops, shapes, op, cs, reps=1):
    lanes, n_in, n_out, n_par, _ = shapes[op]
    assert len(cs['vecs']) == n_in and len(cs['par']) == n_par, (op, cs['name'])
    flat = [x for v in cs['vecs'] for x in v]
    out = (ctypes.c_int32 * (14 * n_out))()
    rc = (hs.hs_coop_op if lanes == 64 else hs.hs_field_op)(ops[op], (ctypes.c_int32 * len(flat))(*flat), (ctypes.c_double * n_in)(*cs['lb']), (ctypes.c_double * n_in)(*cs['vb']),
                        (ctypes.c_int32 * n_in)(*cs['nn']), (ctypes.c_int32 * max(n_par, 1))(*cs['par']), reps, out)
    assert rc == 0, op
    o = list(out)
    return [o[14 * k:14 * (k + 1)] for k in range(n_out)]


def header_shapes(pkg):
    """(lanes, n_in, n_out, n_par, chain) per operation from the one table of csrc/debug_ops.h, as api.field_op_table parses it"""
    return {name: row[1:] for name, row in pkg.api.field_op_table().items()}


def test_case_list_covers_every_operation(pkg, ops):
    cases = fc.build()
    assert set(cases) == set(ops) == set(header_shapes(pkg))
    for op, lst in sorted(cases.items()):
        assert len(lst) >= 4, op
        print('%-20s %4d cases' % (op, len(lst)))
    print('total %d cases' % sum(len(v) for v in cases.values()))


def test_neighbours_always_differ():
    """consecutive cases of a list are different records, the wrap-around included: however a test cuts a run of items out of a list,
    adjacent lanes and lane pairs hold different operands, so that a leak between neighbours shows"""
    for op, lst in fc.build().items():
        for i in range(len(lst)):
            a, b = lst[i], lst[(i + 1) % len(lst)]
            assert (a['vecs'], a['par']) != (b['vecs'], b['par']), '%s: cases %d "%s" and %d "%s" are the same record' % (op, i, a['name'], (i + 1) % len(lst), b['name'])


def test_shape_query_matches_the_header(pkg):
    """the library's own statement of the table (blsgpu_debug_field_op_shape: needs the built library, no device)"""
    for op, shape in header_shapes(pkg).items():
        assert pkg.api.field_op_shape(op) == shape, op


@pytest.mark.parametrize('op', sorted(fc.build()))
def test_cases_are_legal_and_right_on_the_host(pkg, hs, ops, op):
    """every case through the tracked host build: inside the contract (no abort) and right (field_cases.check)"""
    shapes = header_shapes(pkg)
    lst = fc.build()[op]
    if op == 'G2Q_DBL':          # jac_dbl_quad is DPP code with no host form: it follows jac_dbl_body's operation order and reductions, so its
        op = 'G2S_DBL'           # cases (those of G2S_DBL, unchanged) are proved legal on jac_dbl_body
        lst = [fc.with_pars(cs, first=1) for cs in fc.build()[op]]
    for cs in lst:
        fc.check(op, cs, run_host(hs, ops, shapes, op, cs))
    print('%s: %d cases' % (op, len(lst)))


@pytest.mark.parametrize('op', fc.CHAINS)
def test_chains_are_legal_and_right_on_the_host(pkg, hs, ops, op):
    """reps = 2, 17 and 63: an operation's lazy output as its own next operand; the squarings of the cyclotomic subgroup run every
    cyclotomic element of the list at every length (63: the compressed squarings of one a^x)"""
    shapes = header_shapes(pkg)
    assert shapes[op][4] == 1
    for reps, stride in fc.CHAIN_REPS:
        cases = fc.chain_cases(op, stride)
        if op == 'G2Q_DBL':      # (as above: on jac_dbl_body)
            op, cases = 'G2S_DBL', [fc.with_pars(cs, first=1) for cs in fc.chain_cases('G2S_DBL', stride)]
        for cs in cases:
            fc.check(op, cs, run_host(hs, ops, shapes, op, cs, reps), reps)


def test_compressed_squaring_formula_is_the_square_in_the_cyclotomic_subgroup():
    """the restated formulas that fix "right" for the compressed and Granger-Scott squarings agree with the oracle's plain squaring
    where they must: on elements a^((p^6 - 1)(p^2 + 1))"""
    import random
    rng = random.Random(3)
    for nm, g in fc.cyclotomic_elements(rng):
        assert c.f12_mul(g, c.f12_conj(g)) == fc.F12_ONE, nm
        sq = c.f12_sqr(g)
        assert fc.gs_sqr(g) == sq, nm
        assert fc.cyc_c_sqr(fc.compress(g)) == fc.compress(sq), nm
