"""The curve layer ON THE DEVICE, one operation at a time (the G1_*, G2L_*, G2S_* and G2Q_DBL rows of csrc/debug_ops.h).  The whole
lists, the item counts, both quad positions and the chains run in tests/test_gpu_field_ops.py with every other row; here are the shapes
that are about the branches of the adders: a wave whose neighbours each take another branch, both forms of a function (the non-inlined
one and its body), and the two Fp2 layouts against each other.  Cases and judging: tests/point_cases.py, exact."""
import pytest

import field_cases as fc
import point_cases as pc

pytestmark = pytest.mark.gpu


def run(api, op, cases, reps=1):
    return api.debug_field_op(op, [(cs['vecs'], cs['par']) for cs in cases], reps)


@pytest.mark.parametrize('op', pc.ADDER_ROWS)
def test_every_branch_in_every_wave(api, op):
    """64 + 1 items cycling the branch classes (generic, doubling, cancelling, identity left, identity right): each wave holds every
    branch side by side, and the last item sits alone in the second workgroup (for the lane-split rows: item 32 opens it, item 64 the
    third).  Every item is checked."""
    lst = fc.build()[op]
    ncls = len(pc.CLASSES[pc.ROWS[op][2]])
    cases = [lst[(i + 7) % len(lst)] for i in range(65)]
    for i in range(65 - ncls + 1):
        assert len({cs['cls'] for cs in cases[i:i + ncls]}) == ncls
    outs = run(api, op, cases)
    assert len(outs) == 65
    for cs, o in zip(cases, outs):
        fc.check(op, cs, o)


@pytest.mark.parametrize('op', pc.FORM_ROWS)
def test_both_forms_give_the_same_limbs(api, op):
    """par[0] = 0 runs the non-inlined function (jac_dbl, jac_add, jac_madd), 1 its body as the kernels inline it: identical limbs on
    every case of the list"""
    lst = fc.build()[op]
    outs = [run(api, op, [fc.with_pars(cs, first=form) for cs in lst]) for form in (0, 1)]
    for cs, a, b in zip(lst, *outs):
        fc.check(op, cs, a)
        assert a == b, '%s, case "%s": the function and its body differ' % (op, cs['name'])


@pytest.mark.parametrize('kind', ('DBL', 'ADD', 'MADD', 'PSI', 'PSI2', 'CLEAR'))
def test_the_two_fp2_layouts_agree(api, kind):
    """the one-lane and the lane-split row on the same cases: the same point (both identities, or the same affine coordinates)"""
    E = pc.c.E2
    lst = fc.build()['G2L_' + kind]
    assert fc.build()['G2S_' + kind] is lst
    one, split = run(api, 'G2L_' + kind, lst), run(api, 'G2S_' + kind, lst)
    for cs, a, b in zip(lst, one, split):
        fc.check('G2L_' + kind, cs, a)
        fc.check('G2S_' + kind, cs, b)
        ja, jb = pc.parse_jac(E, a), pc.parse_jac(E, b)
        assert pc.affine(E, ja) == pc.affine(E, jb), '%s, case "%s": the layouts disagree' % (kind, cs['name'])
