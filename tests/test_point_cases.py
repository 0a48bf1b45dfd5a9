"""What tests/point_cases.py claims about its own lists, on the CPU: the reference is the oracle's group law wherever the operands lie
on the curve, every run of consecutive adder cases holds every branch, the crafted Fp2 operands hit one component of h or rr at a time,
and the small-order points have the order they are named for."""
import random

import field_cases as fc
import point_cases as pc
from util import c, P, val

CURVES = (c.E1, c.E2)


def test_reference_is_the_oracle_group_law_on_the_curve():
    """chord and tangent with a = 0 equals Curve.add on every adder and doubling case whose operands lie on the curve"""
    n = 0
    for op in pc.ADDER_ROWS + ['G1_DBL', 'G2L_DBL']:
        E, _, kind = pc.ROWS[op]
        for cs in fc.build()[op]:
            if kind == 'DBL':
                p = pc.affine(E, pc.parse_jac(E, cs['vecs'][:3 * E.k]))
                p, q = p, p
            else:
                p, q = pc.operands(op, cs)
            if E.on_curve(p) and E.on_curve(q):
                assert pc.ct_add(E, p, q) == E.add(p, q), (op, cs['name'])
                n += 1
    assert n > 200
    rng = random.Random(5)
    for E in CURVES:
        for _ in range(20):
            p, q = pc.curve_point(E, rng), pc.curve_point(E, rng)
            assert pc.ct_add(E, p, q) == E.add(p, q) and pc.ct_add(E, p, p) == E.dbl(p) and pc.ct_add(E, p, E.neg(p)) is None


def test_every_run_of_adder_cases_holds_every_branch():
    """any five (mixed addition: four) consecutive cases, cyclically, are one of each branch class: every cut of a list puts all
    branches into one wave"""
    for op in pc.ADDER_ROWS:
        E, _, kind = pc.ROWS[op]
        lst, classes = fc.build()[op], pc.CLASSES[kind]
        for cs in lst:
            assert cs['cls'] == pc.branch_class(*pc.operands(op, cs)), (op, cs['name'])
        for i in range(len(lst)):
            assert {lst[(i + j) % len(lst)]['cls'] for j in range(len(classes))} == set(classes), (op, i)
        for must in ('Z = p', 'jac_neg', 'v - p', 'two Z representatives', 'small order', 'chain'):
            assert any(must in cs['name'] for cs in lst), (op, must)


def test_crafted_fp2_operands_hit_one_component_at_a_time():
    """after the cross-multiplication (u = X Z'^2, s = Y Z'^3) the named component of h = u2 - u1 or rr = s2 - s1 is zero and the other
    is not -- the input that tells a lane-split fe_is_zero that combines both lanes from one that looks at its own"""
    E = c.E2
    for op in ('G2L_ADD', 'G2L_MADD'):
        seen = set()
        for cs in fc.build()[op]:
            if 'after the cross-multiplication' not in cs['name']:
                continue
            (X1, Y1, Z1) = pc.parse_jac(E, cs['vecs'][:6])
            if op == 'G2L_ADD':
                (X2, Y2, Z2) = pc.parse_jac(E, cs['vecs'][6:12])
            else:
                X2, Y2, Z2 = pc.felem(E, cs['vecs'][6:8]), pc.felem(E, cs['vecs'][8:10]), (1, 0)
            z1z1, z2z2 = c.f2_sqr(Z1), c.f2_sqr(Z2)
            h = c.f2_sub(c.f2_mul(X2, z1z1), c.f2_mul(X1, z2z2))
            rr = c.f2_sub(c.f2_mul(Y2, c.f2_mul(z1z1, Z1)), c.f2_mul(Y1, c.f2_mul(z2z2, Z2)))
            nm = cs['name']
            if nm.startswith('x agree in c0 only'):
                assert h[0] == 0 and h[1] != 0 and cs['cls'] == 'generic'
            elif nm.startswith('x agree in c1 only'):
                assert h[1] == 0 and h[0] != 0 and cs['cls'] == 'generic'
            elif nm.startswith('x equal, y differ in c0 only'):
                assert h == (0, 0) and rr[0] != 0 and rr[1] == 0 and cs['cls'] == 'cancelling'
            elif nm.startswith('x equal, y differ in c1 only'):
                assert h == (0, 0) and rr[1] != 0 and rr[0] == 0 and cs['cls'] == 'cancelling'
            if 'y equal' in nm:
                assert rr == (0, 0)
            seen.add(nm)
        assert len(seen) == 12, (op, sorted(seen))


def test_small_order_points():
    """(0, 2) has order 3 on E1; the E2 point has the small prime order q, a factor of the cofactor h2 = #E'(Fp2) / r"""
    rng = random.Random(9)
    assert c.E1.on_curve(pc.G1_LOW) and c.E1.mul(pc.G1_LOW, 3) is None and pc.low_order(c.E1) == (3, pc.G1_LOW)
    for _ in range(3):
        assert c.E2.mul(pc.curve_point(c.E2, rng), c.R * pc.H2) is None          # r h2 is the group order
    q, T = pc.low_order(c.E2)
    assert pc.H2 % q == 0 and all(q % d for d in range(2, q)) and q < 100
    assert c.E2.on_curve(T) and T is not None and c.E2.mul(T, q) is None
    assert not c.g2_in_subgroup(T) and not c.g1_in_subgroup(pc.G1_LOW)


def test_ladders_meet_their_own_exceptional_steps_on_the_small_order_point():
    """[3] (0, 2) cancels in the middle of the ladder and [5] (0, 2) takes the doubling branch there"""
    E, T = c.E1, pc.G1_LOW
    acc = E.dbl(T)
    assert pc.branch_class(acc, T) == 'cancelling'                    # k = 3 = 0b11: after the doubling, 2T + T
    acc = E.dbl(E.dbl(T))
    assert pc.branch_class(acc, T) == 'doubling'                      # k = 5 = 0b101: 4T = T, then T + T
    for op in ('G1_MUL_U64', 'G1_MUL_SCALAR'):
        ks = {pc.scalar_of(cs['par']) for cs in fc.build()[op] if 'order 3' in cs['name']}
        assert {3, 5, 6, 7} <= ks


def test_subgroup_lists_hold_both_verdicts():
    for op in ('G1_IN_SUBGROUP', 'G2L_IN_SUBGROUP'):
        verdicts = [pc._expected(op, cs, 1)[0] for cs in fc.build()[op]]
        assert verdicts.count(True) >= 8 and verdicts.count(False) >= 8, op


def test_no_curve_point_separates_the_y_comparison_of_the_g2_subgroup_test():
    """g2_in_subgroup compares x(psi P) with x([x] P) and then y.  Equal x-coordinates mean psi(P) = +-[x] P; psi(P) = -[x] P puts P
    into the kernel of psi + x, an endomorphism of degree x^2 + t x + p (psi^2 - t psi + p = 0, t = x + 1), which is coprime to the
    group order r h2: E'(Fp2) holds no such point but the identity.  So on points of the curve -- all that g2_decompress hands the
    function -- the y comparison cannot change a verdict, and no case of G2L_IN_SUBGROUP can tell it from a comparison of x alone."""
    from math import gcd
    assert gcd(2 * c.X * c.X + c.X + P, c.R * pc.H2) == 1


def test_zero_spellings_have_non_zero_limbs():
    for E in CURVES:
        for nm, vs in pc.identities(E, random.Random(1)):
            z = vs[2 * E.k:]
            assert all(val(v) % P == 0 for v in z), nm
            if 'p' in nm.split('Z =')[-1]:
                assert any(any(v) for v in z), nm
