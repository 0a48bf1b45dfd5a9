"""What tests/miller_cases.py claims about its restatement of the Miller steps, on the CPU: pinned to the oracle's curve, its Miller
loop and the constants of csrc/g2neg_lines.cuh, so that a wrong formula copied into the restatement cannot pass for right."""
import random

import field_cases as fc
import miller_cases as mc
from util import c, P

E2 = c.E2


def on_curve_step_cases():
    """(row, case, T affine, Q) of the step cases whose operands lie on the twist"""
    out = []
    for op in ('MILLER1_DBL', 'MILLER1_ADD'):
        for cs in fc.build()[op]:
            vs = cs['vecs']
            t = mc.hom_affine(tuple(mc.f2_of(vs[2 * k:2 * k + 2]) for k in range(3)))
            q = (mc.f2_of(vs[6:8]), mc.f2_of(vs[8:10])) if op.endswith('ADD') else t
            if t is not None and E2.on_curve(t) and E2.on_curve(q):
                out.append((op, cs, t, q))
    return out


def test_steps_are_the_oracle_group_law_on_the_curve():
    """after X / Z, Y / Z the restated doubling is Curve.dbl and the restated addition Curve.add, on every on-curve case of the lists
    (T = +-Q excepted: the chord formula is not the group law there) and on random points"""
    n = 0
    for op, cs, t, q in on_curve_step_cases():
        want = mc.expected(op, cs)
        if op.endswith('DBL'):
            assert mc.hom_affine(tuple(want[:3])) == E2.dbl(t), cs['name']
            n += 1
        elif t[0] != q[0]:
            assert mc.hom_affine(tuple(want[:3])) == E2.add(t, q), cs['name']
            n += 1
    assert n >= 16
    rng = random.Random(7)
    for _ in range(10):
        t, q, z = mc._g2(rng), mc._g2(rng), mc.rand_f2(rng)
        T = (c.f2_mul(t[0], z), c.f2_mul(t[1], z), z)
        assert mc.hom_affine(mc.dbl_step(T)[0]) == E2.dbl(t)
        assert mc.hom_affine(mc.add_step(T, q)[0]) == E2.add(t, q)


def test_lines_vanish_where_they_must():
    """the tangent at T vanishes at T, the chord through T and Q at both and at -(T + Q): the line is l0 + g x + h y on the twist"""
    rng = random.Random(8)
    at = lambda l, pt: c.f2_add(l[0], c.f2_add(c.f2_mul(l[1], pt[0]), c.f2_mul(l[2], pt[1])))
    for _ in range(5):
        t, q, z = mc._g2(rng), mc._g2(rng), mc.rand_f2(rng)
        T = (c.f2_mul(t[0], z), c.f2_mul(t[1], z), z)
        ld, la = mc.dbl_step(T)[1], mc.add_step(T, q)[1]
        assert at(ld, t) == (0, 0) and at(ld, E2.neg(E2.dbl(t))) == (0, 0) and at(ld, q) != (0, 0)
        assert at(la, t) == (0, 0) and at(la, q) == (0, 0) and at(la, E2.neg(E2.add(t, q))) == (0, 0)


def walk_points():
    """every G2 argument of the case lists"""
    qs = []
    for cs in fc.pairing_cases():
        for _, q in cs['pairs']:
            if q not in qs:
                qs.append(q)
    return qs


def test_the_walk_ends_at_x_times_q():
    qs = [q for q in walk_points() if fc.miller_walk_is_regular(q)]
    assert len(qs) >= 6
    for q in qs:
        lines, T = mc.walk(q)
        assert len(lines) == mc.ENTRIES
        assert mc.hom_affine(T) == E2.mul(q, c.X_ABS)


def test_restated_lines_give_the_oracle_miller_value():
    """the merged lines of the restated walks, squared and multiplied as field_cases.miller_expected orders them, then conjugated: the
    easy part equals that of the oracle's Miller loop for every entry of field_cases.pairing_cases() (the Fp2 factors by which the
    projective lines differ from the oracle's affine ones vanish under p^6 - 1)"""
    tables = [mc.pair_table(cs['pairs']) for cs in fc.pairing_cases()]      # all alive at once: miller_expected caches by id(table)
    for cs, table in zip(fc.pairing_cases(), tables):
        assert fc.cyclotomic(fc.miller_expected(table)) == fc.pairing_expected(cs)[1], cs['name']


def test_constant_tables_are_the_restated_walks():
    """all 68 rows of the four tables of csrc/g2neg_lines.cuh: (l0, g, h) of the restated walks of -g2 and -[c] g2, and their
    normalised rows (l0 / h, g / h)"""
    tabs = mc.g2neg_tables()
    assert set(tabs) == {'G2NEG_LINES', 'G2NEGC_LINES', 'G2NEG_LINES_N', 'G2NEGC_LINES_N'}
    for name, q in (('G2NEG', E2.neg(c.G2_GEN)), ('G2NEGC', fc.g2_negc())):
        lines, _ = mc.walk(q)
        for e, l in enumerate(lines):
            assert list(l) == tabs[name + '_LINES'][e], (name, e)
            assert list(mc.norm_row(l)) == tabs[name + '_LINES_N'][e], (name, e)


def test_the_y_merges_are_the_merge_with_y_embedded():
    rng = random.Random(9)
    r2 = lambda: mc.rand_f2(rng)
    for _ in range(10):
        a, b, ya, yb = (r2(), r2(), r2()), (r2(), r2()), rng.randrange(P), rng.randrange(P)
        assert mc.merge_y(a, b[0], b[1], yb) == mc.merge(a, (b[0], b[1], (yb, 0)))
        assert mc.merge_yy(a[0], a[1], ya, b[0], b[1], yb) == mc.merge((a[0], a[1], (ya, 0)), (b[0], b[1], (yb, 0)))
    # ... and the merge is the five coefficients the comments of tower.cuh lines_merge state
    a, b = (r2(), r2(), r2()), (r2(), r2(), r2())
    mul, add = c.f2_mul, c.f2_add
    want = (add(mul(a[0], b[0]), c.f2_mul_xi(mul(a[2], b[2]))), add(mul(a[0], b[1]), mul(a[1], b[0])), mul(a[1], b[1]),
            add(mul(a[0], b[2]), mul(a[2], b[0])), add(mul(a[1], b[2]), mul(a[2], b[1])))
    assert mc.merge(a, b) == want
    assert fc.line5_f12(*want) == c.f12_mul(fc.line3_f12(*a), fc.line3_f12(*b))


def test_row_evaluation_is_the_normalised_line():
    """n0 + (c x) w^2 + y w^3 is the line value divided by h yP ... times yP: line_at / h"""
    rng = random.Random(10)
    q, p = mc._g2(rng), mc._g1(rng)
    for l in mc.walk(q)[0][:6]:
        hi = c.f2_inv(l[2])
        assert mc.line3_row(*mc.norm_row(l), p[0], p[1]) == (c.f2_mul(l[0], hi), c.f2_muls(c.f2_mul(l[1], hi), p[0]), (p[1], 0))


def test_new_lists_have_their_families_and_neighbours_differ():
    L = mc.build()
    assert set(L) == set(mc.ROWS)
    for op, lst in L.items():
        for i in range(len(lst)):
            a, b = lst[i], lst[(i + 1) % len(lst)]
            assert a['vecs'] != b['vecs'], '%s: cases %d "%s" and %d "%s" hold the same operands' % (op, i, a['name'], (i + 1) % len(lst), b['name'])
    for op in mc.STEP_ROWS:
        names = [cs['name'] for cs in L[op]]
        for must in ('random Z', '0.52 p', 'top limb', 'limbs negative', 'limbs alternating', 'xP = 0', 'p - 1', '(p + 1)/2', 'Z = 0', 'Y = 0', 'T = Q', 'T = -Q'):
            assert any(must in nm for nm in names), (op, must)
        assert {cs['par'][0] for cs in L[op]} == {0, 1}
        assert sum(bool(cs['chain']) for cs in L[op]) >= 10
    for op in ('LINES_MERGE', 'LINES_MERGE_Y', 'LINES_MERGE_YY'):
        names = [cs['name'] for cs in L[op]]
        for must in ('the line 1 times', 'times the line 1', 'the zero line times', 'times the zero line', 'only a0', 'only b2', 'largest magnitude', 'opposite ends'):
            assert any(must in nm for nm in names), (op, must)
    for op in ('LINES_MERGE_Y', 'LINES_MERGE_YY'):
        names = [cs['name'] for cs in L[op]]
        for e in ('0', '1', 'p - 1', '(p - 1)/2', '(p + 1)/2'):
            assert any(('y = %s' % e) in nm or ('yb = %s' % e) in nm for nm in names), (op, e)
