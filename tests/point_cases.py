"""Case lists of the curve-layer rows of csrc/debug_ops.h (G1_*: jac<fp>, G2L_*: jac<fp2>, G2S_*: jac<hfp2>, G2Q_DBL: jac_dbl_quad) and
what "right" means for them.  field_cases.build() merges these lists into its own, so the machinery of tests/test_field_cases.py (the
tracked host build) and of the device tests runs them like every other row.

The reference.  The adders and the doubling never use the curve constant b, so "right" is the affine chord-and-tangent rule with
a = 0 over Python integers (Fp2 through the oracle's f2_*), after de-homogenising each operand by X / Z^2, Y / Z^3:
    chord   lambda = (y2 - y1) / (x2 - x1),   tangent  lambda = 3 x^2 / (2 y),   x3 = lambda^2 - x1 - x2,   y3 = lambda (x1 - x3) - y1,
the identity for a vertical chord or tangent.  It is defined for ANY coordinates, on the curve or not, which lets a case choose its
operands coordinate by coordinate; tests/test_point_cases.py asserts that it is the oracle's Curve.add on every on-curve case.
Everything else is judged by the oracle itself: Curve.mul, g2_psi, g2_clear_cofactor, multiplication by r for the subgroup verdicts.

The comparison is exact: the output is the identity (Z = 0 mod p) exactly when the expected point is; otherwise X / Z^2 and Y / Z^3
equal the expected affine coordinates; every coordinate has the output form its branch gives it (a value reduction, a product); a
branch that copies an operand through returns that operand's limbs."""
import random

import util
from util import c, P, val, limbs_of, limbs_of_elem, elem_of, NL, R392

M = util.LIMB_MASK
ZERO = [0] * NL
ONE = limbs_of(R392 % P)              # fp_one: the constant FP_ONE, R mod p in exact limbs
R = c.R

# row -> (curve, layout, kind).  layout: how a product leaves the field layer (g1 / g2s: multiplier outputs per vector; g2l: the
# one-lane Karatsuba fp2_mul, normalised differences of products)
ROWS = {}
for _g, _E, _lay in (('G1', c.E1, 'g1'), ('G2L', c.E2, 'g2l')):
    for _k in ('DBL', 'ADD', 'MADD', 'TO_AFF', 'MUL_U64', 'MUL_SCALAR', 'IN_SUBGROUP'):
        ROWS['%s_%s' % (_g, _k)] = (_E, _lay, _k)
for _lay, _g in (('g2l', 'G2L'), ('g2s', 'G2S')):
    for _k in ('PSI', 'PSI2', 'CLEAR'):
        ROWS['%s_%s' % (_g, _k)] = (c.E2, _lay, _k)
for _k in ('DBL', 'ADD', 'MADD'):
    ROWS['G2S_' + _k] = (c.E2, 'g2s', _k)
ROWS['G2Q_DBL'] = (c.E2, 'g2s', 'DBL')
FORM_ROWS = sorted(op for op, (_, _, k) in ROWS.items() if k in ('DBL', 'ADD', 'MADD') and op != 'G2Q_DBL')     # par[0] = form
ADDER_ROWS = sorted(op for op, (_, _, k) in ROWS.items() if k in ('ADD', 'MADD'))
CHAINS = tuple(sorted(FORM_ROWS + ['G2Q_DBL']))
# the branches of jac_add_body; jac_madd_body has no "identity right": its second operand is affine and never the identity
CLASSES = {'ADD': ('generic', 'doubling', 'cancelling', 'identity left', 'identity right'),
           'MADD': ('generic', 'doubling', 'cancelling', 'identity left')}


# ---- field elements of either curve as limb vectors
def fvecs(E, x):
    """the reduced internal form: one vector over Fp, two (c0, c1) over Fp2"""
    return [limbs_of_elem(x)] if E.k == 1 else [limbs_of_elem(x[0]), limbs_of_elem(x[1])]


def felem(E, vs):
    return elem_of(vs[0]) if E.k == 1 else (elem_of(vs[0]), elem_of(vs[1]))


def one(E):
    return 1 if E.k == 1 else (1, 0)


def rand_elem(E, rng):
    return rng.randrange(1, P) if E.k == 1 else (rng.randrange(1, P), rng.randrange(1, P))


def gen(E):
    return c.G1_GEN if E.k == 1 else c.G2_GEN


def rand_point(E, rng):
    """a random point of the prime-order subgroup"""
    return E.mul(gen(E), rng.randrange(1, R))


def curve_point(E, rng):
    """a random point of the whole curve E(Fp) / E'(Fp2)"""
    while True:
        x = rand_elem(E, rng)
        y2 = E.rhs(x)
        if E.k == 1 and c.fp_is_square(y2):
            return (x, c.fp_sqrt(y2))
        if E.k == 2 and c.f2_is_square(y2):
            return (x, c.f2_sqrt(y2))


def jac_of(E, pt, z):
    z2 = E.sqr_(z)
    return (E.mul_(pt[0], z2), E.mul_(pt[1], E.mul_(z2, z)), z)


def jvecs(E, J):
    return fvecs(E, J[0]) + fvecs(E, J[1]) + fvecs(E, J[2])


def parse_jac(E, vs):
    w = E.k
    return tuple(felem(E, vs[i * w:(i + 1) * w]) for i in range(3))


def affine(E, J):
    if J[2] == E.zero:
        return None
    zi = E.inv_(J[2])
    zi2 = E.sqr_(zi)
    return (E.mul_(J[0], zi2), E.mul_(J[1], E.mul_(zi2, zi)))


# ---- the reference
def ct_add(E, p1, p2):
    """chord and tangent with a = 0 on affine coordinates (None: the identity), for any coordinates"""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if y1 != y2 or y1 == E.zero:
            return None
        lam = E.mul_(E.muls_(E.sqr_(x1), 3), E.inv_(E.muls_(y1, 2)))
    else:
        lam = E.mul_(E.sub_(y2, y1), E.inv_(E.sub_(x2, x1)))
    x3 = E.sub_(E.sub_(E.sqr_(lam), x1), x2)
    return (x3, E.sub_(E.mul_(lam, E.sub_(x1, x3)), y1))


def branch_class(p1, p2):
    """the branch the adders take on the affine operands"""
    if p1 is None:
        return 'identity left'
    if p2 is None:
        return 'identity right'
    if p1[0] == p2[0]:
        return 'doubling' if p1[1] == p2[1] else 'cancelling'
    return 'generic'


def operands(op, cs):
    """(p, q) of an adder case, affine"""
    E, _, kind = ROWS[op]
    w = E.k
    p = affine(E, parse_jac(E, cs['vecs'][:3 * w]))
    if kind == 'ADD':
        return p, affine(E, parse_jac(E, cs['vecs'][3 * w:6 * w]))
    return p, (felem(E, cs['vecs'][3 * w:4 * w]), felem(E, cs['vecs'][4 * w:5 * w]))


def scalar_of(par):
    return sum((w & 0xffffffff) << (32 * i) for i, w in enumerate(par))


def scalar_words(k, n):
    out = []
    for i in range(n):
        w = (k >> (32 * i)) & 0xffffffff
        out.append(w - 2**32 if w & 0x80000000 else w)
    return out


# ---- points of small order
H2 = (c.X**8 - 4 * c.X**7 + 5 * c.X**6 - 4 * c.X**4 + 6 * c.X**3 - 4 * c.X**2 - 4 * c.X + 13) // 9      # #E'(Fp2) / r
G1_LOW = (0, 2)                       # on y^2 = x^3 + 4, of order 3: phi(P) = (beta 0, 2) = P
_low = {}


def small_factor(n):
    """the smallest prime factor of n, by trial division"""
    q = 2
    while n % q:
        q += 1
    return q


def point_of_order(E, q, n, rng):
    """a point of prime order q, from the group order n: [n / q^e] (a curve point) has q-power order, and is multiplied by q until
    the next multiple is the identity"""
    m = n
    while m % q == 0:
        m //= q
    while True:
        T = E.mul(curve_point(E, rng), m)
        while T is not None and E.mul(T, q) is not None:
            T = E.mul(T, q)
        if T is not None:
            return T


def low_order(E):
    """(q, T): a point of small prime order q outside the prime-order subgroup -- (0, 2) of order 3 on E1; on E2 a point of order q
    for the smallest prime factor q of the cofactor h2 = #E'(Fp2) / r, found by trial division"""
    if E.k not in _low:
        if E.k == 1:
            _low[1] = (3, G1_LOW)
        else:
            q = small_factor(H2)
            _low[2] = (q, point_of_order(E, q, R * H2, random.Random(13)))
    return _low[E.k]


def torsion(E, rng):
    """[r] (a curve point): a random point of the cofactor subgroup"""
    T = None
    while T is None:
        T = E.mul(curve_point(E, rng), R)
    return T


# ---- operand spellings
def identities(E, rng):
    """(name, the vectors X, Y, Z) of the identity: (1, 1, 0) as jac_set_inf writes it, random X and Y over Z = 0, and Z a non-zero
    multiple of p in exact limbs (non-zero limbs, zero value: fe_is_zero must go through fp_canon)"""
    rx, ry = rand_elem(E, rng), rand_elem(E, rng)
    zp = [limbs_of(P)] if E.k == 1 else [limbs_of(P), limbs_of(-P)]
    zm = [limbs_of(-P)] if E.k == 1 else [ZERO, limbs_of(P)]
    w = E.k
    return [('the identity (1, 1, 0)', fvecs(E, one(E)) * 2 + [ZERO] * w),
            ('the identity (X, Y, 0)', fvecs(E, rx) + fvecs(E, ry) + [ZERO] * w),
            ('the identity (X, Y, Z = p)', fvecs(E, ry) + fvecs(E, rx) + zp),
            ('the identity (1, 1, Z = a multiple of p in one component)', fvecs(E, one(E)) * 2 + zm)]


def raw_points(E, rng, n):
    """(name, X, Y, Z vectors) whose coordinates are the edges of the reduced range (field_cases.reduced_values), Z not zero: points of
    no curve, judged by the chord-and-tangent rule"""
    import field_cases as fc
    red = [(nm, l) for nm, l in fc.reduced_values(rng, 0) if val(l) % P]
    out, w = [], E.k
    for i in range(n):
        pick = [red[(5 * i + 3 * j + 1) % len(red)] for j in range(3 * w)]
        out.append(('coordinates at ' + ' | '.join(nm for nm, _ in pick[:3]) + ' ...', [l for _, l in pick]))
    return out


def neg_y(E, vs, limbwise=False):
    """the negative of a Jacobian point: Y as the reduced form of -y, or negated limb by limb as jac_neg leaves it"""
    w = E.k
    y = [[-x for x in v] for v in vs[w:2 * w]] if limbwise else fvecs(E, E.neg_(felem(E, vs[w:2 * w])))
    return vs[:w] + y + vs[2 * w:]


def two_reps(E, x):
    """the same field element in two exact-limb forms more than p / 2 apart: its Montgomery residue v in [0, 7 p / 8) and v - p"""
    def reps(a):
        v = a % P * R392 % P
        return limbs_of(v), limbs_of(v - P)
    if E.k == 1:
        a, b = reps(x)
        return [a], [b]
    (a0, b0), (a1, b1) = reps(x[0]), reps(x[1])
    return [a0, b1], [b0, a1]


def _point_with_small_residues(E, rng):
    """a subgroup point whose x has Montgomery residues below 7 p / 8 in every component: then a product congruent to x (in
    (-p / 8, p + p / 8)) is never the form v - p, and h = 0 is reached on unequal limb vectors"""
    while True:
        pt = rand_point(E, rng)
        xs = [pt[0]] if E.k == 1 else list(pt[0])
        if all(8 * (x * R392 % P) < 7 * P for x in xs):
            return pt


def _interleave(kind, bins):
    """round-robin over the branch classes: any len(classes) consecutive cases of the list, cyclically, hold every class -- however a
    test cuts a run of items out of the list, each wave holds every branch"""
    classes = CLASSES[kind]
    n = max(len(bins[k]) for k in classes)
    out = []
    for i in range(n):
        for k in classes:
            out.append(bins[k][i % len(bins[k])])
    return out


def adder_cases(op, rng):
    import field_cases as fc
    E, _, kind = ROWS[op]
    w = E.k
    cands = []                                    # (name, p vectors, q vectors (Jacobian), chain)
    o = one(E)

    def J(pt, z=None):
        return jvecs(E, jac_of(E, pt, o if z is None else z))
    rz = lambda: rand_elem(E, rng)
    A, B, C_, D = (rand_point(E, rng) for _ in range(4))
    # generic sums
    cands += [('P + Q, Z = 1', J(A), J(B)), ('P + Q, random Z on the left', J(B, rz()), J(C_)), ('P + Q, random Z on the right', J(C_), J(D, rz())),
              ('P + Q, random Z on both sides', J(D, rz()), J(A, rz())), ('P + 2P', J(A, rz()), J(E.dbl(A), rz())),
              ('a point of small order plus a subgroup point', J(low_order(E)[1], rz()), J(B, rz()))]
    raws = raw_points(E, rng, 10)
    for i in range(0, 10, 2):
        cands.append(('%s + %s' % (raws[i][0], raws[i + 1][0]), raws[i][1], raws[i + 1][1]))
    # the same point twice
    z1 = rz()
    cands += [('P + P, the same representative', J(A, z1), J(A, z1)), ('P + P, Z = 1', J(B), J(B)), ('P + P, two Z representatives', J(C_, rz()), J(C_, rz())),
              ('P + P, Z = 1 on the right', J(D, rz()), J(D)), ('Q + Q: a chain that starts with a doubling', J(A, rz()), J(A), True),
              ('T + T for T of small order', J(low_order(E)[1], rz()), J(low_order(E)[1]))]
    for i in range(3):
        S = _point_with_small_residues(E, rng)
        xa, xb = two_reps(E, S[0])
        yv, zv = fvecs(E, S[1]), fvecs(E, o)
        cands.append(('P + P, x as v - p on the left and v on the right (%d)' % i, xb + yv + zv, xa + yv + zv))
        ya, yb = two_reps(E, S[1])
        cands.append(('P + P, x and y as v - p on the left (%d)' % i, xb + yb + zv, xa + ya + zv))
        cands.append(('P - P, x as v - p on the left (%d)' % i, xb + yv + zv, xa + fvecs(E, E.neg_(S[1])) + zv))
    cands.append(('%s twice' % raws[0][0], raws[0][1], raws[0][1]))
    # a point and its negative
    z1 = rz()
    pa = J(A, z1)
    cands += [('P - P, the same representative', pa, neg_y(E, pa)), ('P - P, Z = 1', J(B), neg_y(E, J(B))), ('-P + P, two Z representatives', neg_y(E, J(C_, rz())), J(C_, rz())),
              ('P + jac_neg(P): Y negated limb by limb', J(D, z1), neg_y(E, J(D, z1), True)),
              ('-Q + Q: a chain through the identity and the copy', neg_y(E, J(B, rz())), J(B), True),
              ('T - T for T of small order', J(low_order(E)[1], rz()), neg_y(E, J(low_order(E)[1])))]
    # the identity on either side
    ids = identities(E, rng)
    for i, (nm, iv) in enumerate(ids):
        q = J((A, B, C_, D)[i], rz() if i % 2 else None)
        cands.append(('%s + Q' % nm, iv, q, i == 0))
        cands.append(('P + %s' % nm, J((B, C_, D, A)[i], None if i % 2 else rz()), iv))
        cands.append(('%s + %s' % (nm, ids[(i + 1) % len(ids)][0]), iv, ids[(i + 1) % len(ids)][1]))
    cands.append(('%s + %s' % (ids[0][0], raws[2][0]), ids[0][1], raws[2][1]))
    # Fp2: the components of h and rr zero one at a time -- operands of no curve, chosen after the cross-multiplication
    if w == 2:
        for zs in ('Z = 1', 'random Z'):
            za, zb = (o, o) if zs == 'Z = 1' else (rz(), o if kind == 'MADD' else rz())
            wx = c.f2_sqr(c.f2_mul(za, zb))                   # u2 - u1 = (x2 - x1) (Z1 Z2)^2
            wy = c.f2_mul(wx, c.f2_mul(za, zb))               # s2 - s1 = (y2 - y1) (Z1 Z2)^3
            for nm, dx, dy in (('x agree in c0 only', (0, 1), None), ('x agree in c1 only', (1, 0), None),
                               ('x equal, y differ in c0 only', None, (1, 0)), ('x equal, y differ in c1 only', None, (0, 1)),
                               ('x agree in c0 only, y equal', (0, 1), (0, 0)), ('x agree in c1 only, y equal', (1, 0), (0, 0))):
                t = rng.randrange(1, P)
                x1, y1 = rz(), rz()
                ddx = (0, 0) if dx is None else c.f2_mul((dx[0] * t, dx[1] * t), c.f2_inv(wx))
                ddy = rz() if dy is None else c.f2_mul((dy[0] * t % P, dy[1] * t % P), c.f2_inv(wy))
                cands.append(('%s after the cross-multiplication, %s' % (nm, zs), J((x1, y1), za), J((c.f2_add(x1, ddx), c.f2_add(y1, ddy)), zb)))
    # bin by the branch the reference takes, then interleave
    bins = {k: [] for k in CLASSES[kind]}
    for i, cand in enumerate(cands):
        nm, pv, qv = cand[:3]
        if kind == 'MADD':
            qa = affine(E, parse_jac(E, qv))
            if qa is None:
                continue                          # the affine operand of a mixed addition is never the identity
            if val(qv[2 * w]) != val(ONE) or any(val(v) for v in qv[2 * w + 1:]):       # not Z = 1: hand over the affine point
                qv = fvecs(E, qa[0]) + fvecs(E, qa[1])
            else:
                qv = qv[:2 * w]
        cs = fc.case(nm, pv + qv, (0,))
        cs['chain'] = len(cand) > 3 and cand[3]
        p, q = operands(op, cs)
        cs['cls'] = branch_class(p, q)
        bins[cs['cls']].append(cs)
    lst = _interleave(kind, bins)
    return [dict(cs, par=[i % 2]) for i, cs in enumerate(lst)]          # both forms alternate along the list (tests run either on all)


def dbl_cases(E, rng):
    import field_cases as fc
    w, o = E.k, one(E)
    rz = lambda: rand_elem(E, rng)
    out = []
    for i in range(4):
        A = rand_point(E, rng)
        out.append(('2P, Z = 1 (%d)' % i, jvecs(E, jac_of(E, A, o))))
        out.append(('2P, random Z (%d)' % i, jvecs(E, jac_of(E, A, rz()))))
    out += identities(E, rng)
    y0 = [[ZERO], [limbs_of(P)]] if w == 1 else [[ZERO, ZERO], [limbs_of(P), limbs_of(-P)], [ZERO, limbs_of(P)]]
    for i, yv in enumerate(y0):
        out.append(('Y = 0 mod p (%d): the identity' % i, fvecs(E, rz()) + yv + fvecs(E, rz())))
    out.append(('X = 0', [ZERO] * w + fvecs(E, rz()) + fvecs(E, rz())))
    out.append(('X = 0 as a multiple of p', ([limbs_of(P)] if w == 1 else [limbs_of(-P), limbs_of(P)]) + fvecs(E, rz()) + fvecs(E, o)))
    q, T = low_order(E)
    out.append(('a point of order %d' % q, jvecs(E, jac_of(E, T, rz()))))
    out.append(('the point (0, 2) of E1' if w == 1 else 'a point outside the subgroup', jvecs(E, jac_of(E, G1_LOW if w == 1 else curve_point(E, rng), o))))
    out += raw_points(E, rng, 8)
    lst = []
    for i, (nm, vs) in enumerate(out):
        cs = fc.case(nm, vs, (i % 2,))
        cs['chain'] = 'identity' in nm or i < 2
        lst.append(cs)
    return lst


def scalars(bits):
    xs = [0, 1, 2, 3, 5, 6, 7, R - 1, R, R + 1, 2**255, 2**256 - 1, c.X_ABS, 2**64 - 1] + [1 << b for b in (31, 32, 63, 64, 127, 128, 255)]
    rng = random.Random(77)
    xs += [rng.randrange(2**bits) for _ in range(3)]
    seen, out = set(), []
    for k in xs:
        k %= 2**bits
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def mul_cases(E, rng, bits):
    import field_cases as fc
    q, T = low_order(E)
    S, U = rand_point(E, rng), rand_point(E, rng)
    ids = identities(E, rng)
    out = []
    for i, k in enumerate(scalars(bits)):
        ops = [('a subgroup point', jvecs(E, jac_of(E, S if i % 2 else U, rand_elem(E, rng)))), ids[i % len(ids)],
               ('a point of order %d' % q, jvecs(E, jac_of(E, T, rand_elem(E, rng) if i % 3 else one(E))))]
        for nm, vs in ops:
            out.append(fc.case('[%#x] %s' % (k, nm), vs, scalar_words(k, bits // 32)))
    return out


def subgroup_cases(E, rng):
    import field_cases as fc
    q, T = low_order(E)
    g = gen(E)
    tor = torsion(E, rng)
    pts = [('g', g), ('[2] g', E.dbl(g)), ('[r - 1] g', E.neg(g)), ('[x] g', E.mul(g, c.X_ABS))] + [('[k] g (%d)' % i, rand_point(E, rng)) for i in range(3)]
    pts += [('[r] R: a point of the cofactor subgroup', tor), ('[k] g + [r] R', E.add(rand_point(E, rng), tor)), ('a random curve point', curve_point(E, rng)),
            ('a point of order %d' % q, T), ('[k] g + a point of order %d' % q, E.add(rand_point(E, rng), T)),
            ('g + a point of order %d' % q, E.add(g, T))]
    if q > 3:
        pts.append(('twice the point of order %d' % q, E.dbl(T)))
    if E.k == 1:
        h1 = c.H1
        q2 = small_factor(h1 // 3)
        T2 = point_of_order(E, q2, R * h1, rng)
        pts += [('a point of order %d' % q2, T2), ('[k] g + a point of order %d' % q2, E.add(rand_point(E, rng), T2))]
    out = []
    for nm, pt in pts:
        for sgn, pp in (('', pt), (', -y', E.neg(pt))):
            out.append(fc.case(nm + sgn, fvecs(E, pp[0]) + fvecs(E, pp[1]), (0,)))
    out.insert(3, fc.case('the identity flag over (0, 0)', [ZERO] * (2 * E.k), (1,)))
    out.insert(9, fc.case('the identity flag over a point outside the subgroup', fvecs(E, T[0]) + fvecs(E, T[1]), (1,)))
    return out


def g2_jac_cases(rng, clear):
    """Jacobian inputs of psi, psi^2 and clear_cofactor: inside and outside G2, Z = 1 and random, the identity"""
    import field_cases as fc
    E = c.E2
    q, T = low_order(E)
    out = []
    pts = [('g2', c.G2_GEN), ('a subgroup point', rand_point(E, rng)), ('a curve point outside G2', curve_point(E, rng)), ('another curve point outside G2', curve_point(E, rng)),
           ('a point of the cofactor subgroup', torsion(E, rng)), ('a point of order %d' % q, T), ('a map_to_curve output', c.map_to_curve_g2((rng.randrange(P), rng.randrange(P))))]
    for nm, pt in pts:
        out.append(fc.case(nm + ', Z = 1', jvecs(E, jac_of(E, pt, one(E)))))
        out.append(fc.case(nm + ', random Z', jvecs(E, jac_of(E, pt, rand_elem(E, rng)))))
    ids = identities(E, rng)
    for i, (nm, vs) in enumerate(ids):
        out.insert(3 * i + 1, fc.case(nm, vs))
    return out


_lists = {}


def build():
    """{row: [case]}, deterministic"""
    if _lists:
        return _lists
    L = {}
    for op in ADDER_ROWS:
        if op.startswith('G2S_'):
            continue
        L[op] = adder_cases(op, random.Random(hash_seed(op)))
    for g, E in (('G1', c.E1), ('G2L', c.E2)):
        rng = random.Random(hash_seed(g))
        L[g + '_DBL'] = dbl_cases(E, rng)
        import field_cases as fc
        L[g + '_TO_AFF'] = [fc.case(cs['name'], cs['vecs']) for cs in L[g + '_DBL']]
        L[g + '_MUL_U64'] = mul_cases(E, rng, 64)
        L[g + '_MUL_SCALAR'] = mul_cases(E, rng, 256)
        L[g + '_IN_SUBGROUP'] = subgroup_cases(E, rng)
    # the lane-split rows run the one-lane rows' cases: the same operands, so the two layouts are also compared with each other
    for k in ('DBL', 'ADD', 'MADD'):
        L['G2S_' + k] = L['G2L_' + k]
    L['G2Q_DBL'] = [dict(cs, par=[]) for cs in L['G2S_DBL']]
    rng = random.Random(hash_seed('psi'))
    L['G2L_PSI'] = L['G2S_PSI'] = L['G2L_PSI2'] = L['G2S_PSI2'] = g2_jac_cases(rng, False)
    L['G2L_CLEAR'] = L['G2S_CLEAR'] = L['G2L_PSI']
    _lists.update(L)
    return _lists


def hash_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) + 20261020


def chain_cases(op, stride):
    """the cases a chain runs on: those marked for it (the identity in every spelling, -Q + Q, Q + Q) and every stride-th of the list"""
    lst = build()[op]
    return [cs for cs in lst if cs.get('chain')] + lst[::stride][:12]


# ---- judging
def _is_reduced(o):
    return all(0 <= x <= M for x in o[:NL - 1]) and abs(val(o)) * 100 <= 52 * P


def _is_mult(o):
    return all(0 <= x <= M for x in o[:NL - 1]) and -P < 8 * val(o) < 9 * P


def _is_norm(o, vmax):
    return all(-16 <= x <= M + 16 for x in o[:NL - 1]) and abs(val(o)) <= vmax * P


def _form_ok(layout, form, vs):
    """one coordinate (its one or two vectors) in the form the code gives it: 'reduced' (fe_reduce), 'product' (fe_mul: a multiplier
    output per vector; the one-lane Karatsuba fp2_mul returns c0 = t0 - t1 within 2.25 p and c1 = m - t0 - t1 within 3.375 p,
    normalised), 'any' (either, or an operand copied through, or one of these negated limb by limb by jac_neg)"""
    if form == 'reduced':
        return all(_is_reduced(v) for v in vs)
    if form == 'product' and layout != 'g2l':
        return all(_is_mult(v) for v in vs)
    if form == 'product':
        return _is_norm(vs[0], 2.25) and _is_norm(vs[1], 3.375)
    return all(_is_norm(v, 3.375) or _is_norm([-x for x in v], 3.375) for v in vs)      # (jac_neg negates Y limb by limb)


_want = {}


def _expected(op, cs, reps):
    """(the expected affine point or None, the branch of the last step or None)"""
    E, layout, kind = ROWS[op]
    w = E.k
    vs = cs['vecs']
    if kind == 'DBL':
        p = affine(E, parse_jac(E, vs[:3 * w]))
        for _ in range(reps):
            p = ct_add(E, p, p)
        return p, None
    if kind in ('ADD', 'MADD'):
        p, q = operands(op, cs)
        cls = None
        for _ in range(reps):
            cls = branch_class(p, q)
            p = ct_add(E, p, q)
        return p, cls
    if kind == 'TO_AFF':
        return affine(E, parse_jac(E, vs[:3 * w])), None
    if kind in ('MUL_U64', 'MUL_SCALAR'):
        return E.mul(affine(E, parse_jac(E, vs[:3 * w])), scalar_of(cs['par'])), None
    if kind == 'IN_SUBGROUP':
        pt = (felem(E, vs[:w]), felem(E, vs[w:2 * w]))
        return (cs['par'][0] != 0 or E.mul(pt, R) is None), None
    p = affine(E, parse_jac(E, vs[:3 * w]))
    if kind == 'PSI':
        return c.g2_psi(p), None
    if kind == 'PSI2':
        return c.g2_psi(c.g2_psi(p)), None
    return (None if p is None else c.g2_clear_cofactor(p)), None


def check(op, cs, outs, reps=1):
    E, layout, kind = ROWS[op]
    w = E.k
    tag = '%s%s, case "%s": ' % (op, ' x%d' % reps if reps > 1 else '', cs['name'])
    key = (op if op != 'G2Q_DBL' else 'G2S_DBL', id(cs['vecs']), tuple(cs['par'][1:] if kind in ('DBL', 'ADD', 'MADD') else cs['par']), reps)
    if key not in _want:
        _want[key] = _expected(op, cs, reps)
    want, cls = _want[key]
    outs = [list(o) for o in outs]

    def same_point(vs, what=''):
        J = parse_jac(E, vs)
        if want is None:
            assert J[2] == E.zero, tag + what + 'the sum is the identity, Z is not zero mod p'
        else:
            assert J[2] != E.zero, tag + what + 'the identity (Z = 0 mod p) instead of a point'
            got = affine(E, J)
            assert got[0] == want[0], tag + what + 'X / Z^2 differs'
            assert got[1] == want[1], tag + what + 'Y / Z^3 differs'

    def forms(vs, fs, what=''):
        for k, f in enumerate(fs):
            assert _form_ok(layout, f, vs[k * w:(k + 1) * w]), tag + what + 'coordinate %s is not a %s value: %s' % ('XYZ'[k], f, vs[k * w:(k + 1) * w])

    if kind == 'DBL':
        assert len(outs) == (6 if op == 'G2Q_DBL' else 3) * w, tag + 'output count'
        same_point(outs[:3 * w])
        forms(outs[:3 * w], ('reduced',) * 3)                 # jac_dbl_body ends every coordinate in fe_reduce
        if op == 'G2Q_DBL':
            assert outs[3 * w:] == outs[:3 * w], tag + 'lane pair 1 holds other limbs than lane pair 0'
        return
    if kind in ('ADD', 'MADD'):
        assert len(outs) == 3 * w, tag + 'output count'
        same_point(outs)
        pv, qv = cs['vecs'][:3 * w], cs['vecs'][3 * w:]
        if cls == 'generic':                                  # add-2007-bl: X3, Y3 reduced, Z3 = ((Z1 + Z2)^2 - Z1Z1 - Z2Z2) H; madd: Z3 = 2 Z1 H reduced
            forms(outs, ('reduced', 'reduced', 'product' if kind == 'ADD' else 'reduced'))
        elif cls == 'doubling':
            forms(outs, ('reduced',) * 3)
        elif cls == 'identity left':                          # the second operand copied through
            if kind == 'ADD':
                assert outs == qv, tag + 'the limbs of q changed on the way through'
            else:
                assert outs[:2 * w] == qv and outs[2 * w:] == [ONE] + [ZERO] * (w - 1), tag + 'not (x2, y2, 1) limb for limb'
        elif cls == 'identity right' and reps == 1:
            assert outs == pv, tag + 'the limbs of p changed on the way through'
        else:
            forms(outs, ('any',) * 3)
        return
    if kind == 'TO_AFF':
        assert len(outs) == 2 * w + 1, tag + 'output count'
        assert outs[2 * w] == [int(want is None)] + [0] * (NL - 1), tag + 'the inf flag: %s' % outs[2 * w]
        if want is None:
            assert all(o == ZERO for o in outs[:2 * w]), tag + 'x, y of the identity are not zero'
        else:
            assert felem(E, outs[:w]) == want[0] and felem(E, outs[w:2 * w]) == want[1], tag + 'affine coordinates differ'
            forms(outs[:2 * w], ('product', 'product'))
        return
    if kind == 'IN_SUBGROUP':
        assert outs == [[int(want)] + [0] * (NL - 1)], tag + 'verdict %s, multiplication by r says %d' % (outs[0], want)
        return
    assert len(outs) == 3 * w, tag + 'output count'
    same_point(outs)
    if kind == 'PSI':                                         # (conj X cx, conj Y cy, conj Z): two products; Z's c1 negated limb by limb
        forms(outs, ('product', 'product'))
        zin = cs['vecs'][4:6]
        assert outs[4] == zin[0] and outs[5] == [-x for x in zin[1]], tag + 'Z is not conj(Z) limb for limb'
    elif kind == 'PSI2':                                      # (X cx2, Y cy2, Z): fp2_mul_fp, a multiplier output per vector; Z copied
        assert all(_is_mult(o) for o in outs[:4]), tag + 'X, Y are not multiplier outputs'
        assert outs[4:] == cs['vecs'][4:6], tag + 'the limbs of Z changed'
    else:
        forms(outs, ('any',) * 3)
