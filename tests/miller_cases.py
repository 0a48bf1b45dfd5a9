"""What PRODUCES line values, restated in Python integers, and the case lists of the step, merge and row operations of
csrc/debug_ops.h (MILLER1_* on g2_hom_t<fp2>, MILLER2_* on g2_hom_t<hfp2>, LINES_MERGE*, LINE3_ROW).  field_cases.build() merges
these lists into its own, so the tracked host build (tests/test_field_cases.py) and the device tests run them like every other row.

The reference.  T = (X, Y, Z) is a homogeneous projective point of the twist y^2 = x^3 + b', b' = 4 (1 + u); Fp2 through the oracle's
f2_*.  The steps of csrc/pairing.cuh are
    doubling   l0 = Y^2 - 3b' Z^2,  g = -3 X^2,  h = 2YZ;   with B = Y^2, E = 3b' Z^2 = 12 (1 + u) Z^2, F = 3E, H = 2YZ:
               X3 = 2XY (B - F),  Y3 = (B + F)^2 - 12 E^2,  Z3 = 4BH
    addition   theta = Y - yQ Z,  lambda = X - xQ Z;  l0 = theta xQ - lambda yQ,  g = -theta,  h = lambda;
               with e = lambda^3, f = Z theta^2, g' = X lambda^2, h' = e + f - 2g':  X3 = lambda h',  Y3 = theta (g' - h') - e Y,  Z3 = Z e
and the line value at P = (xP, yP) is l0 + (g xP) w^2 + (h yP) w^3.  They are polynomials, so they define a value for ANY operands,
degenerate ones included, which lets a case choose its operands coordinate by coordinate (as tests/point_cases.py does).  The merges
are the product of two such values as polynomials in w with w^6 = xi, taken from the oracle's f12_mul.  tests/test_miller_cases.py
pins all of it to the oracle: the curve's dbl / add, the scalar [|x|]Q, the Miller value of every pair of field_cases.pairing_cases()
and the constants of csrc/g2neg_lines.cuh.

Judging is exact: every output congruent modulo p to the restated value, and in the form the code gives it -- T' of a doubling
reduced; of an addition Y3 reduced, X3 and Z3 products; l0 normalised; l2, l3 multiplier outputs; of a merged line c0, c2, c3, c5
reduced and c4 a product."""
import os
import random
import re

import util
from util import c, P, val, limbs_of, limbs_of_elem, elem_of, NL, R392

import field_cases as fc

M = util.LIMB_MASK
ZERO = [0] * NL
B3 = (12, 12)                         # 3b' = 12 (1 + u)
ADD_ENTRIES = fc.MILLER_ADD_ENTRIES
ENTRIES = fc.MILLER_ENTRIES
F2_ZERO, F2_ONE = (0, 0), (1, 0)


# ---- the reference
def dbl_step(T):
    """(T', (l0, g, h)) of a doubling step"""
    X, Y, Z = T
    B = c.f2_sqr(Y)
    E = c.f2_mul(B3, c.f2_sqr(Z))
    F = c.f2_muls(E, 3)
    H = c.f2_muls(c.f2_mul(Y, Z), 2)
    line = (c.f2_sub(B, E), c.f2_neg(c.f2_muls(c.f2_sqr(X), 3)), H)
    X3 = c.f2_mul(c.f2_muls(c.f2_mul(X, Y), 2), c.f2_sub(B, F))
    Y3 = c.f2_sub(c.f2_sqr(c.f2_add(B, F)), c.f2_muls(c.f2_sqr(E), 12))
    Z3 = c.f2_muls(c.f2_mul(B, H), 4)
    return (X3, Y3, Z3), line


def add_step(T, Q):
    """(T', (l0, g, h)) of an addition step with the affine Q = (xQ, yQ)"""
    X, Y, Z = T
    xq, yq = Q
    th = c.f2_sub(Y, c.f2_mul(yq, Z))
    la = c.f2_sub(X, c.f2_mul(xq, Z))
    line = (c.f2_sub(c.f2_mul(th, xq), c.f2_mul(la, yq)), c.f2_neg(th), la)
    la2 = c.f2_sqr(la)
    e = c.f2_mul(la, la2)
    f = c.f2_mul(Z, c.f2_sqr(th))
    g = c.f2_mul(X, la2)
    h = c.f2_sub(c.f2_add(e, f), c.f2_muls(g, 2))
    return (c.f2_mul(la, h), c.f2_sub(c.f2_mul(th, c.f2_sub(g, h)), c.f2_mul(e, Y)), c.f2_mul(Z, e)), line


def line_at(line, p):
    """(l0, l2, l3): the line (l0, g, h) evaluated at the affine P = (xP, yP) of E(Fp)"""
    return (line[0], c.f2_muls(line[1], p[0]), c.f2_muls(line[2], p[1]))


def walk(Q):
    """the 68 entries of the Miller loop on the affine Q in loop order: ([(l0, g, h)], the T it ends with)"""
    T, lines = (Q[0], Q[1], F2_ONE), []
    for e in range(ENTRIES):
        T, l = add_step(T, Q) if e in ADD_ENTRIES else dbl_step(T)
        lines.append(l)
    return lines, T


def hom_affine(T):
    """X / Z, Y / Z (None for Z = 0)"""
    if T[2] == F2_ZERO:
        return None
    zi = c.f2_inv(T[2])
    return (c.f2_mul(T[0], zi), c.f2_mul(T[1], zi))


def merge(a, b):
    """(c0, c2, c4, c3, c5) of (a0 + a2 w^2 + a3 w^3)(b0 + b2 w^2 + b3 w^3): the product has no w^1 term"""
    f = c.f12_mul(fc.line3_f12(*a), fc.line3_f12(*b))
    assert f[1] == F2_ZERO
    return (f[0], f[2], f[4], f[3], f[5])


def merge_y(a, b0, b2, y):
    """... with b3 = y in Fp"""
    return merge(a, (b0, b2, (y % P, 0)))


def merge_yy(a0, a2, ya, b0, b2, yb):
    """... with both w^3 coefficients in Fp"""
    return merge((a0, a2, (ya % P, 0)), (b0, b2, (yb % P, 0)))


def norm_row(line):
    """(l0 / h, g / h): a row of the *_LINES_N tables"""
    hi = c.f2_inv(line[2])
    return (c.f2_mul(line[0], hi), c.f2_mul(line[1], hi))


def line3_row(n0, cc, x, y):
    """the line value of a normalised row (n0, c) at P = (x, y): n0 + (c x) w^2 + y w^3"""
    return (n0, c.f2_muls(cc, x), (y % P, 0))


def pair_table(pairs):
    """the 68 merged lines (c0, c2, c4, c3, c5) of two pairs (P, Q): what k_lines2s hands to k_millerf2s, up to factors in Fp2"""
    (p0, q0), (p1, q1) = pairs
    w0, w1 = walk(q0)[0], walk(q1)[0]
    return [list(merge(line_at(a, p0), line_at(b, p1))) for a, b in zip(w0, w1)]


def g2neg_tables():
    """{name: 68 rows of Fp2 elements} parsed from csrc/g2neg_lines.cuh: three per row (l0, g, h) in *_LINES, two (l0 / h, g / h) in *_LINES_N"""
    text = open(os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc', 'g2neg_lines.cuh')).read()
    out = {}
    for m in re.finditer(r'BLS_CONST uint32_t (\w+)\[68\]\[(\d) \* FP_NL\] = \{(.*?)\n\};', text, re.S):
        name, width, body = m.group(1), int(m.group(2)), m.group(3)
        rows = []
        for row in re.findall(r'\{([^{}]*)\}', body):
            w = [int(x.rstrip('u'), 16) for x in row.split(',')]
            assert len(w) == width * NL
            rows.append([(elem_of(w[2 * k * NL:(2 * k + 1) * NL]), elem_of(w[(2 * k + 1) * NL:(2 * k + 2) * NL])) for k in range(width // 2)])
        assert len(rows) == ENTRIES
        out[name] = rows
    return out


# ---- operands as limb vectors
ROWS = {'MILLER1_DBL': ('one', 'DBL'), 'MILLER1_ADD': ('one', 'ADD'), 'MILLER2_DBL': ('split', 'DBL'), 'MILLER2_ADD': ('split', 'ADD'),
        'LINES_MERGE': ('split', 'MERGE'), 'LINES_MERGE_Y': ('split', 'MERGE_Y'), 'LINES_MERGE_YY': ('split', 'MERGE_YY'), 'LINE3_ROW': ('split', 'ROW')}
STEP_ROWS = ('MILLER1_ADD', 'MILLER1_DBL', 'MILLER2_ADD', 'MILLER2_DBL')      # par[0] = form; chains
CHAINS = STEP_ROWS
HI = [M] * (NL - 1) + [fc.TOP_MAX - 1]                  # the largest reduced top limb
LO = [0] * (NL - 1) + [fc.TOP_MIN + 1]                  # the most negative one
FP_EDGES = (0, 1, P - 1, (P - 1) // 2, (P + 1) // 2)
# What the steps take for T beside reduced values: their own outputs -- of the lane-split addition products in (-p/8, p + p/8) with
# limbs in [0, 2^28), of the one-lane addition the normalised Karatsuba differences (limbs within 16 of that range, values within
# 2.375 p).  The extreme patterns run at that limb magnitude with a top limb of 2 p.
T_MAG, T_TOP = 2**28 + 15, 2 * (P >> 364)
# a line coefficient as the steps leave it: l0 normalised (limbs within 16 of [0, 2^28), at most 3.21 p: Y^2 - E with |E| <= 4 * 0.52 p),
# l2 and l3 multiplier outputs
L0_TOP = 3 * (P >> 364)
MULT_HI = [M] * (NL - 1) + [(9 * P // 8 >> 364) - 1]
MULT_LO = [0] * (NL - 1) + [-(P // 8 >> 364)]
L0_HI = [M + 16] * (NL - 1) + [L0_TOP]
L0_LO = [-16] * (NL - 1) + [-L0_TOP]


def f2v(x):
    """an Fp2 element in the reduced internal form: two limb vectors"""
    return [limbs_of_elem(x[0]), limbs_of_elem(x[1])]


def f2m(x):
    """... as two multiplier outputs (the Montgomery residues in [0, p))"""
    return [fc.mult_form(x[0]), fc.mult_form(x[1])]


def f2_of(vs):
    return (elem_of(vs[0]), elem_of(vs[1]))


def hom_vecs(pt, z):
    """the homogeneous point (x z, y z, z) of the affine pt, reduced form"""
    return f2v(c.f2_mul(pt[0], z)) + f2v(c.f2_mul(pt[1], z)) + f2v(z)


def rand_f2(rng):
    return (rng.randrange(1, P), rng.randrange(1, P))


def _g2(rng):
    return c.E2.mul(c.G2_GEN, rng.randrange(1, c.R))


def _g1(rng):
    return c.E1.mul(c.G1_GEN, rng.randrange(1, c.R))


def _extreme_T(add):
    """(name, the six vectors of T) at the ends of what a step takes.  An addition follows a doubling, or (never in this loop) an
    addition whose Y3 is reduced: its Y keeps the reduced range in the top limb (the tracker rejects 2 p there: the one-lane
    product e Y would pass 256 p^2)."""
    out = [('T at +0.52 p', [limbs_of(fc.RED_MAX)] * 6), ('T at -0.52 p', [limbs_of(-fc.RED_MAX)] * 6),
           ('T at +-0.52 p alternating', [limbs_of(fc.RED_MAX), limbs_of(-fc.RED_MAX)] * 3),
           ('T at the largest reduced top limb', [HI] * 6), ('T at the most negative reduced top limb', [LO] * 6),
           ('T at the reduced top limbs alternating', [LO, HI] * 3)]
    ext = fc.extreme_operands(T_MAG, T_TOP)
    for i, (nm, l) in enumerate(ext):
        tv = [ext[(i + 3 * k) % len(ext)][1] for k in range(6)]
        if add:
            tv[2:4] = [v[:NL - 1] + [(fc.TOP_MAX - 1) * (1 if v[-1] > 0 else -1)] for v in tv[2:4]]
        out.append(('T ' + nm, tv))
    return out


def step_cases(kind, rng):
    """the cases of a step row, shared by the one-lane and the lane-split row (so the two layouts are also compared with each other)"""
    add = kind == 'ADD'
    E2 = c.E2
    out = []                                      # (name, T vectors, Q or None, P, chain)

    def put(name, tv, q=None, p=None, chain=False):
        if q is None:
            q = _g2(rng)
        if p is None:
            p = _g1(rng)
        qv = (f2v(q[0]) + f2v(q[1])) if not isinstance(q, list) else q
        pv = [limbs_of_elem(p[0]), limbs_of_elem(p[1])] if not isinstance(p, list) else p
        out.append((name, tv, qv, pv, chain))
    for i in range(4):
        q, t = _g2(rng), _g2(rng)
        put('T on the curve, random Z (%d)' % i, hom_vecs(t, rand_f2(rng)), q, chain=True)
    t = c.map_to_curve_g2(rand_f2(rng))
    put('T outside the subgroup, random Z', hom_vecs(t, rand_f2(rng)), chain=True)
    q = _g2(rng)
    put('T = Q, Z = 1: the first step of a walk', hom_vecs(q, F2_ONE), q, chain=True)
    put('T = 2Q, Z = 1', hom_vecs(E2.dbl(q), F2_ONE), q)
    for nm, tv in _extreme_T(add):
        put(nm, tv, chain=nm.endswith(('+0.52 p', 'top limb')))
    ql = fc.largest_g2()
    put('Q and P with the largest canonical coordinates', hom_vecs(_g2(rng), rand_f2(rng)), ql, fc.largest_g1(), chain=True)
    put('Q at the reduced top limbs, P at +-0.52 p', hom_vecs(_g2(rng), rand_f2(rng)), [HI, LO, LO, HI], [limbs_of(fc.RED_MAX), limbs_of(-fc.RED_MAX)])
    put('Q at +-0.52 p, P at the reduced top limbs', hom_vecs(_g2(rng), rand_f2(rng)), [limbs_of(-fc.RED_MAX), limbs_of(fc.RED_MAX)] * 2, [LO, HI])
    # xP, yP at the edges of Fp, as the reduced form picks them and in the other representative where there are two
    for i, x in enumerate(FP_EDGES):
        y = FP_EDGES[(i + 2) % len(FP_EDGES)]
        put('xP = %s, yP = %s' % (_edge_name(x), _edge_name(y)), hom_vecs(_g2(rng), rand_f2(rng)), None, [limbs_of_elem(x * pow(R392, -1, P)), limbs_of_elem(y * pow(R392, -1, P))])
        put('xP, yP the field elements %s, %s' % (_edge_name(y), _edge_name(x)), hom_vecs(_g2(rng), rand_f2(rng)), None, (y, x))
    # degenerate operands: the formulas are polynomials and define a value there too
    t, q = _g2(rng), _g2(rng)
    z = rand_f2(rng)
    put('Z = 0', f2v(rand_f2(rng)) + f2v(rand_f2(rng)) + [ZERO, ZERO], q, chain=True)
    put('Z = 0 as multiples of p', f2v(rand_f2(rng)) + f2v(rand_f2(rng)) + [limbs_of(P), limbs_of(-P)], q)
    put('Y = 0', f2v(rand_f2(rng)) + [ZERO, ZERO] + f2v(z), q, chain=True)
    put('X = 0', [ZERO, ZERO] + f2v(rand_f2(rng)) + f2v(z), q)
    put('T = 0', [ZERO] * 6, q)
    put('T = Q with a random Z: theta = lambda = 0', hom_vecs(q, z), q, chain=True)
    put('T = -Q with a random Z: lambda = 0', hom_vecs(E2.neg(q), z), q, chain=True)
    put('T = Q, Z = 1, and P = 0', hom_vecs(q, F2_ONE), q, (0, 0))
    put('theta = 0 alone', hom_vecs((t[0], q[1]), z), q)
    for i in range(6):
        put('random coordinates of no curve (%d)' % i, sum((f2v(rand_f2(rng)) for _ in range(3)), []), (rand_f2(rng), rand_f2(rng)), (rng.randrange(P), rng.randrange(P)))
    lst = []
    for i, (nm, tv, qv, pv, chain) in enumerate(out):
        cs = fc.case(nm, tv + (qv if add else []) + pv, (i % 2,))
        cs['chain'] = chain
        lst.append(cs)
    return lst


def _edge_name(x):
    return {0: '0', 1: '1', P - 1: 'p - 1', (P - 1) // 2: '(p - 1)/2', (P + 1) // 2: '(p + 1)/2'}[x]


def _line_forms(rng, pt, q, p, add):
    """a line value as a step leaves it, from the restated step at T = pt (affine, lifted with a random Z): l0 in the reduced form,
    l2 and l3 as multiplier outputs"""
    z = rand_f2(rng)
    T = (c.f2_mul(pt[0], z), c.f2_mul(pt[1], z), z)
    l = line_at((add_step(T, q) if add else dbl_step(T))[1], p)
    return f2v(l[0]) + f2m(l[1]) + f2m(l[2]), l


def _single(npos, k, rng):
    cs = [F2_ZERO] * npos
    cs[k] = rand_f2(rng) if k % 2 else F2_ONE
    return cs


def merge_cases(kind, rng):
    """LINES_MERGE: a0, a2, a3, b0, b2, b3;  LINES_MERGE_Y: a0, a2, a3, b0, b2, y;  LINES_MERGE_YY: a0, a2, ya, b0, b2, yb.  The w^0
    coefficients arrive normalised (of a table row: canonical), the w^2 and w^3 ones as multiplier outputs, y as a reduced value."""
    out = []
    fpv = lambda x: [limbs_of_elem(x)]
    canon = lambda x: [limbs_of(x[0] % P * R392 % P), limbs_of(x[1] % P * R392 % P)]
    na = 3 if kind != 'MERGE_YY' else 2            # Fp2 coefficients of line a before its y

    def put(name, a, b, ya=None, yb=None):
        """a, b: lists of Fp2 vector pairs (already limb vectors); ya / yb: one vector each where the row takes y in Fp"""
        vs = sum(a, []) + (ya if kind == 'MERGE_YY' else []) + sum(b, []) + (yb if kind != 'MERGE' else [])
        out.append(fc.case(name, vs))

    def rnd_a():
        return [f2v(rand_f2(rng))] + [f2m(rand_f2(rng)) for _ in range(na - 1)]

    def rnd_b():
        return ([f2v(rand_f2(rng)), f2m(rand_f2(rng)), f2m(rand_f2(rng))] if kind == 'MERGE' else [canon(rand_f2(rng)), f2m(rand_f2(rng))])
    ry = lambda: fpv(rng.randrange(P))
    # lines of the restated steps, in the forms the steps give them
    for i in range(6):
        q0, q1, p0, p1 = _g2(rng), _g2(rng), _g1(rng), _g1(rng)
        va, la = _line_forms(rng, _g2(rng), q0, p0, i % 2 == 1)
        vb, lb = _line_forms(rng, _g2(rng), q1, p1, i % 2 == 1)
        a = [va[0:2], va[2:4], va[4:6]][:na]
        if kind == 'MERGE':
            put('two %s lines (%d)' % ('chord' if i % 2 else 'tangent', i), a, [vb[0:2], vb[2:4], vb[4:6]])
        else:
            n0, cc = norm_row(walk(q1)[0][i])                      # (entry 1 is the first addition)
            put('a %s line and a normalised row (%d)' % ('chord' if i % 2 else 'tangent', i), a, [canon(n0), f2m(c.f2_muls(cc, p1[0]))], fpv(p0[1]), fpv(p1[1]))
    # the line 1 and the zero line on either side
    one_a = [f2v(F2_ONE)] + [f2v(F2_ZERO)] * (na - 1)
    zero_a = [f2v(F2_ZERO)] * na
    nb = 3 if kind == 'MERGE' else 2
    one_b = [f2v(F2_ONE)] + [f2v(F2_ZERO)] * (nb - 1)
    zero_b = [f2v(F2_ZERO)] * nb
    z1 = fpv(0)
    put('the line 1 times a line', one_a, rnd_b(), z1, ry())
    put('a line times the line 1', rnd_a(), one_b, ry(), z1)
    put('the line 1 twice', one_a, one_b, z1, z1)
    put('the zero line times a line', zero_a, rnd_b(), z1, ry())
    put('a line times the zero line', rnd_a(), zero_b, ry(), z1)
    put('the zero line twice', zero_a, zero_b, z1, z1)
    # a single non-zero coefficient in each position (the Fp positions of the _Y rows: y alone)
    for k in range(na):
        put('only a%d non-zero' % (0, 2, 3)[k], [f2v(x) for x in _single(na, k, rng)], rnd_b(), z1, ry())
    for k in range(nb):
        put('only b%d non-zero' % (0, 2, 3)[k], rnd_a(), [f2v(x) for x in _single(nb, k, rng)], ry(), z1)
    if kind == 'MERGE_YY':
        put('only ya non-zero', zero_a, rnd_b(), ry(), ry())
    if kind != 'MERGE':
        put('only yb non-zero', rnd_a(), zero_b, ry(), ry())
    # a0 + a2, a0 + a3, a2 + a3 (and the b sums) at the largest magnitude the operands' forms allow, either sign
    for sa, sb in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        l0a, ma = (L0_HI, MULT_HI) if sa > 0 else (L0_LO, MULT_LO)
        l0b, mb = (L0_HI, MULT_HI) if sb > 0 else (L0_LO, MULT_LO)
        yv = [limbs_of(sa * fc.RED_MAX)], [limbs_of(sb * fc.RED_MAX)]
        put('every coefficient at its largest magnitude, signs %+d %+d' % (sa, sb), [[l0a, l0a]] + [[ma, ma]] * (na - 1), [[l0b, l0b]] + [[mb, mb]] * (nb - 1), *yv)
        put('components at opposite ends, signs %+d %+d' % (sa, sb), [[l0a, L0_LO if sa > 0 else L0_HI]] + [[MULT_LO if sa > 0 else MULT_HI, ma]] * (na - 1),
            [[L0_LO if sb > 0 else L0_HI, l0b]] + [[mb, MULT_LO if sb > 0 else MULT_HI]] * (nb - 1), yv[1], yv[0])
    # y at the edges of Fp and of the reduced range
    if kind != 'MERGE':
        for i, x in enumerate(FP_EDGES):
            y = FP_EDGES[(i + 3) % len(FP_EDGES)]
            put('ya = %s, yb = %s' % (_edge_name(x), _edge_name(y)) if kind == 'MERGE_YY' else 'y = %s' % _edge_name(y), rnd_a(), rnd_b(), fpv(x), fpv(y))
            put('the Montgomery residues %s, %s' % (_edge_name(x), _edge_name(y)), rnd_a(), rnd_b(), fpv(x * pow(R392, -1, P)), fpv(y * pow(R392, -1, P)))
        put('y at the largest reduced top limb', rnd_a(), rnd_b(), [HI], [HI])
        put('y at the most negative reduced top limb', rnd_a(), rnd_b(), [LO], [LO])
        put('y at the reduced top limbs, opposite', rnd_a(), rnd_b(), [HI], [LO])
    for i in range(8):
        put('random lines (%d)' % i, rnd_a(), rnd_b(), ry(), ry())
    return out


def row_cases(rng):
    """LINE3_ROW: n0, c (a table row: canonical limbs), x, y (reduced)"""
    canon = lambda x: [limbs_of(x[0] % P * R392 % P), limbs_of(x[1] % P * R392 % P)]
    out = []
    tabs = g2neg_tables()
    rows = tabs['G2NEG_LINES_N'][:3] + tabs['G2NEGC_LINES_N'][-3:]
    for i, (n0, cc) in enumerate(rows):
        p = _g1(rng)
        out.append(fc.case('a row of the constant tables at a subgroup point (%d)' % i, canon(n0) + canon(cc) + [limbs_of_elem(p[0]), limbs_of_elem(p[1])]))
    for i, x in enumerate(FP_EDGES):
        y = FP_EDGES[(i + 2) % len(FP_EDGES)]
        out.append(fc.case('x = %s, y = %s' % (_edge_name(x), _edge_name(y)), canon(rand_f2(rng)) + canon(rand_f2(rng)) + [limbs_of_elem(x), limbs_of_elem(y)]))
    pl = fc.largest_g1()
    out.append(fc.case('P with the largest canonical coordinates', canon(rand_f2(rng)) + canon(rand_f2(rng)) + [limbs_of_elem(pl[0]), limbs_of_elem(pl[1])]))
    out.append(fc.case('the zero row', [ZERO] * 4 + [limbs_of_elem(rng.randrange(P)), limbs_of_elem(rng.randrange(P))]))
    out.append(fc.case('the row (p - 1, p - 1) at +-0.52 p', canon((P - 1, P - 1)) * 2 + [limbs_of(fc.RED_MAX), limbs_of(-fc.RED_MAX)]))
    out.append(fc.case('x, y at the reduced top limbs', canon(rand_f2(rng)) + canon(rand_f2(rng)) + [HI, LO]))
    out.append(fc.case('x, y at the reduced top limbs, opposite', canon(rand_f2(rng)) + canon(rand_f2(rng)) + [LO, HI]))
    for i in range(4):
        out.append(fc.case('random row (%d)' % i, canon(rand_f2(rng)) + canon(rand_f2(rng)) + [limbs_of_elem(rng.randrange(P)), limbs_of_elem(rng.randrange(P))]))
    return out


_lists = {}


def build():
    """{row: [case]}, deterministic"""
    if _lists:
        return _lists
    L = {}
    for i, kind in enumerate(('DBL', 'ADD')):
        L['MILLER1_' + kind] = L['MILLER2_' + kind] = step_cases(kind, random.Random(20261020 + i))
    for i, kind in enumerate(('MERGE', 'MERGE_Y', 'MERGE_YY')):
        L['LINES_' + kind] = merge_cases(kind, random.Random(20261030 + i))
    L['LINE3_ROW'] = row_cases(random.Random(20261040))
    _lists.update(L)
    return _lists


def chain_cases(op, stride):
    """the cases a chain runs on: those marked for it (on-curve points, the extremes, the degenerate operands) and every stride-th"""
    lst = build()[op]
    return [cs for cs in lst if cs.get('chain')] + lst[::stride][:8]


# ---- judging
def _is_reduced(o):
    return all(0 <= x <= M for x in o[:NL - 1]) and abs(val(o)) * 100 <= 52 * P


def _is_mult(o):
    return all(0 <= x <= M for x in o[:NL - 1]) and -P < 8 * val(o) < 9 * P


def _is_norm(o, vmax):
    return all(-16 <= x <= M + 16 for x in o[:NL - 1]) and abs(val(o)) <= vmax * P


# The forms, read from csrc/pairing.cuh and csrc/tower.cuh.  A multiplier output lies in (-p/8, p + p/8) with limbs in [0, 2^28).
# 'product': what fp2_mul returns -- lane-split, one multiplier output per component; one-lane (Karatsuba), c0 = t0 - t1 within 1.25 p
# and c1 = m - t0 - t1 within 2.375 p, normalised.
# l0 normalised: of a doubling Y^2 - E, Y^2 a square (one-lane: c0 a product, c1 twice a product) and E = 4 * (a reduced value);
# of an addition the difference of two products.
L0_BOUND = {('split', 'DBL'): (3.21, 3.21), ('split', 'ADD'): (1.25, 1.25), ('one', 'DBL'): (3.21, 4.34), ('one', 'ADD'): (2.5, 4.75)}


def _form(layout, form, vs):
    if form == 'reduced':
        return all(_is_reduced(v) for v in vs)
    if form == 'mult' or (form == 'product' and layout == 'split'):
        return all(_is_mult(v) for v in vs)
    assert form == 'product'
    return _is_norm(vs[0], 1.25) and _is_norm(vs[1], 2.375)


_want = {}


def expected(op, cs, reps=1):
    """the restated outputs as Fp2 elements, in the order of the output record"""
    layout, kind = ROWS[op]
    vs = cs['vecs']
    if kind in ('DBL', 'ADD'):
        T = tuple(f2_of(vs[2 * k:2 * k + 2]) for k in range(3))
        if kind == 'ADD':
            Q = (f2_of(vs[6:8]), f2_of(vs[8:10]))
        p = (elem_of(vs[-2]), elem_of(vs[-1]))
        for _ in range(reps):
            T, l = add_step(T, Q) if kind == 'ADD' else dbl_step(T)
        return list(T) + list(line_at(l, p))
    if kind == 'MERGE':
        f = [f2_of(vs[2 * k:2 * k + 2]) for k in range(6)]
        return list(merge(f[:3], f[3:]))
    if kind == 'MERGE_Y':
        f = [f2_of(vs[2 * k:2 * k + 2]) for k in range(5)]
        return list(merge_y(f[:3], f[3], f[4], elem_of(vs[10])))
    if kind == 'MERGE_YY':
        return list(merge_yy(f2_of(vs[0:2]), f2_of(vs[2:4]), elem_of(vs[4]), f2_of(vs[5:7]), f2_of(vs[7:9]), elem_of(vs[9])))
    return list(line3_row(f2_of(vs[0:2]), f2_of(vs[2:4]), elem_of(vs[4]), elem_of(vs[5])))


def check(op, cs, outs, reps=1):
    layout, kind = ROWS[op]
    tag = '%s%s, case "%s": ' % (op, ' x%d' % reps if reps > 1 else '', cs['name'])
    key = (kind, id(cs['vecs']), reps)             # the one-lane and the lane-split row share their cases, and both forms the value
    if key not in _want:
        _want[key] = expected(op, cs, reps)
    want = _want[key]
    outs = [list(o) for o in outs]
    assert len(outs) == 2 * len(want), tag + 'output count'
    if kind in ('DBL', 'ADD'):
        names = ('X3', 'Y3', 'Z3', 'l0', 'l2', 'l3')
        forms = ('reduced',) * 3 if kind == 'DBL' else ('product', 'reduced', 'product')
    elif kind == 'ROW':
        names = ('l0', 'l2', 'l3')
    else:
        names = ('c0', 'c2', 'c4', 'c3', 'c5')
    for k, w in enumerate(want):
        o = outs[2 * k:2 * k + 2]
        got = f2_of(o)
        assert got == w, tag + '%s is not congruent to the restated value (components off by %d, %d mod p)' % (names[k], (got[0] - w[0]) % P, (got[1] - w[1]) % P)
    if kind in ('DBL', 'ADD'):
        for k in range(3):
            assert _form(layout, forms[k], outs[2 * k:2 * k + 2]), tag + '%s is not a %s value: %s' % (names[k], forms[k], outs[2 * k:2 * k + 2])
        b0, b1 = L0_BOUND[(layout, kind)]
        assert _is_norm(outs[6], b0) and _is_norm(outs[7], b1), tag + 'l0 is not normalised within %s p, %s p: %s' % (b0, b1, outs[6:8])
        for k in (4, 5):
            assert _form(layout, 'mult', outs[2 * k:2 * k + 2]), tag + '%s is not a pair of multiplier outputs: %s' % (names[k], outs[2 * k:2 * k + 2])
    elif kind == 'ROW':                            # l0 = n0 and l3 = (y, 0) are copies, l2 = c x an Fp2-by-Fp product
        vs = cs['vecs']
        assert outs[0:2] == vs[0:2], tag + 'the limbs of n0 changed on the way through'
        assert _form(layout, 'mult', outs[2:4]), tag + 'l2 is not a pair of multiplier outputs: %s' % outs[2:4]
        assert outs[4] == vs[5] and outs[5] == ZERO, tag + 'l3 is not (y, 0) limb for limb'
    else:
        for k in (0, 1, 3, 4):
            assert _form(layout, 'reduced', outs[2 * k:2 * k + 2]), tag + '%s is not a reduced value: %s' % (names[k], outs[2 * k:2 * k + 2])
        assert _form(layout, 'mult', outs[4:6]), tag + 'c4 is not a plain product: %s' % outs[4:6]
