"""ONE case list per operation of csrc/debug_ops.h, and what "right" means for each.

tests/test_field_cases.py runs every case through the host-compiled headers with the bound tracker on (hs_field_op: a case the
tracker accepts lies inside the function's documented input contract) and tests/test_gpu_field_ops.py runs the very same cases
through the device door blsgpu_debug_field_op.  Both judge the outputs with check() below: exact integer arithmetic -- congruence
modulo p against Python integers and the oracle's tower, plus the output contracts fp.cuh states -- and no tolerance.

A case: {'name', 'vecs': [limb vectors], 'par': [integers], 'lb' / 'vb' / 'nn': the declared bounds per vector for the tracker}.
Limb vectors are the internal form (util.limbs_of): the integer v they sum to stands for the field element v / 2^392."""
import random

import util
from util import c, P, val, limbs_of, limbs_of_elem, elem_of, NL, R392, R392_INV

M = util.LIMB_MASK
TOWER_TO_W = [0, 2, 4, 1, 3, 5]       # record slot (c0.a0, c0.a1, c0.a2, c1.a0, c1.a1, c1.a2) -> power of w
RED_MAX = 52 * P // 100               # fp_reduce's output range: |value| * 100 <= 52 p
TOP_UNIT = 1 << 364                   # the top limb's unit, p / 106,514
# the top limbs at the two ends of that range: what the 20-bit packed field of sh_st_fp / sh_ld_fp has to carry
TOP_MAX = RED_MAX >> 364
TOP_MIN = -((RED_MAX >> 364) + 1)
LIN2_PAIRS = ((3, 2), (3, -2), (1, 1), (12, 0), (1, -12), (-3, 5))   # the coefficient pairs the device door compiles (tu_debug_ops1.hip)


# ---- generators (promoted from tests/test_hostsim.py)
def scramble(l, spread, rng):
    """the same integer in redundant limbs: multiples of 2^28 moved between neighbours"""
    l = list(l)
    for i in range(NL - 1):
        d = rng.randint(-spread, spread)
        l[i] += d << 28
        l[i + 1] -= d
    return l


def lazy(v, spread, rng):
    """redundant signed limbs of the integer v"""
    l = scramble(limbs_of(v), spread, rng)
    assert val(l) == v
    return l


def pattern(mag, signs, top):
    """limbs 0..12 of magnitude mag with the given sign pattern, and the top limb"""
    return [mag * signs[i % len(signs)] for i in range(NL - 1)] + [top]


def case(name, vecs, par=(), nn=None):
    vecs = [list(v) for v in vecs]
    for v in vecs:
        assert len(v) == NL and all(-2**31 <= x < 2**31 for x in v), name
    if nn is None:
        nn = [all(0 <= x <= M for x in v[:NL - 1]) and abs(v[-1]) < 2**20 for v in vecs]
    return {'name': name, 'vecs': vecs, 'par': list(par), 'lb': [float(max(abs(x) for x in v) + 1) for v in vecs],
            'vb': [abs(val(v)) / P + 1e-9 for v in vecs], 'nn': [int(bool(x)) for x in nn]}


CANON_EDGES = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2**380, 2**381 % P, 2**28 - 1, 2**28, 2**364, R392 % P]


def fp_values(rng, nrand, kmax, spread, boundary_ks=(-9, -1, 0, 1, 8), multiples=(-100, -7, -3, -1, 0, 1, 2, 5, 64, 100)):
    """(name, limbs) of the Fp operand families, for a function that takes values up to kmax p and limbs up to (spread + 1) 2^28"""
    out = []
    for v in CANON_EDGES:
        out.append(('canon %#x' % v if v < 2**64 else 'canon ~2^%d' % v.bit_length(), limbs_of(v)))
        out.append(('redundant limbs of ~2^%d' % v.bit_length(), scramble(limbs_of(v), spread, rng)))
        for k in (-3, -1, 1, 2, 5):
            if abs(k) + 1 <= kmax:
                out.append(('~2^%d %+d p' % (v.bit_length(), k), lazy(v + k * P, min(spread, 1), rng)))
    for k in multiples:
        if abs(k) <= kmax:
            out.append(('%d p exact limbs' % k, limbs_of(k * P)))
            out.append(('%d p lazy' % k, lazy(k * P, spread, rng)))
    for k in boundary_ks:
        if abs(k) + 1 <= kmax:
            for d in (-2, -1, 0, 1, 2):
                out.append(('rounding boundary %d p + p/2 %+d' % (k, d), lazy(k * P + P // 2 + d, min(spread, 2), rng)))
                out.append(('rounding boundary %d p + p/2 %+d exact limbs' % (k, d), limbs_of(k * P + P // 2 + d)))
    for v in (RED_MAX, -RED_MAX, P // 2, -(P // 2)):            # top limbs 55386, -55387, 53256, -53257
        out.append(('extreme reduced top limb %d' % (v >> 364), limbs_of(v)))
    for i in range(nrand):
        v = rng.randrange(-kmax * P, kmax * P)
        out.append(('random %d' % i, lazy(v, rng.choice([0, 1, spread][:spread + 1] if spread < 2 else (0, 1, spread)), rng)))
    return out


SIGNS = {'positive': (1,), 'negative': (-1,), 'alternating': (1, -1), 'alternating from minus': (-1, 1)}


def extreme_operands(mag, top):
    """operands at the limb magnitude a contract allows: all positive, all negative, alternating signs (the signed 64-bit column sums
    and the arithmetic-shift carries), with a top limb of either sign"""
    return [('limbs %s at %d, top %d' % (nm, mag, t), pattern(mag, s, t)) for nm, s in SIGNS.items() for t in ((top, -top) if top else (0,))]


def reduced_values(rng, nrand):
    """reduced operands (fp_reduce / REDC outputs: limbs 0..12 in [0, 2^28)) at the edges and at random"""
    out = [('reduced %d' % v if abs(v) < 4 else 'reduced ~%s2^%d' % ('-' if v < 0 else '', abs(v).bit_length()), limbs_of(v))
           for v in (0, 1, -1, 2, RED_MAX, -RED_MAX, P // 2, -(P // 2), val(limbs_of_elem(1)), 2**364, -2**364, 2**28 - 1, 2**28)]
    out.append(('reduced all limbs maximal, top %d' % TOP_MAX, [M] * (NL - 1) + [TOP_MAX - 1]))
    out.append(('reduced top %d alone' % TOP_MIN, [0] * (NL - 1) + [TOP_MIN + 1]))
    out.append(('reduced all limbs maximal, top -1', [M] * (NL - 1) + [-1]))
    for i in range(nrand):
        out.append(('reduced random %d' % i, limbs_of(rng.randrange(-RED_MAX, RED_MAX))))
    for nm, l in out:
        assert abs(val(l)) * 100 <= 52 * P, nm
    return out


# ---- Fp12 helpers: twelve limb vectors in tower order <-> the oracle's six Fp2 in w-power order
def f12_of_vecs(vs):
    f = [None] * 6
    for k in range(6):
        f[TOWER_TO_W[k]] = (elem_of(vs[2 * k]), elem_of(vs[2 * k + 1]))
    return tuple(f)


def vecs_of_f12(f):
    out = []
    for k in range(6):
        x = f[TOWER_TO_W[k]]
        out += [limbs_of_elem(x[0]), limbs_of_elem(x[1])]
    return out


def f2_of_vecs(vs):
    return (elem_of(vs[0]), elem_of(vs[1]))


F12_ONE = ((1, 0),) + ((0, 0),) * 5
F12_ZERO = ((0, 0),) * 6


def cyclotomic(a):
    """a^((p^6 - 1)(p^2 + 1)): an element of the cyclotomic subgroup"""
    t = c.f12_mul(c.f12_conj(a), c.f12_inv(a))
    return c.f12_mul(c.f12_frob(t, 2), t)


def rand_f12(rng):
    return tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))


def fp4_sqr(a, b):
    """(a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi): (a^2 + xi b^2, 2 a b)"""
    return c.f2_add(c.f2_sqr(a), c.f2_mul_xi(c.f2_sqr(b))), c.f2_muls(c.f2_mul(a, b), 2)


def cyc_c_sqr(z):
    """Karabina's compressed squaring on (z2, z3, z4, z5), restated from the formulas (pairing.cuh cyc_c_sqr): defined for any input,
    and equal to the compressed square for elements of the cyclotomic subgroup (test_field_cases checks that against f12_sqr)"""
    z2, z3, z4, z5 = z
    t0, t1 = fp4_sqr(z2, z3)
    t2, t3 = fp4_sqr(z4, z5)
    three = lambda t: c.f2_muls(t, 3)
    two = lambda t: c.f2_muls(t, 2)
    return (c.f2_add(three(c.f2_mul_xi(t3)), two(z2)), c.f2_sub(three(t2), two(z3)), c.f2_sub(three(t0), two(z4)), c.f2_add(three(t1), two(z5)))


def gs_sqr(f):
    """the Granger-Scott squaring restated from its formulas (tower.cuh fp12_cyclotomic_sqr_body), w-power order in and out"""
    z0, z2, z4, z1, z3, z5 = f[0], f[1], f[2], f[3], f[4], f[5]     # w^0 .. w^5 = z0 z2 z4 z1 z3 z5
    t0, t1 = fp4_sqr(z0, z1)
    n2, n3, n4, n5 = cyc_c_sqr((z2, z3, z4, z5))
    n0 = c.f2_sub(c.f2_muls(t0, 3), c.f2_muls(z0, 2))
    n1 = c.f2_add(c.f2_muls(t1, 3), c.f2_muls(z1, 2))
    return (n0, n2, n4, n1, n3, n5)


def compress(f):
    return (f[1], f[4], f[2], f[5])     # z2 = c1.a0 (w), z3 = c0.a2 (w^4), z4 = c0.a1 (w^2), z5 = c1.a2 (w^5)


def line3_f12(l0, l2, l3):
    """l0 + l2 w^2 + l3 w^3 (tower.cuh fp12_mul_by_line_body)"""
    z = (0, 0)
    return (l0, z, l2, l3, z, z)


def line5_f12(c0, c2, c4, c3, c5):
    """c0 + c2 w^2 + c3 w^3 + c4 w^4 + c5 w^5, coefficients in the order of tower.cuh line5_t (c0, c2, c4, c3, c5): the embedding of
    tower.cuh fp12_from_line5 -- c0.a0 = c0, c0.a1 = c2, c0.a2 = c4, c1.a0 = 0, c1.a1 = c3, c1.a2 = c5"""
    return (c0, (0, 0), c2, c3, c4, c5)


# ---- the lists
_cache = {}


def f12_operands(rng):
    """(name, oracle f12) of the Fp12 operand families"""
    h, g = (P - 1) // 2, (P + 1) // 2
    out = [('zero', F12_ZERO), ('one', F12_ONE), ('minus one', ((P - 1, 0),) + ((0, 0),) * 5),
           ('every component p-1', ((P - 1, P - 1),) * 6), ('every component (p-1)/2', ((h, h),) * 6), ('every component (p+1)/2', ((g, g),) * 6)]
    for pos in range(12):
        f = [[0, 0] for _ in range(6)]
        f[pos // 2][pos % 2] = rng.randrange(1, P) if pos % 3 else 1
        out.append(('single component %d (w^%d, c%d)' % (pos, pos // 2, pos % 2), tuple(tuple(x) for x in f)))
    r = rand_f12(rng)
    out.append(('element of Fp6', (r[0], (0, 0), r[2], (0, 0), r[4], (0, 0))))
    out.append(('element of Fp2', (r[0],) + ((0, 0),) * 5))
    for i in range(6):
        out.append(('random %d' % i, rand_f12(rng)))
    return out


def f12_extreme_vecs():
    """(name, twelve limb vectors) at the ends of the reduced range: the pack / unpack edge of the LDS accumulator"""
    hi, lo = [M] * (NL - 1) + [TOP_MAX - 1], [0] * (NL - 1) + [TOP_MIN + 1]
    return [('every component at the largest reduced top limb', [hi] * 12), ('every component at the most negative reduced top limb', [lo] * 12),
            ('reduced top limbs alternating', [hi, lo] * 6), ('reduced top limbs alternating from minus', [lo, hi] * 6),
            ('every component +0.52 p', [limbs_of(RED_MAX)] * 12), ('every component -0.52 p', [limbs_of(-RED_MAX)] * 12),
            ('every component -1 (all limbs maximal, top -1)', [limbs_of(-1)] * 12)]


def cyclotomic_elements(rng):
    return [('cyclotomic one', F12_ONE)] + [('cyclotomic %d' % i, cyclotomic(rand_f12(rng))) for i in range(3)]


def line_coeff_sets(rng, npos, nrand):
    """coefficient tuples of a sparse line value with npos positions: all zero, one non-zero in each position, +-(p-1)/2, random"""
    h = (P - 1) // 2
    out = [('all coefficients zero', [(0, 0)] * npos)]
    for k in range(npos):
        cs = [(0, 0)] * npos
        cs[k] = (rng.randrange(1, P), rng.randrange(P)) if k % 2 else (1, 0)
        out.append(('only coefficient %d non-zero' % k, cs))
    out.append(('coefficients at (p-1)/2', [(h, h)] * npos))
    out.append(('coefficients at -(p-1)/2', [(P - h, P - h)] * npos))
    out.append(('coefficients at +-(p-1)/2', [(h, P - h) if k % 2 else (P - h, h) for k in range(npos)]))
    for i in range(nrand):
        out.append(('random line %d' % i, [(rng.randrange(P), rng.randrange(P)) for _ in range(npos)]))
    return out


def f2_vecs(x):
    return [limbs_of_elem(x[0]), limbs_of_elem(x[1])]


def build():
    """{operation name: [case]}, deterministic"""
    if _cache:
        return _cache
    rng = random.Random(20240607)
    L = {}
    big = 2**31 - 2**8 - 2
    # -- fp_norm / fp_reduce / fp_canon: any limbs below 2^31 - 2^8, values within +-120 p
    wide = fp_values(rng, 300, 110, 3) + extreme_operands(big, 12_000_000) + extreme_operands(big, 0)
    for op in ('FP_NORM', 'FP_REDUCE', 'FP_CANON'):
        L[op] = [case(nm, [l]) for nm, l in wide]
    # -- fp_reduce_lin2: |ka| a.lb + |kb| b.lb < 2^35, |ka| |a| + |kb| |b| <= 120 p
    lin2 = []
    for ka, kb in LIN2_PAIRS:
        for i in range(50):
            va, vb = rng.randrange(-4 * P, 4 * P), rng.randrange(-4 * P, 4 * P)
            lin2.append(case('(%d, %d) random %d' % (ka, kb, i), [lazy(va, rng.choice((0, 1, 5)), rng), lazy(vb, rng.choice((0, 1, 5)), rng)], (ka, kb)))
        for k in (-7, -1, 0, 3):                            # ka a + kb b at k p + p/2 +- a little (b = 0 there)
            for d in (-2, -1, 0, 1, 2):
                v = k * P + P // 2 + d
                if v % ka == 0:
                    lin2.append(case('(%d, %d) rounding boundary %d p + p/2 %+d' % (ka, kb, k, d), [lazy(v // ka, 2, rng), lazy(0, 2, rng)], (ka, kb)))
        for nm, l in extreme_operands(2**31 - 2, 300_000):
            lin2.append(case('(%d, %d) %s' % (ka, kb, nm), [l, [-x for x in l]], (ka, kb)))
        for nm, l in reduced_values(rng, 0):
            lin2.append(case('(%d, %d) %s' % (ka, kb, nm), [l, limbs_of(RED_MAX)], (ka, kb)))
    L['FP_REDUCE_LIN2'] = lin2
    # -- multiplier leaves: operand limb bounds A B <= 2^59, |a| |b| <= 256 p^2
    mv = fp_values(rng, 300, 11, 1, boundary_ks=(-9, -1, 0, 1, 8), multiples=(-7, -3, -1, 0, 1, 2, 5))
    ext_a, ext_b = extreme_operands(2**30 - 1, 1_600_000), extreme_operands(2**29, 1_600_000)
    mul = [case('%s * %s' % (mv[i][0], mv[(7 * i + 3) % len(mv)][0]), [mv[i][1], mv[(7 * i + 3) % len(mv)][1]]) for i in range(len(mv))]
    mul += [case('%s * %s' % (a[0], b[0]), [a[1], b[1]]) for a in ext_a for b in ext_b]
    L['FP_MUL'] = mul
    L['FP_SQR'] = [case(nm, [l]) for nm, l in mv + extreme_operands(759_250_124, 1_600_000)]
    inv = [case(nm, [l]) for nm, l in mv] + [case('2^%d' % k, [limbs_of_elem(2**k)]) for k in range(0, 381, 13)] + \
        [case('p - 2^%d' % k, [limbs_of_elem(P - 2**k)]) for k in range(1, 380, 17)]
    L['FP_INV'] = inv
    L['FP_INV_VAR'] = inv
    # (the whole multiplier list -- its 300 random operands are squares and non-squares as they fall -- and both kinds by construction:
    # x^2, and -x^2, a non-square since p = 3 mod 4)
    L['FP_SQRT'] = [case(nm, [l]) for nm, l in mv] + \
        [case('%s %d' % ('square' if i % 2 == 0 else 'non-square', i), [limbs_of_elem(pow(rng.randrange(1, P), 2, P) * (1 if i % 2 == 0 else -1))]) for i in range(60)]
    R384 = 1 << 384
    raws = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, R384 - 1, R384 - P, (R384 // P) * P, (R384 // P) * P - 1, 1 << 383, (1 << 376) - 1, 0xff << 376]
    raws += [((2 * k + 1) * P // 512 + d) % R384 for k in (0, 1, 7, 100, 1260, 2520, 2521) for d in (-1, 0, 1)]
    raws += [rng.randrange(R384) for _ in range(150)] + [rng.randrange(P) for _ in range(100)]
    L['FP_FROM_RAW'] = [{'name': 'raw words %#x' % v if v < 2**64 else 'raw words ~2^%d (%d)' % (v.bit_length(), i), 'par': [], 'lb': [0.0], 'vb': [0.0], 'nn': [0],
                         'vecs': [[(v >> (32 * k)) & 0xffffffff if not (v >> (32 * k)) & 0x80000000 else ((v >> (32 * k)) & 0xffffffff) - 2**32 for k in range(12)] + [0, 0]]}
                        for i, v in enumerate(raws)]
    # -- one-lane Karatsuba Fp2 products: normalised operands (limbs up to 2^28 + 2^8), the difference form on REDUCED operands
    red = reduced_values(rng, 200)
    nrm = red + [('normalised %s + 255 per limb' % nm, [x + 255 for x in l[:NL - 1]] + [l[-1]]) for nm, l in red[:20]] + \
        [('normalised %s - 255 per limb' % nm, [x - 255 for x in l[:NL - 1]] + [l[-1]]) for nm, l in red[:20]] + \
        [('%s %+d p' % (nm, k), limbs_of(val(l) + k * P)) for nm, l in red[:12] for k in (-2, 1, 2)]

    def quads(vs, n):
        return [case(' | '.join(vs[(j * i + j) % len(vs)][0] for j in (1, 3, 5, 7)), [vs[(j * i + j) % len(vs)][1] for j in (1, 3, 5, 7)]) for i in range(n)]

    def pairs(vs, n):
        return [case(' | '.join(vs[(j * i + j) % len(vs)][0] for j in (1, 3)), [vs[(j * i + j) % len(vs)][1] for j in (1, 3)]) for i in range(n)]
    L['FP2_KARA_PRODUCTS'] = quads(nrm, len(nrm))
    L['FP2_KARA_DIFFS'] = quads(red, len(red))
    L['FP2L_MUL'] = quads(red, len(red))
    L['FP2L_SQR'] = pairs(red, len(red))
    L['FP2L_INV'] = pairs(red, len(red))          # (its last pair is zero: 0 -> 0)
    # -- lane-split Fp2
    ext2 = extreme_operands(2**29, 1_100_000)
    L['FP2_MUL'] = quads(mv, len(mv)) + [case(' | '.join(ext2[(i + j) % len(ext2)][0] for j in (0, 3, 5, 6)), [ext2[(i + j) % len(ext2)][1] for j in (0, 3, 5, 6)]) for i in range(len(ext2))]
    sq = nrm + [('%s %+d p' % (nm, k), limbs_of(val(l) + k * P)) for nm, l in red[:12] for k in (-7, -3, 3, 7)] + \
        [('normalised limbs %s' % nm, [x if x > 0 else -15 for x in pattern(2**28 + 15, s, t)[:NL - 1]] + [t]) for nm, s in SIGNS.items() for t in (800_000, -800_000)]
    L['FP2_SQR'] = pairs(sq, len(sq))
    xv = fp_values(rng, 200, 110, 2) + extreme_operands(2**30 - 2, 12_000_000)
    L['FP2_MUL_XI'] = pairs(xv, len(xv))
    L['FP2_CONJ'] = pairs(xv, len(xv))
    L['FP2_MUL_FP'] = [case(' | '.join(mv[(j * i + j) % len(mv)][0] for j in (1, 3, 5)), [mv[(j * i + j) % len(mv)][1] for j in (1, 3, 5)]) for i in range(len(mv))] + \
        [case('%s | %s' % (a[0], b[0]), [a[1], [-x for x in a[1]], b[1]]) for a in ext_a for b in ext_b[:2]]
    L['FP2_INV'] = pairs(mv, len(mv)) + [case('zero as lazy multiples of p', [lazy(3 * P, 1, rng), lazy(-2 * P, 1, rng)])]          # (the last pair of the list is zero in exact limbs)
    # -- Fp12: reduced operands (only reduced elements pack into the LDS accumulator)
    ops12 = [(nm, vecs_of_f12(f)) for nm, f in f12_operands(rng)] + f12_extreme_vecs()
    cyc = [(nm, vecs_of_f12(f)) for nm, f in cyclotomic_elements(rng)]
    packs = ops12 + cyc + [('packed field ends', [[M] * (NL - 1) + [2**19 - 1], [0] * (NL - 1) + [-2**19]] * 6),
                           ('packed field: every top limb bit alone', [[0] * (NL - 1) + [(1 << (k % 19)) * (-1 if k % 2 else 1)] for k in range(12)])] + \
        [('random reduced %d' % i, [limbs_of(rng.randrange(-RED_MAX, RED_MAX)) for _ in range(12)]) for i in range(20)]
    L['F12_PACK'] = [case(nm, vs) for nm, vs in packs]
    L['F12_SH_SQR'] = [case(nm, vs) for nm, vs in ops12 + cyc]
    L['F12_SH_CYC_SQR'] = [case(nm, vs) for nm, vs in cyc + ops12]
    L['F12_SH_MUL'] = [case('%s * %s' % (ops12[i][0], ops12[(5 * i + 2) % len(ops12)][0]), ops12[i][1] + ops12[(5 * i + 2) % len(ops12)][1]) for i in range(len(ops12))]
    accs = ops12[:6] + ops12[-9:]
    for op, npos in (('F12_SH_MUL_LINE', 3), ('F12_SH_MUL_2LINES', 6), ('F12_SH_MUL_LINE5', 5)):
        lines = line_coeff_sets(rng, npos, 8)
        ext = [('coefficients at the largest reduced top limb', [[M] * (NL - 1) + [TOP_MAX - 1]] * (2 * npos)),
               ('coefficients at the most negative reduced top limb', [[0] * (NL - 1) + [TOP_MIN + 1]] * (2 * npos))]
        L[op] = [case('%s * %s' % (accs[(3 * i + 1) % len(accs)][0], nm), accs[(3 * i + 1) % len(accs)][1] + sum((f2_vecs(x) for x in cs), []))
                 for i, (nm, cs) in enumerate(lines * 2)] + \
            [case('%s * %s' % (accs[-(i + 1)][0], nm), accs[-(i + 1)][1] + vs) for i, (nm, vs) in enumerate(ext)]
    # -- compressed squarings: (z2, z3, z4, z5) of cyclotomic elements, and of anything (the formulas are defined everywhere)
    def z_vecs(vs):          # tower slots c1.a0, c0.a2, c0.a1, c1.a2
        return vs[6:8] + vs[4:6] + vs[2:4] + vs[10:12]
    cz, seen = [], set()
    for nm, vs in cyc + ops12[3:]:                  # (several Fp12 operands share their z-vectors, e.g. all zero: each once)
        z = z_vecs(vs)
        if repr(z) not in seen:
            seen.add(repr(z))
            cz.append(case(nm, z))
    for op in ('CYC_C_SQR', 'CYC_C_SQR_UNPACKED', 'CYC_C_SQR_KARA'):
        L[op] = cz
    L['F12_POW_X'] = [case(nm, vs) for nm, vs in cyc] + [case('cyclotomic %d' % i, vecs_of_f12(cyclotomic(rand_f12(rng)))) for i in range(3, 9)]
    L['F12_INV'] = [case(nm, vs) for nm, vs in ops12 + cyc]
    L['F12_FROB1'] = L['F12_INV']
    L['F12_FROB2'] = L['F12_INV']
    coop_lists(L, ops12, cyc, accs, mv, ext2)
    import point_cases                       # the curve-layer rows (G1_*, G2L_*, G2S_*, G2Q_DBL): tests/point_cases.py
    L.update(point_cases.build())
    import miller_cases                      # the Miller steps, the merged lines and the row evaluation: tests/miller_cases.py
    L.update(miller_cases.build())
    _cache.update(L)
    return _cache


# ---- the wave-cooperative engine (csrc/coop.cuh, lanes = 64).  The last parameter of every row is the fill word of coop_shared.
FILLS = (0, -1, 0x7fffffff)           # 0, 0xffffffff and 0x7fffffff as the signed words of a record
COOP_ALIASES = {'COOP_MUL': (0, 1, 2), 'COOP_CYC_SQR': (0, 1)}
ZERO_VEC = [0] * NL
# the two ends of the reduced range, as (name, the positive vector, the negative vector)
COOP_MAGS = (('0.52 p', limbs_of(RED_MAX), limbs_of(-RED_MAX)),
             ('extreme limbs', [M] * (NL - 1) + [TOP_MAX - 1], [0] * (NL - 1) + [TOP_MIN + 1]))


def neg_vec(v):
    return [-x for x in v]


def conj_vecs(vs):
    """what coop_conj makes of a reduced element: the odd powers of w (tower vectors 6..11) negated limb by limb"""
    return [list(v) for v in vs[:6]] + [neg_vec(v) for v in vs[6:]]


def mult_form(x):
    """a multiplier output for the field element x: its Montgomery residue in [0, p), exact limbs"""
    return limbs_of(x % P * R392 % P)


def frob_vecs(f, j):
    """what coop_frob<j> makes of the reduced element f: the w^0 coefficient copied (j = 2) or conjugated limb-wise (j = 1), every
    other coefficient a product by a constant"""
    g = c.f12_frob(f, j)
    out = []
    for k in range(6):
        pw = TOWER_TO_W[k]
        if pw == 0:
            a = f2_vecs(f[0])
            out += [a[0], neg_vec(a[1]) if j == 1 else a[1]]
        else:
            out += [mult_form(g[pw][0]), mult_form(g[pw][1])]
    return out


def signed_f12(pos, neg, re, im, flip0=False):
    """twelve vectors: every coefficient (re, im) times the magnitude (+1: pos, -1: neg, 0: zero); flip0 negates the w^0 coefficient"""
    pick = lambda s: pos if s > 0 else neg if s < 0 else ZERO_VEC
    out = []
    for k in range(6):
        s = -1 if flip0 and TOWER_TO_W[k] == 0 else 1
        out += [pick(s * re), pick(s * im)]
    return out


# (a.re, a.im, b.re, b.im): the signs that give every product a_i b_j the same sign in the named part (and zero in the other one):
# re = a.re b.re - a.im b.im, im = a.re b.im + a.im b.re.  All 36 products alike means six like terms in the half i + j = 5 of
# coefficient 5 and five in the wrapped half i + j = 6 of coefficient 0; flip0 (a_0 negated) sets coefficient 0's own half i + j = 0
# against its wrapped half and one term of every other sum against the rest.
SAME_SIGN = (('real parts all positive', (1, 1, 1, -1)), ('real parts all negative', (1, 1, -1, 1)),
             ('imaginary parts all positive', (1, 1, 1, 1)), ('imaginary parts all negative', (1, 1, -1, -1)))
# squaring: a_i a_j of one operand (re = re^2 - im^2, im = 2 re im); the off-diagonal products are doubled
SAME_SIGN_SQR = (('real parts all positive', (1, 0)), ('real parts all negative', (0, 1)), ('imaginary parts all positive', (1, 1)),
                 ('imaginary parts all negative', (1, -1)), ('imaginary parts all positive, operand negative', (-1, -1)))


def _cycle_pars(cases_, pars):
    """give case i the parameters pars(i) + fill i: alias / set / njobs and the three fills all occur, and neighbours differ"""
    out = []
    for i, (nm, vs) in enumerate(cases_):
        out.append(case(nm, vs, tuple(pars(i)) + (FILLS[(i + i // 3) % 3],)))
    for a, b in zip(out, out[1:] + out[:1]):
        assert a['vecs'] != b['vecs'], (a['name'], b['name'])       # neighbours differ in their operands, whatever the parameters
    return out


def coop_lists(L, ops12, cyc, accs, mv, ext2):
    rng = random.Random(20250923)          # a generator of its own: the lists above stay as they were
    n12 = len(ops12)
    rand12 = [vs for nm, vs in ops12 if nm.startswith('random')]
    # -- coop_mul
    mul = [('%s * %s' % (ops12[i][0], ops12[(5 * i + 2) % n12][0]), ops12[i][1] + ops12[(5 * i + 2) % n12][1]) for i in range(n12)]
    for mn, pos, neg in COOP_MAGS:
        for sn, (ar, ai, br, bi) in SAME_SIGN:
            for flip0 in (False, True):
                mul.append(('same-sign products, %s, at %s%s' % (sn, mn, ', a_0 negated' if flip0 else ''),
                            signed_f12(pos, neg, ar, ai, flip0) + signed_f12(pos, neg, br, bi)))
    ext12 = f12_extreme_vecs()
    chain_ops = [(nm, vs) for nm, vs in ext12] + [('random %d' % i, vs) for i, vs in enumerate(rand12[:3])] + cyc[1:]
    for i, (nm, vs) in enumerate(chain_ops):
        onm, ovs = chain_ops[(i + 3) % len(chain_ops)]
        mul.append(('conj(%s) * %s' % (nm, onm), conj_vecs(vs) + ovs))
        mul.append(('%s * conj(%s)' % (onm, nm), ovs + conj_vecs(vs)))
        mul.append(('conj(%s) * conj(%s)' % (nm, onm), conj_vecs(vs) + conj_vecs(ovs)))
    for i, (nm, vs) in enumerate(chain_ops):
        f, (onm, ovs) = f12_of_vecs(vs), chain_ops[(i + 2) % len(chain_ops)]
        mul.append(('frob1(%s) * %s' % (nm, onm), frob_vecs(f, 1) + ovs))
        mul.append(('%s * frob2(%s)' % (onm, nm), ovs + frob_vecs(f, 2)))
        mul.append(('frob1(%s) * frob2(%s)' % (nm, onm), frob_vecs(f, 1) + frob_vecs(f12_of_vecs(ovs), 2)))
    L['COOP_MUL'] = _cycle_pars(mul, lambda i: (i % 3,))
    # -- coop_sqr
    sqr = list(ops12) + list(cyc)
    for mn, pos, neg in COOP_MAGS:
        for sn, (re, im) in SAME_SIGN_SQR:
            for flip0 in (False, True):
                sqr.append(('same-sign products, %s, at %s%s' % (sn, mn, ', a_0 negated' if flip0 else ''), signed_f12(pos, neg, re, im, flip0)))
    L['COOP_SQR'] = _cycle_pars(sqr, lambda i: ())
    # -- coop_mul_line: f, l0, l2, l3
    lines = line_coeff_sets(rng, 3, 8)
    for z in range(3):
        cs = [(rng.randrange(1, P), rng.randrange(1, P)) for _ in range(3)]
        cs[z] = (0, 0)
        lines.append(('sparse line, coefficient %d zero' % z, cs))
    ml = [('%s * %s' % (accs[(3 * i + 1) % len(accs)][0], nm), accs[(3 * i + 1) % len(accs)][1] + sum((f2_vecs(x) for x in cs), []))
          for i, (nm, cs) in enumerate(lines * 2)]
    for i, (mn, pos, neg) in enumerate(COOP_MAGS):
        ml.append(('%s * coefficients at %s' % (accs[-(i + 1)][0], mn), accs[-(i + 1)][1] + [pos] * 6))
        ml.append(('%s * coefficients at -%s' % (accs[-(i + 3)][0], mn), accs[-(i + 3)][1] + [neg] * 6))
        for sn, (ar, ai, br, bi) in SAME_SIGN:
            for flip0 in (False, True):
                ml.append(('same-sign products, %s, at %s%s' % (sn, mn, ', f_0 negated' if flip0 else ''),
                           signed_f12(pos, neg, ar, ai, flip0) + signed_f12(pos, neg, br, bi)[:6]))
    for i, (nm, vs) in enumerate(cyc[1:]):
        ml.append(('conj(%s) * %s' % (nm, lines[-(i + 1)][0]), conj_vecs(vs) + sum((f2_vecs(x) for x in lines[-(i + 1)][1]), [])))
    L['COOP_MUL_LINE'] = _cycle_pars(ml, lambda i: (i % 2,))
    # -- the cyclotomic squaring (judged by gs_sqr, defined everywhere), a^x, conjugation and the Frobenius maps
    L['COOP_CYC_SQR'] = _cycle_pars(list(cyc) + list(ops12) + [('conj(%s)' % nm, conj_vecs(vs)) for nm, vs in cyc[1:]], lambda i: (i % 2,))
    more = [('cyclotomic %d' % i, vecs_of_f12(cyclotomic(rand_f12(rng)))) for i in range(3, 7)]
    L['COOP_POW_X'] = _cycle_pars(list(cyc) + more + [('conj(%s)' % nm, conj_vecs(vs)) for nm, vs in cyc[1:3]], lambda i: ())
    for op in ('COOP_CONJ', 'COOP_FROB1', 'COOP_FROB2'):
        L[op] = _cycle_pars(list(ops12) + list(cyc), lambda i: ())
    # -- the product rounds of the point steps: operands as fp2_mul takes them (the multiplier's operand families)
    def jobs(i, count, step):
        return [mv[(step * i + 7 * t + 1) % len(mv)] for t in range(count)]
    jl = []
    for i in range(36):
        js = jobs(i, 48, 11)
        jl.append((' | '.join(nm for nm, _ in js[:4]) + ' ...', [l for _, l in js]))
    for i in range(4):
        jl.append(('extreme limbs: %s ...' % ext2[i][0], [ext2[(i + t) % len(ext2)][1] for t in range(48)]))
    L['COOP_JOBS'] = _cycle_pars(jl, lambda i: (5 + i % 2,))
    fs = list(ops12) + list(cyc)
    L['COOP_SQR_MUL_JOBS'] = _cycle_pars([('%s, jobs from %d' % (nm, i), vs + [l for _, l in jobs(i, 40, 13)]) for i, (nm, vs) in enumerate(fs)], lambda i: ())
    L['COOP_LINE_MUL_JOBS'] = _cycle_pars([(nm + ', jobs from %d' % i, vs + [l for _, l in jobs(i, 48, 17)]) for i, (nm, vs) in enumerate(ml[::2])], lambda i: (i % 2,))
    # -- the final exponentiation: random elements (not one), r-th powers, elements of Fp6 and Fp2, +-1 (one), zero (fp12_inv(0) = 0
    # must give INVALID); Fp12 is a field, so there is no non-invertible element but zero
    fe = [(nm, vs) for nm, vs in ops12 if nm.startswith(('random', 'element of', 'one', 'minus one', 'zero', 'every component'))]
    rth = [('r-th power %d' % i, vecs_of_f12(c.f12_pow(rand_f12(rng), c.R))) for i in range(3)]
    fe += rth
    fe += [('single component %d' % pos, ops12[6 + pos][1]) for pos in (0, 1, 5, 6, 11)]
    fe += ext12[:3] + cyc[1:2]
    fe.append(('r-th power times an element of Fp6', vecs_of_f12(c.f12_mul(f12_of_vecs(rth[0][1]), f12_of_vecs(ops12[18][1])))))
    assert ops12[18][0] == 'element of Fp6'
    L['COOP_FINAL_EASY'] = _cycle_pars(fe, lambda i: ())
    L['COOP_FINAL_VERDICT'] = _cycle_pars(fe, lambda i: ())


def with_pars(cs, fill=None, first=None):
    """the same case (the same operand vectors, so the same expected value) with another fill word or another first parameter"""
    par = list(cs['par'])
    if fill is not None:
        par[-1] = fill
    if first is not None:
        par[0] = first
    return dict(cs, par=par)


# ---- judging the outputs
MULT_OUT = {'FP_MUL', 'FP_SQR', 'FP_INV', 'FP_INV_VAR', 'FP2_KARA_PRODUCTS', 'FP2_KARA_DIFFS', 'FP2_MUL', 'FP2_SQR', 'FP2_MUL_FP'}
REDUCED_OUT = {'FP_REDUCE', 'FP_REDUCE_LIN2', 'FP_FROM_RAW', 'F12_SH_SQR', 'F12_SH_MUL', 'F12_SH_MUL_LINE', 'F12_SH_MUL_2LINES', 'F12_SH_MUL_LINE5', 'F12_SH_CYC_SQR',
               'CYC_C_SQR', 'CYC_C_SQR_UNPACKED', 'CYC_C_SQR_KARA', 'F12_INV',
               'COOP_MUL', 'COOP_SQR', 'COOP_MUL_LINE', 'COOP_CYC_SQR', 'COOP_FINAL_EASY'}     # (the rounds of coop.cuh end in fp2_reduce)
COOP_REDUCED_F = {'COOP_SQR_MUL_JOBS', 'COOP_LINE_MUL_JOBS'}      # outputs 0..11: f, reduced; the rest: products


def _f2mul_raw(a, b):
    """the Montgomery Fp2 product on raw integers: (a0 b0 - a1 b1, a0 b1 + a1 b0) / R"""
    return ((a[0] * b[0] - a[1] * b[1]) * R392_INV % P, (a[0] * b[1] + a[1] * b[0]) * R392_INV % P)


def expected(op, cs, reps=1):
    """what the outputs must be congruent to modulo p, as raw integers per output vector (None: judged otherwise)"""
    v = [val(l) for l in cs['vecs']]
    if op in ('FP_NORM', 'FP_REDUCE', 'FP_CANON'):
        return [v[0]] if op != 'FP_CANON' else [v[0], None]
    if op == 'FP_REDUCE_LIN2':
        return [cs['par'][0] * v[0] + cs['par'][1] * v[1]]
    if op == 'FP_MUL':
        a = v[0]
        for _ in range(reps):
            a = a * v[1] * R392_INV % P
        return [a]
    if op == 'FP_SQR':
        a = v[0]
        for _ in range(reps):
            a = a * a * R392_INV % P
        return [a]
    if op in ('FP_INV', 'FP_INV_VAR'):
        return [R392 * R392 * pow(v[0], -1, P) % P if v[0] % P else 0]
    if op == 'FP_SQRT':
        return [None, None]
    if op == 'FP_FROM_RAW':
        return [sum((w & 0xffffffff) << (32 * k) for k, w in enumerate(cs['vecs'][0][:12])) << 8]
    if op == 'FP2_KARA_PRODUCTS':
        r = _f2mul_raw(v[0:2], v[2:4])
        return [r[0], r[0] + r[1]]
    if op == 'FP2_KARA_DIFFS':           # (a - b)(a - xi b), xi = 1 + u
        x = (v[0] - v[2], v[1] - v[3])
        y = (v[0] - v[2] + v[3], v[1] - v[2] - v[3])
        r = _f2mul_raw(x, y)
        return [r[0], r[0] + r[1]]
    if op in ('FP2_MUL', 'FP2L_MUL'):
        a = v[0:2]
        for _ in range(reps):
            a = _f2mul_raw(a, v[2:4])
        return list(a)
    if op in ('FP2_SQR', 'FP2L_SQR'):
        a = v[0:2]
        for _ in range(reps):
            a = _f2mul_raw(a, a)
        return list(a)
    if op == 'FP2_MUL_XI':
        return [v[0] - v[1], v[0] + v[1]]
    if op == 'FP2_CONJ':
        return [v[0], -v[1]]
    if op == 'FP2_MUL_FP':
        return [v[0] * v[2] * R392_INV % P, v[1] * v[2] * R392_INV % P]
    if op in ('FP2_INV', 'FP2L_INV'):
        n = (v[0] * v[0] + v[1] * v[1]) % P
        if n == 0:
            return [0, 0]
        ni = pow(n, -1, P) * R392 * R392 % P
        return [v[0] * ni % P, -v[1] * ni % P]
    if op.startswith('COOP_'):
        return _coop_expected(op, cs, v, reps)
    if op in ('CYC_C_SQR', 'CYC_C_SQR_UNPACKED', 'CYC_C_SQR_KARA'):
        z = tuple(f2_of_vecs(cs['vecs'][2 * k:2 * k + 2]) for k in range(4))
        for _ in range(reps):
            z = cyc_c_sqr(z)
        return [x * R392 % P for t in z for x in t]
    f = f12_of_vecs(cs['vecs'][:12])
    if op == 'F12_PACK':
        return v[:12]
    if op == 'F12_SH_SQR':
        for _ in range(reps):
            f = c.f12_sqr(f)
    elif op == 'F12_SH_CYC_SQR':
        for _ in range(reps):
            f = gs_sqr(f)
    elif op == 'F12_POW_X':
        f = c.f12_conj(c.f12_pow(f, c.X_ABS))
    elif op == 'F12_INV':
        f = c.f12_inv(f) if f != F12_ZERO else F12_ZERO
    elif op == 'F12_FROB1':
        f = c.f12_frob(f, 1)
    elif op == 'F12_FROB2':
        f = c.f12_frob(f, 2)
    else:
        rest = [f2_of_vecs(cs['vecs'][12 + 2 * k:14 + 2 * k]) for k in range((len(cs['vecs']) - 12) // 2)]
        if op == 'F12_SH_MUL':
            b = f12_of_vecs(cs['vecs'][12:24])
        elif op == 'F12_SH_MUL_LINE':
            b = line3_f12(*rest)
        elif op == 'F12_SH_MUL_2LINES':
            b = c.f12_mul(line3_f12(*rest[:3]), line3_f12(*rest[3:]))
        elif op == 'F12_SH_MUL_LINE5':
            b = line5_f12(*rest)
        else:
            raise KeyError(op)
        for _ in range(reps):
            f = c.f12_mul(f, b)
    return [x * R392 % P for k in range(6) for x in f[TOWER_TO_W[k]]]

BLS_OK, BLS_INVALID = 0, 1             # status codes of coop_final_verdict (BLS_OK, BLS_ERR_INVALID_SIGNATURE)


def coop_pow_x(f):
    """coop_pow_x restated on the oracle's tower with the Granger-Scott formulas, so that it is defined for any input; on the
    cyclotomic subgroup it is conj(f^|x|) (tests/test_hostsim_coop.py checks that)"""
    acc = f
    for i in range(62, -1, -1):
        acc = gs_sqr(acc)
        if (c.X_ABS >> i) & 1:
            acc = c.f12_mul(acc, f)
    return c.f12_conj(acc)


def final_verdict(f):
    """the status coop_final_verdict must return for S.f = f, from the oracle's final exponentiation; zero has no inverse: INVALID"""
    return BLS_OK if f != F12_ZERO and c.final_exponentiation(f) == F12_ONE else BLS_INVALID


def _coop_expected(op, cs, v, reps):
    tower = lambda f: [x * R392 % P for k in range(6) for x in f[TOWER_TO_W[k]]]
    prods = lambda k0, cnt: [x for t in range(cnt) for x in _f2mul_raw(v[k0 + 4 * t:k0 + 4 * t + 2], v[k0 + 4 * t + 2:k0 + 4 * t + 4])]
    if op == 'COOP_JOBS':            # res[k][j] for j < njobs; the other slots keep the fill (None: judged in check)
        out = prods(0, 12)
        for t in range(12):
            if t % 6 >= cs['par'][0]:
                out[2 * t] = out[2 * t + 1] = None
        return out
    f = f12_of_vecs(cs['vecs'][:12])
    if op == 'COOP_CONJ':
        return [v[k] if k < 6 else -v[k] for k in range(12)]
    if op == 'COOP_FINAL_VERDICT':
        return [None]
    if op == 'COOP_SQR_MUL_JOBS':
        return tower(c.f12_sqr(f)) + prods(12, 10)
    if op in ('COOP_MUL_LINE', 'COOP_LINE_MUL_JOBS'):
        b = line3_f12(*[f2_of_vecs(cs['vecs'][12 + 2 * k:14 + 2 * k]) for k in range(3)])
        for _ in range(reps):
            f = c.f12_mul(f, b)
        return tower(f) + (prods(18, 12) if op == 'COOP_LINE_MUL_JOBS' else [])
    if op == 'COOP_MUL':
        b = f12_of_vecs(cs['vecs'][12:24])
        for _ in range(reps):
            f = c.f12_mul(f, b)
    elif op == 'COOP_SQR':
        for _ in range(reps):
            f = c.f12_sqr(f)
    elif op == 'COOP_CYC_SQR':
        for _ in range(reps):
            f = gs_sqr(f)
    elif op == 'COOP_POW_X':
        f = coop_pow_x(f)
    elif op == 'COOP_FROB1':
        f = c.f12_frob(f, 1)
    elif op == 'COOP_FROB2':
        f = c.f12_frob(f, 2)
    elif op == 'COOP_FINAL_EASY':
        f = cyclotomic(f) if f != F12_ZERO else F12_ZERO       # fp12_inv(0) = 0
    else:
        raise KeyError(op)
    return tower(f)


_expected = {}


def check(op, cs, outs, reps=1):
    """assert that the output vectors of one case are right; the message names the operation and the case"""
    import point_cases
    if op in point_cases.ROWS:               # a point row: judged by the chord-and-tangent rule and the oracle's curve (tests/point_cases.py)
        return point_cases.check(op, cs, outs, reps)
    import miller_cases
    if op in miller_cases.ROWS:              # a step, merge or row operation: judged by the restated formulas (tests/miller_cases.py)
        return miller_cases.check(op, cs, outs, reps)
    tag = '%s%s, case "%s": ' % (op, ' x%d' % reps if reps > 1 else '', cs['name'])
    # (a lanes = 64 case run with another fill shares its operand vectors, and so its expected value, with the case of the list)
    key = (op, id(cs['vecs']), tuple(cs['par'][:-1]), reps) if op.startswith('COOP_') else (op, id(cs), reps)
    if key not in _expected:
        _expected[key] = expected(op, cs, reps)        # computed once, shared by every test that runs the case
    want = _expected[key]
    assert len(outs) == len(want), tag + 'output count'
    v0 = val(cs['vecs'][0])
    for k, (o, w) in enumerate(zip(outs, want)):
        if w is None:
            continue
        got = val(o)
        if op in ('FP_NORM', 'FP2_MUL_XI', 'FP2_CONJ', 'F12_PACK', 'COOP_CONJ'):
            assert got == w, tag + 'output %d is not the same integer: %d instead of %d' % (k, got, w)
        else:
            assert (got - w) % P == 0, tag + 'output %d is not congruent to the exact result (off by %d mod p)' % (k, (got - w) % P)
        if op in REDUCED_OUT or (op in COOP_REDUCED_F and k < 12):
            assert all(0 <= x <= M for x in o[:NL - 1]), tag + 'output %d: a limb outside [0, 2^28): %s' % (k, o)
            assert abs(got) * 100 <= 52 * P, tag + 'output %d: reduced value outside +-0.52 p: %.6f p' % (k, got / P)
        if op in MULT_OUT or (op in COOP_REDUCED_F and k >= 12) or op == 'COOP_JOBS':
            assert all(0 <= x <= M for x in o[:NL - 1]), tag + 'output %d: a limb outside [0, 2^28): %s' % (k, o)
            assert -P < 8 * got < 9 * P, tag + 'output %d: multiplier output outside (-p/8, p + p/8): %.6f p' % (k, got / P)
    def mult_out(o, what):
        assert all(0 <= x <= M for x in o[:NL - 1]) and -P < 8 * val(o) < 9 * P, tag + '%s is not a multiplier output (limbs in [0, 2^28), value in (-p/8, p + p/8)): %s' % (what, o)

    def reduced_out(o, what):
        assert all(0 <= x <= M for x in o[:NL - 1]) and abs(val(o)) * 100 <= 52 * P, tag + '%s is not a reduced value: %s' % (what, o)

    def normalised_out(o, what, vmax):
        assert all(-16 <= x <= M + 16 for x in o[:NL - 1]) and abs(val(o)) <= vmax * P, tag + '%s is not normalised within %s p: %s' % (what, vmax, o)
    neg = lambda o: [-x for x in o]
    if op in ('FP2_INV', 'FP2L_INV'):        # (a0 n, -(a1 n)): a product and a negated product
        mult_out(outs[0], 'c0')
        mult_out(neg(outs[1]), '-c1')
    if op == 'FP2L_MUL':                     # tower.cuh: "both return normalised limbs"; c0 = t0 - t1, c1 = m - t0 - t1 of three products
        normalised_out(outs[0], 'c0', 2.25)
        normalised_out(outs[1], 'c1', 3.375)
    if op == 'FP2L_SQR':                     # c0 a product, c1 twice a product after a carry pass
        mult_out(outs[0], 'c0')
        normalised_out(outs[1], 'c1', 2.25)
    if op == 'COOP_JOBS':                    # a slot the call does not compute still holds the fill word
        for k, (o, w) in enumerate(zip(outs, want)):
            assert w is not None or all(x == cs['par'][-1] for x in o), tag + 'result slot %d (job %d >= njobs) does not hold the fill word: %s' % (k, k // 2 % 6, o)
    if op == 'COOP_FINAL_VERDICT':
        f = f12_of_vecs(cs['vecs'][:12])
        st = _expected.setdefault(key + ('status',), None)
        if st is None:
            st = _expected[key + ('status',)] = final_verdict(f)
        assert list(outs[0]) == [st] + [0] * (NL - 1), tag + 'status %s, the oracle says %d' % (outs[0], st)
    if op == 'COOP_CONJ':                    # the same integers, the odd powers of w negated limb by limb
        assert [list(o) for o in outs] == conj_vecs(cs['vecs']), tag + 'limbs'
    if op in ('F12_POW_X', 'COOP_POW_X'):    # conj(accumulator): a reduced c0 and a limb-wise negated reduced c1 (tower order: vectors 6..11)
        for k, o in enumerate(outs):
            reduced_out(o if k < 6 else neg(o), 'vector %d%s' % (k, '' if k < 6 else ' negated'))
    if op in ('F12_FROB1', 'F12_FROB2', 'COOP_FROB1', 'COOP_FROB2'):     # the w^0 coefficient is copied (J = 2) or conjugated limb-wise (J = 1); the others are products by constants
        a0, a1 = cs['vecs'][0], cs['vecs'][1]
        assert list(outs[0]) == a0 and list(outs[1]) == (neg(a1) if op.endswith('FROB1') else a1), tag + 'limbs of the w^0 coefficient'
        for k in range(2, 12):
            mult_out(outs[k], 'vector %d' % k)
    if op == 'FP_NORM':
        assert all(-16 <= x <= M + 16 for x in outs[0][:NL - 1]), tag + 'limbs after the carry pass: %s' % outs[0]
    if op == 'F12_PACK':
        assert [list(o) for o in outs] == cs['vecs'], tag + 'the limbs changed in the pack / unpack round trip'
    if op == 'FP2_CONJ':
        assert list(outs[0]) == cs['vecs'][0] and list(outs[1]) == [-x for x in cs['vecs'][1]], tag + 'limbs'
    if op == 'FP2_MUL_XI':
        a0, a1 = cs['vecs'][0], cs['vecs'][1]
        assert list(outs[0]) == [x - y for x, y in zip(a0, a1)] and list(outs[1]) == [x + y for x, y in zip(a0, a1)], tag + 'limbs'
    if op == 'FP_CANON':
        assert val(outs[0]) == v0 % P and all(0 <= x <= M for x in outs[0]), tag + 'fp_canon: not the representative in [0, p) with exact limbs'
        assert outs[1][0] == (1 if v0 % P == 0 else 0), tag + 'fp_is_zero'
        words = sum((w & 0xffffffff) << (32 * i) for i, w in enumerate(outs[1][1:13]))
        assert words == v0 * pow(256, -1, P) % P, tag + 'fp_to_raw words'
    if op == 'FP_SQRT':
        x = v0 * R392_INV % P
        sq = c.fp_is_square(x)
        assert outs[1][0] == int(sq) and outs[1][1] == int(sq), tag + 'square flags %s for a %s' % (outs[1][:2], 'square' if sq else 'non-square')
        mult_out(outs[0], 'the root (a^((p+1)/4), computed either way)')
        if sq:
            r = elem_of(outs[0])
            assert r * r % P == x, tag + 'the root does not square to the operand'


# ---- line tables for k_millerf2s (blsgpu_debug_millerf): 68 entries of five Fp2 coefficients in the order c0, c2, c4, c3, c5
MILLER_ENTRIES = 68
MILLER_ADD_ENTRIES = (1, 4, 8, 18, 51)        # pairing.cuh miller_entry_is_add
LINE_ONE = [(1, 0)] + [(0, 0)] * 4
LINE_ZERO = [(0, 0)] * 5


def miller_tables():
    """[(name, 68 lines of five oracle Fp2)], deterministic"""
    if 'tables' in _cache_b:
        return _cache_b['tables']
    rng = random.Random(68)
    h = (P - 1) // 2
    rl = lambda: [(rng.randrange(P), rng.randrange(P)) for _ in range(5)]
    out = [('all lines 1', [LINE_ONE] * MILLER_ENTRIES)]
    for e in (0, 1, 2, 51, 67):
        t = [LINE_ONE] * MILLER_ENTRIES
        t[e] = rl()
        out.append(('one random line at entry %d (%s)' % (e, 'addition' if e in MILLER_ADD_ENTRIES else 'first' if e == 0 else 'doubling'), t))
    for e in (0, 3, 51):
        t = [rl() for _ in range(MILLER_ENTRIES)]
        t[e] = LINE_ZERO
        out.append(('the zero line at entry %d' % e, t))
    for k in range(5):
        t = []
        for e in range(MILLER_ENTRIES):
            cs = [(0, 0)] * 5
            cs[k] = (rng.randrange(1, P), rng.randrange(P))
            t.append(cs)
        out.append(('only coefficient %d non-zero in every line' % k, t))
    out.append(('coefficients at +-(p-1)/2', [[(h, P - h) if (e + k) % 2 else (P - h, h) for k in range(5)] for e in range(MILLER_ENTRIES)]))
    for i in range(5):
        out.append(('random table %d' % i, [rl() for _ in range(MILLER_ENTRIES)]))
    _cache_b['tables'] = out
    return out


_cache_b = {}


def miller_expected(table):
    """f <- L_0; for e = 1 .. 67: f <- f^2 unless entry e is an addition, then f <- f L_e; the result is conj(f)"""
    key = id(table)
    if key not in _cache_b:
        f = line5_f12(*table[0])
        for e in range(1, MILLER_ENTRIES):
            if e not in MILLER_ADD_ENTRIES:
                f = c.f12_sqr(f)
            f = c.f12_mul(f, line5_f12(*table[e]))
        _cache_b[key] = c.f12_conj(f)
    return _cache_b[key]


def miller_table_vecs(table):
    key = ('vecs', id(table))
    if key not in _cache_b:
        _cache_b[key] = [[(limbs_of_elem(x[0]), limbs_of_elem(x[1])) for x in line] for line in table]
    return _cache_b[key]


def check_miller(name, table, out):
    """one item's output of k_millerf2s (twelve limb vectors, tower order) against the oracle's tower"""
    tag = 'k_millerf2s, table "%s": ' % name
    want = miller_expected(table)
    got = f12_of_vecs(out)
    for k in range(6):
        assert got[k] == want[k], tag + 'coefficient of w^%d differs' % k
    for k, o in enumerate(out):            # the accumulator is reduced; the kernel negates c1 limb-wise when it conjugates
        l = o if k < 6 else [-x for x in o]
        assert all(0 <= x <= M for x in l[:NL - 1]) and abs(val(l)) * 100 <= 52 * P, tag + 'vector %d is not a (negated) reduced value: %s' % (k, o)


# ---- pairs for the shipped wave-cooperative kernels (blsgpu_debug_coop_pairing): chosen and judged with the oracle alone
def g2_negc():
    """-[c] g2, c = (1 - x)^-1 mod r: the constant of G2NEGC_LINES (tools/gen_g2_lines.py)"""
    return c.E2.neg(c.E2.mul(c.G2_GEN, pow(c.H_EFF_G1, -1, c.R)))


def largest_g1():
    """the point of E1(Fp) with the largest canonical x, and of its two y the larger one"""
    x = P - 1
    while not c.fp_is_square((x * x * x + 4) % P):
        x -= 1
    y = c.fp_sqrt((x * x * x + 4) % P)
    return (x, max(y, P - y))


def largest_g2():
    """the point of E2(Fp2) with x = (p - 1) + (p - 1 - t) u for the smallest t that gives one, and the y with the larger c1"""
    x = (P - 1, P - 1)
    while not c.f2_is_square(c.E2.rhs(x)):
        x = (x[0], x[1] - 1)
    y = c.f2_sqrt(c.E2.rhs(x))
    ny = c.f2_neg(y)
    return (x, y if (y[1], y[0]) > (ny[1], ny[0]) else ny)


def two_representatives(x):
    """the Montgomery residue of x lies in [0.48 p, 0.52 p]: both v and v - p are reduced forms of it"""
    v = x % P * R392 % P
    return 48 * P <= 100 * v <= 52 * P


def miller_walk_is_regular(q):
    """no step of the 63-iteration loop on Q is exceptional: T is never infinity, no doubling meets y = 0, and no addition meets
    T = +-Q"""
    t = q
    for bit in bin(c.X_ABS)[3:]:
        if t is None or t[1] == (0, 0):
            return False
        t = c.E2.dbl(t)
        if bit == '1':
            if t is None or t[0] == q[0]:
                return False
            t = c.E2.add(t, q)
    return t is not None


def pair_vecs(pairs, negative=()):
    """twelve limb vectors (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1 per pair) in reduced form, each the representative limbs_of_elem
    picks -- except the vectors named in `negative`: index i >= 0 takes the representative v - p, index -(i + 1) the one in [0, p)"""
    out = []
    for (px, py), ((qx0, qx1), (qy0, qy1)) in pairs:
        out += [limbs_of_elem(z) for z in (px, py, qx0, qx1, qy0, qy1)]
    for i in negative:
        k = i if i >= 0 else -(i + 1)
        v = val(out[k]) % P
        out[k] = limbs_of(v - P if i >= 0 else v)
        assert abs(val(out[k])) * 100 <= 52 * P
    return out


def pairing_cases():
    """[{'name', 'fixed_g2', 'pairs': two (P, Q) of oracle points, 'vecs': the twelve limb vectors}], deterministic.  For fixed_g2 = 1
    pair 1's Q is -g2, for 2 the constant of G2NEGC_LINES (the kernels take it from their line table)."""
    if 'pairs' in _cache_b:
        return _cache_b['pairs']
    rng = random.Random(4096)
    E1, E2, g1, g2, R = c.E1, c.E2, c.G1_GEN, c.G2_GEN, c.R
    a, b, sk, h = (rng.randrange(1, R) for _ in range(4))
    ag1, bg2, H, pk = E1.mul(g1, a), E2.mul(g2, b), E1.mul(g1, h), E2.mul(g2, sk)
    sig = E1.mul(H, sk)
    PL, QL = largest_g1(), largest_g2()
    PU, QU = c.map_to_curve_g1(rng.randrange(P)), c.map_to_curve_g2((rng.randrange(P), rng.randrange(P)))     # not cofactor-cleared
    fixed_q = {1: E2.neg(g2), 2: g2_negc()}
    sig2 = E1.mul(E1.mul(PU, c.H_EFF_G1), sk)
    out = []

    def add(name, fixed, pairs, negative=()):
        out.append({'name': 'fixed_g2 = %d: %s' % (fixed, name), 'fixed_g2': fixed, 'pairs': pairs, 'vecs': pair_vecs(pairs, negative)})
    add('subgroup points, product one', 0, [(ag1, bg2), (E1.neg(g1), E2.mul(g2, a * b % R))])
    add('subgroup points, product not one', 0, [(ag1, bg2), (H, pk)])
    add('P with the largest canonical coordinates', 0, [(PL, bg2), (ag1, pk)])
    add('Q with the largest canonical coordinates', 0, [(ag1, QL), (H, bg2)])
    add('the largest P and Q as pair 1', 0, [(H, bg2), (PL, QL)])
    add('points outside the subgroups', 0, [(PU, QU), (ag1, bg2)])
    add('the same P and Q in both pairs', 0, [(ag1, bg2), (ag1, bg2)])
    add('P and -P against the same Q, product one', 0, [(ag1, bg2), (E1.neg(ag1), bg2)])
    for fx in (1, 2):
        fq = fixed_q[fx]
        add('signature, product one', fx, [(H, pk), (sig, fq)] if fx == 1 else [(PU, pk), (sig2, fq)])
        add('another message, product not one', fx, [(ag1, pk), (sig, fq)])
        add('P with the largest canonical coordinates in both pairs', fx, [(PL, pk), (PL, fq)])
        add('Q with the largest canonical coordinates', fx, [(H, QL), (sig, fq)])
        add('points outside the subgroups', fx, [(PU, QU), (PL, fq)])
        add('the same P and Q in both pairs', fx, [(H, fq), (H, fq)])
    # a coordinate with two reduced representatives: the positive one beside the negative one (congruent results)
    t, found = g1, {}
    while len(found) < 2:
        t = E1.add(t, g1)
        for k in (0, 1):
            if k not in found and two_representatives(t[k]):
                found[k] = t
    u, qx = g2, None
    while qx is None:
        u = E2.add(u, g2)
        if two_representatives(u[0][0]):
            qx = u
    for fx in (0, 1, 2):
        second = (H, bg2 if fx == 0 else fixed_q[fx])
        for k, nm in ((0, 'P.x'), (1, 'P.y')):
            add('%s as its positive representative' % nm, fx, [(found[k], pk), second], (-(k + 1),))
            add('%s as its negative representative' % nm, fx, [(found[k], pk), second], (k,))
            if fx:       # ... and in pair 1, whose P scales the rows of the line table
                add('%s of pair 1 as its positive representative' % nm, fx, [(H, pk), (found[k], second[1])], (-(6 + k + 1),))
                add('%s of pair 1 as its negative representative' % nm, fx, [(H, pk), (found[k], second[1])], (6 + k,))
        add('Q.x.c0 as its positive representative', fx, [(ag1, qx), second], (-3,))
        add('Q.x.c0 as its negative representative', fx, [(ag1, qx), second], (2,))
    _cache_b['pairs'] = out
    return out


def pairing_expected(cs):
    """(the oracle's Miller value, its easy part, the status of the pairing check)"""
    key = ('pairing', id(cs))
    if key not in _cache_b:
        m = c.miller_loop(cs['pairs'])
        _cache_b[key] = (m, cyclotomic(m), BLS_OK if c.final_exponentiation(m) == F12_ONE else BLS_INVALID)
    return _cache_b[key]


def check_easy(cs, out):
    """one item's exported easy-part value (twelve limb vectors, tower order): miller_loop(pairs)^((p^6 - 1)(p^2 + 1)) exactly -- the
    Fp2 factors by which the kernel's projective lines differ from the oracle's affine ones vanish under p^6 - 1 -- and reduced"""
    tag = 'k_pairing_coop_easy, case "%s": ' % cs['name']
    want, got = pairing_expected(cs)[1], f12_of_vecs(out)
    for k in range(6):
        assert got[k] == want[k], tag + 'coefficient of w^%d differs' % k
    for k, o in enumerate(out):
        assert all(0 <= x <= M for x in o[:NL - 1]) and abs(val(o)) * 100 <= 52 * P, tag + 'vector %d is not a reduced value: %s' % (k, o)


CHAINS = ('FP_MUL', 'FP_SQR', 'FP2_MUL', 'FP2_SQR', 'F12_SH_SQR', 'F12_SH_MUL', 'F12_SH_MUL_LINE', 'F12_SH_MUL_2LINES', 'F12_SH_MUL_LINE5', 'F12_SH_CYC_SQR',
          'CYC_C_SQR', 'CYC_C_SQR_UNPACKED', 'CYC_C_SQR_KARA', 'COOP_MUL', 'COOP_SQR', 'COOP_MUL_LINE', 'COOP_CYC_SQR',
          'G1_ADD', 'G1_DBL', 'G1_MADD', 'G2L_ADD', 'G2L_DBL', 'G2L_MADD', 'G2Q_DBL', 'G2S_ADD', 'G2S_DBL', 'G2S_MADD',      # (point_cases.CHAINS)
          'MILLER1_ADD', 'MILLER1_DBL', 'MILLER2_ADD', 'MILLER2_DBL')                                                         # (miller_cases.CHAINS)
CHAIN_REPS = ((2, 1), (17, 5), (63, 11))       # (reps, stride through the list)


def chain_cases(op, stride):
    """the cases a chain runs on: every stride-th of the list (24 at the most), and for the squarings in the cyclotomic subgroup
    every element of that subgroup -- so that at each length, 63 included, non-trivial cyclotomic elements are squared"""
    import point_cases
    if op in point_cases.ROWS:               # P + Q, P + 2Q, ...: the marked cases (through the identity, from a doubling) and every stride-th
        return point_cases.chain_cases(op, stride)
    import miller_cases
    if op in miller_cases.ROWS:
        return miller_cases.chain_cases(op, stride)
    lst = build()[op]
    cases = lst[::stride][:24]
    if op in ('F12_SH_CYC_SQR', 'CYC_C_SQR', 'CYC_C_SQR_UNPACKED', 'CYC_C_SQR_KARA', 'COOP_CYC_SQR'):
        cases = [cs for cs in lst if cs['name'].startswith('cyclotomic')] + [cs for cs in cases if not cs['name'].startswith('cyclotomic')]
        assert sum(cs['name'].startswith('cyclotomic ') and cs['name'] != 'cyclotomic one' for cs in cases) >= 3
    return cases
