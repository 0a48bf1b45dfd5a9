"""Crafted Fp12 inputs of the final exponentiation (tests/test_gpu_finalexp.py, tests/test_finalexp_inputs.py) with the oracle's
verdict for each: OK when fin^(3 (p^12 - 1) / r) == 1, INVALID otherwise.

Families (oracle Fp12 tuples in w-power order; None is the zero element):
  Z  zero: not in Fp12*, so it can never be a valid Miller value.  The oracle's inversion refuses it, so its verdict is stated,
     not computed: INVALID.
  S  1, -1, random Fp2*, random Fp6* (the w^1, w^3, w^5 coefficients zero): the easy part maps every nonzero element of Fp6 to
     exactly 1, so every a^x of the hard part has a = 1, whose compressed squarings meet z2 = 0 -- the compressed chain declines
     and the plain chain answers.
  K  y^r and y^r s (s in Fp6*): the easy part leaves a nontrivial cyclotomic element, the compressed chain runs; OK.
  N  random y, and y^r z with z random (not an r-th power): INVALID.
  M  Miller values of a pair product whose pairing product is 1 (OK) and of one whose product is not (INVALID)."""
import random

import util
from util import c

P = c.P
OK, INVALID = 0, 1
ZERO_RECORD = bytes(576)


def rand_fp2_star(rng):
    while True:
        a = (rng.randrange(P), rng.randrange(P))
        if a != c.F2_ZERO:
            return a


def rand_f12(rng):
    return tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))


def rand_fp6_star(rng):
    """A random nonzero element of Fp6 = Fp2[v], v = w^2: only the even powers of w are set."""
    return (rand_fp2_star(rng), c.F2_ZERO, (rng.randrange(P), rng.randrange(P)), c.F2_ZERO, (rng.randrange(P), rng.randrange(P)), c.F2_ZERO)


def fp2_elem(a):
    return (a,) + (c.F2_ZERO,) * 5


def easy_part(f):
    """f^((p^6 - 1)(p^2 + 1)) as the oracle's final exponentiation begins."""
    g = c.f12_mul(c.f12_conj(f), c.f12_inv(f))
    return c.f12_mul(c.f12_frob(g, 2), g)


def verdict(f):
    """The oracle's verdict on a Fp12 value; 0 is not in Fp12* and is INVALID by definition (the oracle's inversion refuses it)."""
    if f is None or f == (c.F2_ZERO,) * 6:
        return INVALID
    return OK if c.final_exponentiation(f) == c.F12_ONE else INVALID


def record(f):
    return ZERO_RECORD if f is None else util.f12_record(f)


def family_pool(seed=7):
    """[(name, family, value)] -- a few members of every family (the values whose verdicts the tests compare)."""
    rng = random.Random(seed)
    pool = [('zero', 'Z', None),
            ('one', 'S', c.F12_ONE),
            ('minus_one', 'S', fp2_elem((P - 1, 0)))]
    for i in range(3):
        pool.append(('fp2_%d' % i, 'S', fp2_elem(rand_fp2_star(rng))))
    for i in range(3):
        pool.append(('fp6_%d' % i, 'S', rand_fp6_star(rng)))
    yr = [c.f12_pow(rand_f12(rng), c.R) for _ in range(3)]
    for i, v in enumerate(yr):
        pool.append(('y^r_%d' % i, 'K', v))
        pool.append(('y^r*s_%d' % i, 'K', c.f12_mul(v, rand_fp6_star(rng))))
    for i in range(4):
        pool.append(('y_%d' % i, 'N', rand_f12(rng)))
    for i, v in enumerate(yr):
        pool.append(('y^r*z_%d' % i, 'N', c.f12_mul(v, rand_f12(rng))))
    for i in range(2):
        a, b = rng.randrange(1, c.R), rng.randrange(1, c.R)
        Pa, Qb = c.E1.mul(c.G1_GEN, a), c.E2.mul(c.G2_GEN, b)
        # e(aG1, bG2) e(-abG1, G2) = 1;  e(aG1, bG2) e(abG1 + G1, -G2) != 1
        pool.append(('miller_valid_%d' % i, 'M', c.miller_loop([(Pa, Qb), (c.E1.neg(c.E1.mul(c.G1_GEN, a * b % c.R)), c.G2_GEN)])))
        pool.append(('miller_invalid_%d' % i, 'M', c.miller_loop([(Pa, Qb), (c.E1.mul(c.G1_GEN, (a * b + 1) % c.R), c.E2.neg(c.G2_GEN))])))
    return pool


def product(values):
    acc = c.F12_ONE
    for v in values:
        if v is None:
            return None
        acc = c.f12_mul(acc, v)
    return acc


def product_sets(k, rng):
    """{name: (values, expected verdict of their product)} for k records: a product equal to 1 in Fp12 (random a_i, the last
    the inverse of the running product), k elements of Fp6*, and each with one record zeroed or replaced by a random y."""
    ones = [rand_f12(rng) for _ in range(k - 1)]
    ones.append(c.f12_inv(product(ones)))
    fp6s = [rand_fp6_star(rng) for _ in range(k)]
    sets = {'one': ones, 'fp6': fp6s}
    for base, vals in list(sets.items()):
        j = rng.randrange(k)
        sets[base + '_zero%d' % j] = vals[:j] + [None] + vals[j + 1:]
        j = k - 1 - rng.randrange(min(k, 3))          # near the end: the odd halvings and the tree's padded groups
        sets[base + '_y%d' % j] = vals[:j] + [rand_f12(rng)] + vals[j + 1:]
    out = {}
    for name, vals in sets.items():
        prod = product(vals)
        assert name != 'one' or prod == c.F12_ONE
        out[name] = (vals, verdict(prod))
    return out
