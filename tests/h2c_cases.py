"""The shared case list of hash-to-curve BEHIND expand_message_xmd: chosen uniform bytes (what the expansion would have produced) and
the points they must map to, built from oracle/py alone, deterministic (seeded).

A case is {'name', 'group', 'uniform', 'u', 'Q', 'H', 'family', 'classes'}: 128 (G1) / 256 (G2) uniform bytes; with e_j the j-th
64-byte block as a big-endian integer, u0 = e_0 mod p, u1 = e_1 mod p for G1 and u0 = (e_0, e_1) mod p, u1 = (e_2, e_3) mod p for G2;
Q = map(u0) + map(u1) with map = the identity at a pole of the isogeny (RFC 9380 6.6.3); H = [1 - x] Q for G1 and
g2_clear_cofactor(Q) for G2.  Points are the oracle's affine tuples, None = the identity.  Expected values are computed once per
process (build() is cached): the Python clearing of G2 is slow.

Families (tests/test_h2c_cases.py proves the list sound and runs it through the host build; tests/test_gpu_h2c_map.py through every
kernel path):
  random      every byte random; the builder classifies each block position by the oracle -- g(x1) square or not, and whether sgn0(u)
              differs from sgn0 of the oracle's root of g(x) (the device picks its own root, so this is a stand-in for its sign flip:
              with 32 random items both outcomes of the device's own choice occur too) -- and asserts every class present
  edge        the edges of the 512-bit reduction in one block, random bytes in the others, moved through every block position
  zero        u = 0 in one position and in both (Q = 2 map(0): the addition doubles), written as 0, as p, as the largest multiple of p
  tv2         G1 only: u = +-sqrt(-1 / 11), the other inputs with tv2 = 0 (they exist because -1 / Z is a square in Fp; in Fp2 it is not)
  eqopp       u1 = u0 (same bytes, and u0 + k p): the addition doubles; u1 = -u0: Q and H are the identity
  sgn0        G2 only: u = (0, odd), (0, even), (even, 0), (odd, 0), (x, 0): sgn0 falls through to c1 when c0 = 0
  pole        G1 only: the 16 u whose SSWU point is a pole of the 11-isogeny (found by inverting SSWU at the five roots of the
              x-denominator, on both branches), in position 0, in position 1, in both (H is the identity)
The list is ordered round-robin over the families, so that exceptional items sit beside regular ones in any run of consecutive cases."""
import functools
import random

from oracle.py import bls381 as c
from oracle.py import iso_consts as iso

P = c.P
TOP = 1 << 512
MAXMULT = (TOP - 1) // P * P            # the largest multiple of p below 2^512

EDGES = [('0', 0), ('1', 1), ('p-1', P - 1), ('p', P), ('p+1', P + 1), ('2p', 2 * P), ('2^381', 1 << 381),
         ('2^384-1 (low 48 bytes ones, high 16 zero)', (1 << 384) - 1), ('2^384', 1 << 384), ('2^384+1', (1 << 384) + 1),
         ('2^512-1', TOP - 1), ('maxmult-1', MAXMULT - 1), ('maxmult', MAXMULT), ('maxmult+1', MAXMULT + 1),
         ('high 16 bytes ones, low 48 zero', ((1 << 128) - 1) << 384)]
assert all(0 <= v < TOP for _, v in EDGES)


# ---------------------------------------------------------------- polynomials over Fp (coefficient lists, low degree first)
def _trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _pmod(a, f):
    a = list(a)
    inv = pow(f[-1], -1, P)
    while len(a) >= len(f):
        k = a[-1] * inv % P
        off = len(a) - len(f)
        for i, fc in enumerate(f):
            a[off + i] = (a[off + i] - k * fc) % P
        a.pop()
    return _trim(a)


def _pmulmod(a, b, f):
    r = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = (r[i + j] + x * y) % P
    return _pmod(r, f)


def _ppowmod(a, e, f):
    r, a = [1], _pmod(a, f)
    while e:
        if e & 1:
            r = _pmulmod(r, a, f)
        a = _pmulmod(a, a, f)
        e >>= 1
    return r


def _pgcd(a, b):
    a, b = _trim(list(a)), _trim(list(b))
    while b:
        a, b = b, _pmod(a, b)
    inv = pow(a[-1], -1, P)
    return [x * inv % P for x in a]


def _psub(a, b):
    n = max(len(a), len(b))
    return _trim([((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % P for i in range(n)])


def fp_roots(f, rng):
    """the roots in Fp of the polynomial f (distinct-root part): gcd with x^p - x, then equal-degree splitting"""
    f = _trim([x % P for x in f])
    g = _pgcd(f, _psub(_ppowmod([0, 1], P, f), [0, 1]))
    roots, work = [], [g]
    while work:
        h = work.pop()
        if len(h) == 1:
            continue
        if len(h) == 2:
            roots.append(-h[0] * pow(h[1], -1, P) % P)
            continue
        while True:
            a = rng.randrange(P)
            d = _pgcd(h, _psub(_ppowmod([a, 1], (P - 1) // 2, h), [1]))
            if 1 < len(d) < len(h):
                q = list(h)
                # h / d by long division
                quo = [0] * (len(h) - len(d) + 1)
                inv = pow(d[-1], -1, P)
                while len(q) >= len(d):
                    k = q[-1] * inv % P
                    off = len(q) - len(d)
                    quo[off] = k
                    for i, dc in enumerate(d):
                        q[off + i] = (q[off + i] - k * dc) % P
                    q.pop()
                assert not _trim(q)
                work += [d, _trim(quo)]
                break
    return sorted(roots)


# ---------------------------------------------------------------- the G1 map's exceptional inputs
def _sswu_g1_x(u):
    return c._sswu(c.E1_ISO, iso.G1_Z, u, c.fp_is_square, c.fp_sqrt, c._sgn0_fp, 1)[0]


def g1_pole_preimages(rng):
    """every u in Fp whose SSWU point has an x-coordinate that is a root of the isogeny's x-denominator.  With t = Z u^2 and
    k = -A x / B: branch x = x1(u) is t^2 + t = 1 / (k - 1); branch x = t x1(u) is t^2 + (1 - k) t + (1 - k) = 0.  Candidates from both
    quadratics, kept when the oracle's SSWU really lands on the root."""
    A, B, Z = iso.G1_A, iso.G1_B, iso.G1_Z
    roots = fp_roots(iso.G1_ISO[1], rng)
    assert len(roots) == 5, 'the x-denominator of the 11-isogeny has five roots in Fp'
    us = set()
    for r in roots:
        assert c.fp_is_square(c.E1_ISO.rhs(r)), 'every root is the x-coordinate of a point of E1\'(Fp)'
        k = -A * r * pow(B, -1, P) % P
        quads = [(1, (1 - k) % P, (1 - k) % P)]
        if k != 1:
            quads.append((1, 1, -pow(k - 1, -1, P) % P))
        for qa, qb, qc in quads:
            disc = (qb * qb - 4 * qa * qc) % P
            s = c.fp_sqrt(disc)
            if s is None:
                continue
            for sg in (s, -s % P):
                t = (-qb + sg) * pow(2 * qa, -1, P) % P
                w = c.fp_sqrt(t * pow(Z, -1, P) % P)
                if w is None:
                    continue
                for u in (w, -w % P):
                    if _sswu_g1_x(u) == r:
                        us.add(u)
    us = sorted(us)
    assert len(us) == 16, len(us)
    assert all(c.map_to_curve_g1(u) is None for u in us)
    return us


def g1_tv2_zero_inputs():
    s = c.fp_sqrt(-pow(iso.G1_Z, -1, P) % P)
    assert s is not None and (iso.G1_Z * s * s + 1) % P == 0
    return s, -s % P


# ---------------------------------------------------------------- bytes <-> field elements, expected points
def block(e):
    assert 0 <= e < TOP
    return e.to_bytes(64, 'big')


def lift(u, rng):
    """a random 64-byte writing of the field element u: u + k p below 2^512"""
    return block(u + rng.randrange((TOP - 1 - u) // P + 1) * P)


def rand_block(rng):
    return bytes(rng.randrange(256) for _ in range(64))


def elements(group, uniform):
    e = [int.from_bytes(uniform[64 * j:64 * j + 64], 'big') % P for j in range(2 * group)]
    return (e[0], e[1]) if group == 1 else ((e[0], e[1]), (e[2], e[3]))


def expected(group, uniform):
    u0, u1 = elements(group, uniform)
    if group == 1:
        q = c.E1.add(c.map_to_curve_g1(u0), c.map_to_curve_g1(u1))
        return q, c.E1.mul(q, c.H_EFF_G1)
    q = c.E2.add(c.map_to_curve_g2(u0), c.map_to_curve_g2(u1))
    return q, c.g2_clear_cofactor(q)


def classify(group, u):
    """(g(x1) is a square, sgn0(u) differs from sgn0 of the oracle's root of g(x)) of one map, None at an exceptional input"""
    cv, Z = (c.E1_ISO, iso.G1_Z) if group == 1 else (c.E2_ISO, iso.G2_Z)
    is_sq, sqrt, sgn0, one = (c.fp_is_square, c.fp_sqrt, c._sgn0_fp, 1) if group == 1 else (c.f2_is_square, c.f2_sqrt, c._sgn0_f2, c.F2_ONE)
    zu2 = cv.mul_(Z, cv.sqr_(u))
    tv1 = cv.add_(cv.sqr_(zu2), zu2)
    if tv1 == cv.zero:
        return None
    x1 = cv.mul_(cv.mul_(cv.neg_(cv.b), cv.inv_(cv.a)), cv.add_(one, cv.inv_(tv1)))
    sq = bool(is_sq(cv.rhs(x1)))
    x = x1 if sq else cv.mul_(zu2, x1)
    return sq, sgn0(u) != sgn0(sqrt(cv.rhs(x)))


# ---------------------------------------------------------------- Jacobian RAW_PROJ bytes -> the oracle's affine tuple
RM_INV = pow(1 << 384, -1, P)


def _fp(b):
    return int.from_bytes(b, 'little') * RM_INV % P


def normalise(group, raw):
    """RAW_PROJ (Jacobian; 144 / 288 bytes, Montgomery words) -> affine (x, y) over the integers, None when Z = 0"""
    if group == 1:
        X, Y, Z = (_fp(raw[48 * k:48 * k + 48]) for k in range(3))
        if Z == 0:
            return None
        zi = pow(Z, -1, P)
        return (X * zi * zi % P, Y * zi * zi * zi % P)
    X, Y, Z = ((_fp(raw[96 * k:96 * k + 48]), _fp(raw[96 * k + 48:96 * k + 96])) for k in range(3))
    if Z == (0, 0):
        return None
    zi = c.f2_inv(Z)
    zi2 = c.f2_sqr(zi)
    return (c.f2_mul(X, zi2), c.f2_mul(Y, c.f2_mul(zi2, zi)))


# ---------------------------------------------------------------- the list
N_RANDOM = 32


def _families(group, rng):
    nb = 2 * group                      # 64-byte blocks per item
    per = group                         # blocks per field element u
    fam = {}

    def put(family, name, blocks):
        assert len(blocks) == nb
        fam.setdefault(family, []).append((name, b''.join(blocks)))

    def elem(u):
        """the blocks of one map's input: u in Fp, or (c0, c1) in Fp2"""
        return [lift(u, rng)] if group == 1 else [lift(u[0], rng), lift(u[1], rng)]

    def rand_elem():
        return [rand_block(rng) for _ in range(per)]

    def rand_u():
        return rng.randrange(1, P) if group == 1 else (rng.randrange(1, P), rng.randrange(1, P))

    def neg(u):
        return -u % P if group == 1 else (-u[0] % P, -u[1] % P)

    for i in range(N_RANDOM):
        put('random', 'random %d' % i, [rand_block(rng) for _ in range(nb)])
    for nm, v in EDGES:
        for pos in range(nb):
            put('edge', 'edge %s in block %d' % (nm, pos), [block(v) if j == pos else rand_block(rng) for j in range(nb)])
    zero_forms = [('0', 0), ('p', P), ('maxmult', MAXMULT)]
    for k, (nm, v) in enumerate(zero_forms):
        z = [block(v)] * per
        nm2, v2 = zero_forms[(k + 1) % 3]
        put('zero', 'u0 = 0 written as %s' % nm, z + rand_elem())
        put('zero', 'u1 = 0 written as %s' % nm, rand_elem() + z)
        put('zero', 'u0 = u1 = 0 written as %s and %s' % (nm, nm2), z + [block(v2)] * per)
    specials = []                        # exceptional inputs for the equal / opposite family
    if group == 1:
        s, ns = g1_tv2_zero_inputs()
        for nm, a, b in (('+s, random', s, None), ('-s, random', ns, None), ('random, +s', None, s), ('random, -s', None, ns),
                         ('+s, +s', s, s), ('+s, -s (identity)', s, ns), ('-s, +s (identity)', ns, s)):
            put('tv2', 'tv2 = 0: u = %s' % nm, (elem(a) if a is not None else rand_elem()) + (elem(b) if b is not None else rand_elem()))
        poles = g1_pole_preimages(rng)
        for i, u in enumerate(poles):
            put('pole', 'pole %d in position 0' % i, elem(u) + rand_elem())
            put('pole', 'pole %d in position 1' % i, rand_elem() + elem(u))
        for i in range(0, 16, 2):
            put('pole', 'poles %d and %d' % (i, (i + 5) % 16), elem(poles[i]) + elem(poles[(i + 5) % 16]))
        specials = [('tv2 = 0', s), ('a pole', poles[3])]
    else:
        odd, even = 2 * rng.randrange(1, P // 2) + 1, 2 * rng.randrange(1, P // 2)
        forms = [('(0, odd)', (0, odd)), ('(0, even)', (0, even)), ('(even, 0)', (even, 0)), ('(odd, 0)', (odd, 0)), ('(x, 0)', (rng.randrange(1, P), 0))]
        for nm, u in forms:
            put('sgn0', 'sgn0: u0 = %s' % nm, elem(u) + rand_elem())
            put('sgn0', 'sgn0: u1 = %s' % nm, rand_elem() + elem(u))
        specials = [('(0, odd)', (0, odd)), ('(x, 0)', forms[4][1])]
    for nm, u in [('random a', rand_u()), ('random b', rand_u())] + specials:
        same = elem(u)
        put('eqopp', 'u1 = u0 (%s), the same bytes' % nm, same + same)
        put('eqopp', 'u1 = u0 (%s), other bytes' % nm, elem(u) + elem(u))
        put('eqopp', 'u1 = -u0 (%s): the identity' % nm, elem(u) + elem(neg(u)))
        put('eqopp', 'u0 = -u1 (%s): the identity' % nm, elem(neg(u)) + elem(u))
    return fam


@functools.lru_cache(maxsize=None)
def build(group):
    """the case list of `group` (1 or 2), expected points included; the same list on every call"""
    rng = random.Random(0x68326300 + group)
    fam = _families(group, rng)
    order, names = [], sorted(fam, key=lambda f: -len(fam[f]))
    for k in range(max(len(v) for v in fam.values())):       # round-robin: the long families spread over the list
        for f in names:
            if k < len(fam[f]):
                order.append((f,) + fam[f][k])
    out = []
    for f, name, uniform in order:
        u0, u1 = elements(group, uniform)
        q, h = expected(group, uniform)
        out.append({'name': name, 'group': group, 'family': f, 'uniform': uniform, 'u': (u0, u1), 'Q': q, 'H': h,
                    'classes': (classify(group, u0), classify(group, u1))})
    present = {(pos, cl) for cs in out if cs['family'] == 'random' for pos, cl in enumerate(cs['classes'])}
    for pos in (0, 1):
        for sq in (False, True):
            for flip in (False, True):
                assert (pos, (sq, flip)) in present, ('class missing among the random cases', pos, sq, flip)
    return out


def take(lst, n, start, stride=1):
    """n cases of the list from `start` on, every `stride`-th, cyclically (stride coprime to the length: no case twice below len)"""
    return [lst[(start + i * stride) % len(lst)] for i in range(n)]


def check(cs, raw, uncleared, what=''):
    """one RAW_PROJ output against the case's expected point, exactly"""
    got = normalise(cs['group'], raw)
    want = cs['Q'] if uncleared else cs['H']
    assert got == want, '%s case "%s" (%s): got %r, want %r' % (what, cs['name'], 'Q' if uncleared else 'H', got, want)
