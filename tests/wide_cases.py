"""The row-wide engine (csrc/wide_engine.cuh) operation by operation: the runs that tests/test_gpu_wide_ops.py sends through the device
door blsgpu_debug_wide_steps, and what "right" means for each.  Pure Python: tests/test_wide_cases.py exercises all of it without a GPU.

A run: {'name', 'set' ('F12' / 'PT'), 'steps': [(operation, dst, a, b)] as the generator writes programs, 'reps', 'in_idx': the value
indices that take inputs, 'items': per item one sixteen-word vector per input, 'ops': the operation names it exercises}.  Expected
values come from tests/wide_tables_check.py sim_program on integers: a limb vector stands for the field element value / 2^392, and the
comparison is congruence modulo p -- exact, no tolerance.  check() also holds every output to the engine's output contract (what makes
it a legal operand of the next operation: words 14 and 15 zero, limbs 0..12 in the range a carry pass leaves, |value| < 0.6 p) and
every value outside the steps' destinations (the product scratch apart) to its initial words.

Inputs per operation: random elements, zeros, ones, values just inside +-0.6 p on the extreme limb patterns of tests/field_cases.py, and
an ALIGNED item derived from the operation's own table: signs chosen so that the widest product row and the heaviest linear row sum
terms of one sign -- the case that takes a (2,2) product row's columns to 2^61.8 of the 2^62 they may reach."""
import itertools
import os
import random

import field_cases as fc
import util
import wide_tables_check as chk
from util import P, val, limbs_of, limbs_of_elem, elem_of, NL, R392

g = chk.g
c = util.c
DST, SA, SB, TMP, CONST = g.DST, g.SA, g.SB, g.TMP, g.CONST
LIMB_LO, LIMB_HI = -8, 2**28 + 7            # what one carry pass leaves of limbs below 2^31 in magnitude (wide.cuh w_norm)
HANDOVER = ('ACQ', 'PUB', 'ACQF', 'PUBF')
FILLS = fc.FILLS
COUNTS = (1, 2, 5)
CHAIN_REPS = (2, 17)


class TableSet:
    def __init__(self, name, number, ops, lay, programs, builtins):
        self.name, self.number, self.ops, self.lay, self.programs = name, number, ops, lay, dict(programs)
        self.by = {o.name: o for o in ops}
        self.ids = {o.name: k for k, o in enumerate(ops)}
        for k, b in enumerate(builtins):
            self.ids[b] = len(ops) + k
        self.nv = lay.count
        tb = lay.base['TMP']
        self.tmp = range(tb, tb + 2 * (max(o.ntmp for o in ops) + 1))
        consts = chk.consts24() if name == 'F12' else chk.psi_consts()
        self.consts = {lay.base['CONST'] + k: x for k, x in enumerate(consts)}

    def words(self, steps):
        """[(operation id, dst, a, b)] as numbers: the door's program"""
        return [(self.ids[n], self.lay.ref(d), self.lay.ref(x), self.lay.ref(y)) for n, d, x, y in steps]


SETS = {'F12': TableSet('F12', 0, g.OPS, g.layout_f12(), g.PROGRAMS, ('FPINV',) + HANDOVER),
        'PT': TableSet('PT', 1, g.OPS_PT, g.layout_pt(), g.PROGRAMS_PT, ())}
ALL_OPS = [('F12', o.name) for o in g.OPS] + [('F12', 'FPINV')] + [('PT', o.name) for o in g.OPS_PT]


# ---- what an operation reads and writes, from its table
def reads(op):
    """({offsets read from A}, {offsets read from B})"""
    ra, rb = set(), set()
    for a, b, _ in op.prods:
        for _, i in a + b:
            if (i >> 12) == SA:
                ra.add(i & 0xfff)
            elif (i >> 12) == SB:
                rb.add(i & 0xfff)
    for terms, _ in op.lins:
        ra |= {i & 0xfff for _, i in terms if (i >> 12) == SA}
    return ra, rb


def writes(op):
    return {o & 0xfff for _, o in op.lins}


def step_io(ts, step):
    """(value indices read, value indices written) of one program step"""
    n, d, x, y = step
    rd, ra, rb = ts.lay.ref(d), ts.lay.ref(x), ts.lay.ref(y)
    if n == 'FPINV':
        return {ra}, {rd}
    op = ts.by[n]
    oa, ob = reads(op)
    return {ra + o for o in oa} | {rb + o for o in ob}, {rd + o for o in writes(op)}


def program_io(ts, steps):
    """(values a program reads before it writes them, values it writes)"""
    need, made = set(), set()
    for st in steps:
        r, w = step_io(ts, st)
        need |= {v for v in r if v not in made and v not in ts.consts}
        made |= w
    return need, made


_shapes = {}


def shapes(ts):
    if ts.name not in _shapes:
        _shapes[ts.name] = _find_shapes(ts)
    return _shapes[ts.name]


def _find_shapes(ts):
    """{operation: [step]}: one real step of the set's programs per aliasing shape in which the operation is used -- dst = a, dst = b,
    a = b, all apart (a reference the operation does not use does not count)"""
    out = {}
    for _, prog in ts.programs.items():
        for st in prog:
            n, d, x, y = st
            if n in HANDOVER:
                continue
            rd, ra, rb = ts.lay.ref(d), ts.lay.ref(x), ts.lay.ref(y)
            uses_b = n != 'FPINV' and bool(reads(ts.by[n])[1])
            key = (rd == ra, uses_b and rd == rb, uses_b and ra == rb)
            out.setdefault(n, {}).setdefault(key, st)
    # an operation of the table that no program uses (LSCALE0, LSCALE1: the packed LSCALE<p>X<n> forms replaced them) runs on the
    # references of the used operation whose name is the closest: its sibling's arrays
    for n in ts.by:
        if n not in out:
            near = max(out, key=lambda m: (len(os.path.commonprefix([m, n])), -len(m)))
            assert len(os.path.commonprefix([near, n])) >= 4, (n, near)
            out[n] = {k: (n,) + st[1:] for k, st in out[near].items()}
            for st in out[n].values():
                rd, wr = step_io(ts, st)
                assert max(rd | wr) < ts.nv and not (rd | wr) & (set(ts.tmp) | set(ts.consts))
    return {n: list(d.values()) for n, d in out.items()}


# ---- input values
def vec16(l):
    assert len(l) == NL
    return list(l) + [0, 0]


def in_contract(v):
    """the engine's input contract: what its own outputs satisfy, with the limb range taken as a magnitude (the column bounds of the
    multiplier are symmetric): words 14, 15 zero, |limb| <= 2^28 + 7 below the top, |value| < 0.6 p"""
    return len(v) == 16 and v[14] == 0 and v[15] == 0 and all(abs(x) <= LIMB_HI for x in v[:NL - 1]) and 5 * abs(val(v[:NL])) < 3 * P


def near_limit(low_limbs, sign):
    """the vector with these limbs 0..12 whose value is the closest to sign * 0.6 p from inside"""
    low = val(list(low_limbs) + [0])
    lim = (3 * P - 1) // 5                  # the largest integer below 0.6 p
    top = (lim - low) >> 364 if sign > 0 else -((lim + low) >> 364)
    v = list(low_limbs) + [top]
    assert 5 * abs(val(v)) < 3 * P and 5 * abs(val(v) + sign * 2**364) >= 3 * P
    return vec16(v)


def extreme_vectors():
    """values at +-(just under 0.6 p) on limbs at the two ends of the carry-pass range, all positive, all negative, alternating"""
    out = []
    for nm, l in fc.extreme_operands(LIMB_HI, 0) + fc.extreme_operands(-LIMB_LO, 0):
        for sign in (1, -1):
            out.append(('%s, value %s0.6 p' % (nm, '-' if sign < 0 else ''), near_limit(l[:NL - 1], sign)))
    return out


EXTREMES = extreme_vectors()
BIG = near_limit(fc.pattern(LIMB_HI, (1,), 0)[:NL - 1], 1)        # every limb maximal, the value just under 0.6 p
BIG_NEG = [-x for x in BIG]


def signed_big(s):
    return BIG if s > 0 else BIG_NEG


def aligned_signs(op, rng):
    """signs (+-1 per (slot, offset) the operation reads) that (1) make every term of the product row with the largest
    (sum|ca|)(sum|cb|) the same sign on both sides, if any such row allows it, and (2) with the signs left free push the linear row
    with the largest sum|k| as far to one side as they can.  Returns (signs, product row, linear row)"""
    key = lambda i: (i >> 12, i & 0xfff)  # noqa: E731
    variables = sorted({key(i) for a, b, _ in op.prods for _, i in a + b if (i >> 12) in (SA, SB)} |
                       {key(i) for t, _ in op.lins for _, i in t if (i >> 12) == SA})
    fixed, prow = {}, None
    rows = sorted(op.prods, key=lambda r: -sum(abs(k) for k, _ in r[0]) * sum(abs(k) for k, _ in r[1]))
    for a, b, o in rows:
        if sum(abs(k) for k, _ in a) * sum(abs(k) for k, _ in b) < sum(abs(k) for k, _ in rows[0][0]) * sum(abs(k) for k, _ in rows[0][1]):
            break
        want = {}
        ok = True
        for k, i in a + b:
            if (i >> 12) == CONST:
                continue
            s = 1 if k > 0 else -1
            ok = ok and want.setdefault(key(i), s) == s
        # a side that holds a constant cannot be steered: it still counts as aligned when it is a single term
        ok = ok and all(len(side) == 1 or all((i >> 12) != CONST for _, i in side) for side in (a, b))
        if ok:
            fixed, prow = want, (a, b, o)
            break
    lrow = max(op.lins, key=lambda r: sum(abs(k) for k, _ in r[0])) if op.lins else None
    free = [v for v in variables if v not in fixed]
    by_out = {o: (a, b) for a, b, o in op.prods}

    def weight(signs):
        side = lambda t: sum(k * (signs[key(i)] if (i >> 12) != CONST else 1) for k, i in t)  # noqa: E731
        tot = 0
        for k, i in lrow[0]:
            tot += k * (side(by_out[i][0]) * side(by_out[i][1]) if (i >> 12) == TMP else signs[key(i)])
        return abs(tot)
    signs = dict(fixed)
    signs.update({v: 1 for v in free})
    if lrow is not None and free:
        if len(free) <= 12:
            best = max(itertools.product((1, -1), repeat=len(free)), key=lambda s: weight({**fixed, **dict(zip(free, s))}))
            signs.update(dict(zip(free, best)))
        else:                                                   # hill climbing from a few starts
            best_w = -1
            for _ in range(8):
                cur = {**fixed, **{v: rng.choice((1, -1)) for v in free}}
                w, moved = weight(cur), True
                while moved:
                    moved = False
                    for v in free:
                        cur[v] = -cur[v]
                        w2 = weight(cur)
                        if w2 > w:
                            w, moved = w2, True
                        else:
                            cur[v] = -cur[v]
                if w > best_w:
                    best_w, signs = w, dict(cur)
    return signs, prow, lrow


def product_columns(ts, step, item_map, row):
    """the 27 column sums of one product row of a step on integers: what the device accumulates in 64 bits"""
    _, d, x, y = step
    base = {SA: ts.lay.ref(x), SB: ts.lay.ref(y)}
    a, b, _ = row

    def side(t):
        out = [0] * NL
        for k, i in t:
            v = limbs_of(ts.consts[ts.lay.base['CONST'] + (i & 0xfff)] * R392 % P) if (i >> 12) == CONST else item_map[base[i >> 12] + (i & 0xfff)][:NL]
            out = [p + k * q for p, q in zip(out, v)]
        return out
    A, B = side(a), side(b)
    return [sum(A[i] * B[k - i] for i in range(NL) if 0 <= k - i < NL) for k in range(2 * NL - 1)]


# ---- the device's integer arithmetic of one linear row (wide.cuh w_mul_cols, w_redc_cols; wide_engine.cuh w_finish's first pass)
MASK = (1 << 28) - 1
P_LIMBS = [(P >> (28 * i)) & MASK for i in range(NL - 1)] + [P >> (28 * (NL - 1))]
N0INV = (-pow(P, -1, 1 << 28)) % (1 << 28)


def carried_columns(cols):
    """w_mul_cols: each 64-bit column leaves its low 28 bits, hands the next 28 one column up and the signed rest two up"""
    out = [0] * 29
    for k, x in enumerate(cols + [0]):
        assert abs(x) < 2**63
        if k < 26:
            out[k] += x & MASK
            out[k + 1] += (x >> 28) & MASK
            out[k + 2] += x >> 56
        else:
            out[k] += x & MASK
            out[k + 1] += x >> 28
    assert out[28] == 0 and all(abs(x) < 2**31 for x in out)
    return out[:28]


def limb_sums(ts, step, item_map, lin_row):
    """the fourteen 64-bit limb sums that a linear row of a step hands to w_finish, and the quotient digits of its reduction"""
    op = ts.by[step[0]]
    by_out = {o: (a, b, o) for a, b, o in op.prods}
    base_a = ts.lay.ref(step[2])
    cols, reduced = [0] * 28, False
    for k, i in lin_row[0]:
        if (i >> 12) == TMP:
            reduced = True
            cols = [x + k * y for x, y in zip(cols, carried_columns(product_columns(ts, step, item_map, by_out[i])))]
        else:
            z = item_map[base_a + (i & 0xfff)]
            cols = [x + (k * z[j - NL] if j >= NL else 0) for j, x in enumerate(cols)]
    if not reduced:
        return cols[NL:], []
    assert all(abs(x) < 2**62 for x in cols)
    cy, qs = 0, []
    for s_ in range(NL):
        col = cols[s_] + cy
        q = (col * N0INV) & MASK
        qs.append(q)
        for i in range(NL):
            cols[s_ + i] += q * P_LIMBS[i]
        cy = (col + q * P_LIMBS[0]) >> 28
    acc = cols[NL:]
    acc[0] += cy
    return acc, qs


def first_pass(acc):
    """limbs 0..12 after w_finish's first carry pass: the low 28 bits plus the neighbour's carry"""
    return [(acc[j] & MASK) + ((acc[j - 1] >> 28) if j else 0) for j in range(NL - 1)]


def maximal_quotient_pairs(rng, count):
    """pairs (a, b) of legal operands (exact limbs, |a| < 2^200, |b| < 0.6 p) with a b = m p (mod 2^392) for a small m: every quotient digit
    of the Montgomery reduction of a b but the lowest is 2^28 - 1, the reduced columns reach 2^58.9, and limb 1 after w_finish's first carry
    pass passes 2^31 -- the inputs that a 32-bit pass gets wrong"""
    out = []
    while len(out) < count:
        a = (rng.getrandbits(200) | 1) * rng.choice((1, -1))
        b = rng.randrange(1, 50) * P * pow(a, -1, R392) % R392
        for x in (b, b - R392):
            if 5 * abs(x) < 3 * P:
                cols = [sum(limbs_of(a)[i] * limbs_of(x)[k - i] for i in range(NL) if 0 <= k - i < NL) for k in range(2 * NL - 1)]
                if max(first_pass(_reduce_columns(carried_columns(cols)))) >= 2**31:
                    out.append((a, x))
    return out


def _reduce_columns(cols):
    cols, cy = list(cols), 0
    for s_ in range(NL):
        col = cols[s_] + cy
        q = (col * N0INV) & MASK
        for i in range(NL):
            cols[s_ + i] += q * P_LIMBS[i]
        cy = (col + q * P_LIMBS[0]) >> 28
    return [cols[NL] + cy] + cols[NL + 1:]


QUOTIENT_PAIRS = maximal_quotient_pairs(random.Random(9), 4)


def quotient_items(ts, step, need):
    """for a linear row that holds, with coefficient +-1, a product of two single values with coefficients +-1: those two values a pair of
    QUOTIENT_PAIRS and every other input zero, so that the row reduces exactly +- a b"""
    op = ts.by[step[0]]
    base = {SA: ts.lay.ref(step[2]), SB: ts.lay.ref(step[3])}
    by_out = {o: (a, b) for a, b, o in op.prods}
    for terms, _ in op.lins:
        for k, i in terms:
            if (i >> 12) != TMP or abs(k) != 1:
                continue
            a, b = by_out[i]
            if len(a) == 1 and len(b) == 1 and abs(a[0][0]) == 1 and abs(b[0][0]) == 1 and (a[0][1] >> 12) != CONST and (b[0][1] >> 12) != CONST:
                va, vb = base[a[0][1] >> 12] + (a[0][1] & 0xfff), base[b[0][1] >> 12] + (b[0][1] & 0xfff)
                if va == vb:
                    continue
                out = []
                for n, (x, y) in enumerate(QUOTIENT_PAIRS):
                    m = {v: [0] * 16 for v in need}
                    m[va], m[vb] = vec16(limbs_of(x)), vec16(limbs_of(y))
                    if max(first_pass(limb_sums(ts, step, m, (terms, 0))[0])) >= 2**31:
                        out.append(('every quotient digit maximal %d' % n, m))
                if out:
                    return out
    return []


# ---- runs of one operation
def op_items(ts, step, rng):
    """(in_idx, [(name, {value index: vector})]) for one step: every input class"""
    n = step[0]
    need = sorted(step_io(ts, step)[0] - set(ts.consts))
    items = []
    if n == 'FPINV':
        (v,) = need
        for nm, x in (('0', 0), ('1', 1), ('p - 1', P - 1), ('2', 2), ('random', rng.randrange(P)), ('random', rng.randrange(P))):
            items.append((nm, {v: vec16(limbs_of_elem(x))}))
            m = x % P * R392 % P
            items.append((nm + ', negative representative', {v: vec16(limbs_of(m - P))}))
            items.append((nm + ', lazy limbs', {v: vec16(fc.lazy(m, 1, rng))}))
            items.append((nm + ', lazy limbs, + p', {v: vec16(fc.lazy(m + P, 1, rng))}))
        return need, items
    for k in range(3):
        items.append(('random %d' % k, {v: vec16(limbs_of_elem(rng.randrange(P))) for v in need}))
    items.append(('zeros', {v: [0] * 16 for v in need}))
    items.append(('ones', {v: vec16(limbs_of_elem(1)) for v in need}))
    items.append(('integer ones', {v: vec16(limbs_of(1)) for v in need}))
    for k, (nm, e) in enumerate(EXTREMES):                      # every input on the same pattern
        items.append(('all inputs: ' + nm, {v: list(e) for v in need}))
    for k in range(len(EXTREMES)):                              # neighbouring inputs on different patterns
        items.append(('mixed extremes %d' % k, {v: list(EXTREMES[(5 * k + 3 * j) % len(EXTREMES)][1]) for j, v in enumerate(need)}))
    signs, _, _ = aligned_signs(ts.by[n], rng)
    base = {SA: ts.lay.ref(step[2]), SB: ts.lay.ref(step[3])}
    al = {v: BIG for v in need}
    for (slot, off), s in sorted(signs.items(), reverse=True):  # where a = b names one value twice the first operand's choice holds
        al[base[slot] + off] = signed_big(s)
    items.append(('aligned', al))
    items.append(('aligned, negated', {v: [-x for x in l] for v, l in al.items()}))
    items += quotient_items(ts, step, need)
    return need, items


def make_run(ts, name, steps, in_idx, items, reps=1, ops=None):
    return {'name': name, 'set': ts.name, 'steps': list(steps), 'reps': reps, 'in_idx': list(in_idx),
            'items': [[list(m[v]) for v in in_idx] for _, m in items], 'item_names': [nm for nm, _ in items],
            'ops': sorted(ops if ops is not None else {st[0] for st in steps})}


def op_runs(set_name, op_name, seed=1):
    """one run per aliasing shape in which the set's programs use the operation, all input classes as its items"""
    ts = SETS[set_name]
    rng = random.Random('%s %s %d' % (set_name, op_name, seed))
    out = []
    for step in shapes(ts)[op_name]:
        need, items = op_items(ts, step, rng)
        out.append(make_run(ts, '%s %r' % (op_name, step[1:]), [step], need, items))
    return out


# ---- sequences: verbatim slices of the generated programs (hand-over built-ins dropped)
def _jac1(pt, rng):
    z = rng.randrange(1, P)
    return [pt[0] * z * z % P, pt[1] * z * z * z % P, z]


def _jac2(q, rng):
    z = (rng.randrange(1, P), rng.randrange(P))
    z2 = c.f2_sqr(z)
    return list(c.f2_mul(q[0], z2)) + list(c.f2_mul(q[1], c.f2_mul(z2, z))) + list(z)


def _elems(ts, array, off, xs):
    b = ts.lay.ref((array, off))
    return {b + k: vec16(limbs_of_elem(x)) for k, x in enumerate(xs)}


def _fill_needed(ts, steps, m):
    """a program's remaining inputs (values it reads before writing that the case does not set) are zero"""
    need, _ = program_io(ts, steps)
    for v in need:
        m.setdefault(v, [0] * 16)
    return sorted(m)


def point_sets(rng):
    """(name, sixteen G1 points, sixteen G2 points, a G1 pair, a G2 pair): the largest coordinates, and random ones"""
    big1, big2 = fc.largest_g1(), fc.largest_g2()
    r1 = [c.E1.mul(c.G1_GEN, rng.randrange(1, c.R)) for _ in range(16)]
    r2 = [c.E2.mul(c.G2_GEN, rng.randrange(1, c.R)) for _ in range(16)]
    return [('largest coordinates', [big1] * 8 + [c.E1.neg(big1)] * 3 + r1[:5], [big2] * 8 + [c.E2.neg(big2)] * 3 + r2[:5], (big1, r1[0]), (big2, r2[0])),
            ('random', r1, r2, (r1[1], r1[2]), (r2[1], r2[2]))]


def pairing_inputs(ts, p0, q0, p1, q1, rng):
    m = {}
    m.update(_elems(ts, 'F', 0, chk.flat(c.F12_ONE)))
    m.update(_elems(ts, 'P', 0, _jac1(p0, rng) + [0] + _jac1(p1, rng) + [0]))
    m.update(_elems(ts, 'PT0', 6, _jac2(q0, rng)))
    m.update(_elems(ts, 'PT1', 6, _jac2(q1, rng)))
    return m


def sequence_runs(seed=5):
    rng = random.Random(seed)
    f12, pt = SETS['F12'], SETS['PT']
    sets_ = point_sets(rng)
    runs = []
    # one Miller doubling step and one addition step of both pairs, with the line scaling and MUL_LINE of the iterations that use them:
    # slices of PAIR_GENERAL (PPREP; per pair QPREP A B C, PDBL1 PDBL2 COPY6, PADD1..4 COPY6, PDBL1 PDBL2 COPY6; the first two iterations)
    prog = f12.programs['PAIR_GENERAL']
    n_kl = len(g.prog_key_lines(0))
    k0, k1, km = 2, 2 + n_kl, 2 + 2 * n_kl
    steps = prog[0:2] + prog[k0:k0 + 14] + prog[k1:k1 + 14] + prog[km:km + 10]
    assert [s[0] for s in prog[k0:k0 + 14]] == ['QPREPA', 'QPREPB', 'QPREPC', 'PDBL1', 'PDBL2', 'COPY6', 'PADD1', 'PADD2', 'PADD3', 'PADD4', 'COPY6', 'PDBL1', 'PDBL2', 'COPY6']
    assert [s[0] for s in prog[km:km + 10]] == ['LSCALE01', 'MUL_LINE', 'MUL_LINE'] * 2 + ['SQR', 'LSCALE01', 'MUL_LINE', 'MUL_LINE']
    items = []
    for nm, _, _, (a1, b1), (a2, b2) in sets_:
        items.append((nm, pairing_inputs(f12, a1, a2, b1, b2, rng)))
    idx = sorted(set().union(*[set(_fill_needed(f12, steps, m)) for _, m in items]))
    runs.append(make_run(f12, 'Miller doubling and addition steps', steps, idx, items))
    # a sixteen-point sum of each group, Jacobian in and out
    for grp, name in ((1, 'G1_JJ'), (2, 'G2_JJ')):
        steps = pt.programs[name]
        items = []
        for nm, p1s, p2s, _, _ in sets_:
            m = {}
            for i, q in enumerate(p1s if grp == 1 else p2s):
                o = g.g1_point_off(i) if grp == 1 else g.g2_point_off(i)
                m.update(_elems(pt, 'L0', o, _jac1(q, rng) if grp == 1 else _jac2(q, rng)))
            items.append((nm, m))
        idx = sorted(set().union(*[set(_fill_needed(pt, steps, m)) for _, m in items]))
        runs.append(make_run(pt, 'sixteen-point sum %s' % name, steps, idx, items))
    # the G2 cofactor clearing
    steps = pt.programs['G2_CLEAR']
    items = [(nm, _elems(pt, 'R0', 0, _jac2(pr[0], rng))) for nm, _, _, _, pr in sets_]
    items.append(('a point outside the subgroup', _elems(pt, 'R0', 0, _jac2(c.map_to_curve_g2((rng.randrange(P), rng.randrange(P))), rng))))
    idx = sorted(set().union(*[set(_fill_needed(pt, steps, m)) for _, m in items]))
    runs.append(make_run(pt, 'G2 cofactor clearing', steps, idx, items))
    # the isogeny chain of hash-to-G1 and the sum of the two mapped points: the first ten steps of G1_HASH_TAIL
    from oracle.py import iso_consts
    steps = pt.programs['G1_HASH_TAIL'][:10]
    assert [s[0] for s in steps[:8]] == ['C1ISOP1', 'C1ISOP2', 'C1ISOP3', 'C1ISOP4', 'C1ISOM', 'C1ISOK', 'C1ISOA1', 'C1ISOA2']
    items = []
    for nm, us in (('largest u', (P - 1, P - 2)), ('random u', (rng.randrange(P), rng.randrange(P)))):
        m = {}
        for k, u in enumerate(us):
            q = c._sswu(c.E1_ISO, iso_consts.G1_Z, u, c.fp_is_square, c.fp_sqrt, c._sgn0_fp, 1)
            d = rng.randrange(1, P)
            o = g.ISO_STRIDE * k
            m.update(_elems(pt, 'ISO', o + g.ISO_XN, [q[0] * d % P]))
            m.update(_elems(pt, 'ISO', o + g.ISO_XD, [d]))
            m.update(_elems(pt, 'ISO', o + g.ISO_Y, [q[1]]))
        items.append((nm, m))
    idx = sorted(set().union(*[set(_fill_needed(pt, steps, m)) for _, m in items]))
    runs.append(make_run(pt, 'isogeny chain', steps, idx, items))
    return runs


def chain_runs(seed=6):
    """reps in (2, 17): MUL and SQR with an aliased accumulator, CYC_SQR on a cyclotomic element, PDBL1 PDBL2 on a point"""
    rng = random.Random(seed)
    f12 = SETS['F12']
    rnd12 = lambda: tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))  # noqa: E731
    runs = []
    for reps in CHAIN_REPS:
        items = []
        for k in range(3):
            m = _elems(f12, 'ACC', 0, chk.flat(rnd12()))
            m.update(_elems(f12, 'F', 0, chk.flat(rnd12())))
            items.append(('random %d' % k, m))
        items.append(('extremes', {**{f12.lay.ref(('ACC', k)): list(EXTREMES[k % len(EXTREMES)][1]) for k in range(12)},
                                   **{f12.lay.ref(('F', k)): list(EXTREMES[(k + 5) % len(EXTREMES)][1]) for k in range(12)}}))
        idx = sorted(items[0][1])
        runs.append(make_run(f12, 'MUL chain x%d' % reps, [('MUL', 'ACC', 'ACC', 'F')], idx, items, reps))
        idx = sorted(f12.lay.ref(('F', k)) for k in range(12))
        runs.append(make_run(f12, 'SQR chain x%d' % reps, [('SQR', 'F', 'F', 'F')], idx, [(nm, {v: m[v] for v in idx}) for nm, m in items], reps))
        cyc = [(('cyclotomic %d' % k), _elems(f12, 'ACC', 0, chk.flat(fc.cyclotomic(rnd12())))) for k in range(3)]
        cyc.append(('one', _elems(f12, 'ACC', 0, chk.flat(c.F12_ONE))))
        runs.append(make_run(f12, 'CYC_SQR chain x%d' % reps, [('CYC_SQR', 'ACC', 'ACC', 'ACC')], sorted(cyc[0][1]), cyc, reps))
        pts = []
        for nm, q in (('largest coordinates', fc.largest_g2()), ('random', c.E2.mul(c.G2_GEN, rng.randrange(1, c.R)))):
            lam = (rng.randrange(1, P), rng.randrange(P))
            hom = list(c.f2_mul(q[0], lam)) + list(c.f2_mul(q[1], lam)) + list(lam)
            pts.append((nm, _elems(f12, 'PT0', g.PT_T, hom)))
        steps = [('PDBL1', 'PT0', 'PT0', 'PT0'), ('PDBL2', 'PT0', 'PT0', 'PT0')]
        idx = sorted(set().union(*[set(_fill_needed(f12, steps, m)) for _, m in pts]))
        runs.append(make_run(f12, 'PDBL chain x%d' % reps, steps, idx, pts, reps))
    return runs


def pairing_run(seed=7):
    """the whole of PAIR_GENERAL, once: a valid and an invalid signature; (run, expected T == 1 per item)"""
    rng = random.Random(seed)
    f12 = SETS['F12']
    sk, h = rng.randrange(1, c.R), rng.randrange(1, c.R)
    Hm, pk = c.E1.mul(c.G1_GEN, h), c.E2.mul(c.G2_GEN, sk)
    sig = c.E1.mul(Hm, sk)
    steps = f12.programs['PAIR_GENERAL']
    items = [(nm, pairing_inputs(f12, Hm, pk, s, c.E2.neg(c.G2_GEN), rng)) for nm, s in (('valid', sig), ('invalid', c.E1.mul(sig, 2)))]
    idx = sorted(set().union(*[set(_fill_needed(f12, steps, m)) for _, m in items]))
    return make_run(f12, 'PAIR_GENERAL', steps, idx, items), [True, False]


# ---- what the device must return
def initial_store(run, item, fill):
    """the store's words before the first step: inputs, the set's constants (canonical residues, as the shipped kernels stage them),
    `fill` everywhere else"""
    ts = SETS[run['set']]
    f = fill - 2**32 if fill >= 2**31 else fill
    V = [[f] * 16 for _ in range(ts.nv)]
    for v, x in ts.consts.items():
        V[v] = vec16(limbs_of(x * R392 % P))
    for v, l in zip(run['in_idx'], run['items'][item]):
        V[v] = list(l)
    return V


def expected_store(run, item):
    """field elements per value after the run (None: not defined by the inputs), by sim_program on integers"""
    ts = SETS[run['set']]
    V = [0] * ts.nv
    for v, l in zip(run['in_idx'], run['items'][item]):
        V[v] = elem_of(l[:NL])
    for _ in range(run['reps']):
        chk.sim_program(ts.ops, ts.lay, run['steps'], V)
    return V


def written(run):
    ts = SETS[run['set']]
    return set().union(*[step_io(ts, st)[1] for st in run['steps']])


def inv_written(run):
    ts = SETS[run['set']]
    return {ts.lay.ref(st[1]) for st in run['steps'] if st[0] == 'FPINV'}


def last_writer_is_inv(run):
    """values whose final contents come from FPINV (fp_reduce's range) and not from a table row"""
    ts = SETS[run['set']]
    last = {}
    for st in run['steps']:
        for v in step_io(ts, st)[1]:
            last[v] = st[0] == 'FPINV'
    return {v for v, inv in last.items() if inv}


def check_output_contract(name, v, from_inv=False):
    assert len(v) == 16 and v[14] == 0 and v[15] == 0, '%s: words 14 and 15 are not zero: %r' % (name, v[14:])
    if from_inv:
        assert all(0 <= x <= fc.M for x in v[:NL - 1]) and 100 * abs(val(v[:NL])) <= 52 * P, "%s: outside fp_reduce's range" % name
    else:
        assert all(LIMB_LO <= x <= LIMB_HI for x in v[:NL - 1]), '%s: a limb outside the carry-pass range: %r' % (name, v[:NL - 1])
        assert 5 * abs(val(v[:NL])) < 3 * P, '%s: |value| >= 0.6 p' % name


def check(run, item, store, fill=0, expected=None):
    """store: the whole value store of one item as the door returns it (one sixteen-word vector per value)"""
    ts = SETS[run['set']]
    name = '%s, item "%s"' % (run['name'], run['item_names'][item])
    assert len(store) == ts.nv
    want = expected if expected is not None else expected_store(run, item)
    init = initial_store(run, item, fill)
    wr, inv = written(run), last_writer_is_inv(run)
    for v in range(ts.nv):
        if v in ts.tmp:
            continue
        if v in wr:
            check_output_contract('%s, value %d' % (name, v), store[v], v in inv)
            assert elem_of(store[v][:NL]) == want[v], '%s: value %d is wrong' % (name, v)
        else:
            assert list(store[v]) == init[v], '%s: value %d is not a destination and was changed' % (name, v)
    return True


def all_runs():
    runs = []
    for s, n in ALL_OPS:
        runs += op_runs(s, n)
    return runs + sequence_runs() + chain_runs() + [pairing_run()[0]]


def exercised(runs):
    return {(r['set'], n) for r in runs for n in r['ops']}
