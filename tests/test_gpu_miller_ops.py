"""What PRODUCES line values ON THE DEVICE: the Miller steps of csrc/pairing.cuh on both Fp2 layouts, the merges of csrc/tower.cuh
and miller_line3_row, one operation at a time (the MILLER1_*, MILLER2_*, LINES_MERGE* and LINE3_ROW rows of csrc/debug_ops.h), against
the integers.

Cases and judging: tests/miller_cases.py -- tests/test_miller_cases.py pins its restatement to the oracle, tests/test_field_cases.py
proves every case legal on the tracked host build.  Every comparison is exact: congruence modulo p of every output, and every output
in the form its step gives it.  Shapes as in tests/test_gpu_field_ops.py: the whole list, 1, 2, 31, 32, 33 and 65 items, both positions
of a lane pair inside a DPP quad, chains of 2, 17 and 63 steps (63 doublings: the depth of the whole walk)."""
import pytest

import field_cases as fc
import miller_cases as mc

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 31, 32, 33, 65)
OPS = sorted(mc.ROWS)
SPLIT_OPS = [op for op in OPS if mc.ROWS[op][0] == 'split']


def run(api, op, cases, reps=1):
    return api.debug_field_op(op, [(cs['vecs'], cs['par']) for cs in cases], reps)


def take(lst, n, start):
    """n consecutive cases from `start` on, cyclically: neighbours differ (tests/test_miller_cases.py)"""
    return [lst[(start + i) % len(lst)] for i in range(n)]


@pytest.mark.parametrize('op', OPS)
def test_whole_list(api, op):
    lst = fc.build()[op]
    outs = run(api, op, lst)
    assert len(outs) == len(lst)
    for cs, o in zip(lst, outs):
        fc.check(op, cs, o)


@pytest.mark.parametrize('op', OPS)
def test_item_counts(api, op):
    """1, 2, 31, 32, 33, 65 items (lane pairs: a lone pair, a full workgroup, one pair into the next, a partly filled third one); the
    one-lane rows also at twice that and across a 64-lane workgroup"""
    lst = fc.build()[op]
    counts = COUNTS if mc.ROWS[op][0] == 'split' else COUNTS + (62, 64, 66, 130)
    for k, n in enumerate(counts):
        cases = take(lst, n, 7 * k)
        outs = run(api, op, cases)
        assert len(outs) == n
        for cs, o in zip(cases, outs):
            fc.check(op, cs, o)


@pytest.mark.parametrize('op', SPLIT_OPS)
def test_both_quad_positions(api, op):
    """the same cases at an even and at an odd pair index -- both positions of a DPP quad -- give identical limbs"""
    lst = fc.build()[op]
    sub = take(lst, min(len(lst), 21), 3)
    even = run(api, op, sub)
    odd = run(api, op, [lst[0]] + sub)[1:]
    for cs, a, b in zip(sub, even, odd):
        fc.check(op, cs, a)
        assert a == b, '%s, case "%s": the result depends on the position in the quad' % (op, cs['name'])


@pytest.mark.parametrize('op', mc.STEP_ROWS)
def test_both_forms_give_the_same_limbs(api, op):
    """par[0] = 0 runs the non-inlined miller_dbl_step / miller_add_step, 1 the body miller_*_step_at inlined through miller_regs:
    identical limbs on every case.  Both forms build the same miller_regs, so this compares the compiler's two code generations of
    one function (a call against the inlined body) and nothing more; the state holders of the line kernels (miller_lds, miller_lds4)
    are reached through the door below, not here."""
    lst = fc.build()[op]
    outs = [run(api, op, [fc.with_pars(cs, first=form) for cs in lst]) for form in (0, 1)]
    for cs, a, b in zip(lst, *outs):
        fc.check(op, cs, a)
        assert a == b, '%s, case "%s": the function and its body differ' % (op, cs['name'])


@pytest.mark.parametrize('kind', ('DBL', 'ADD'))
def test_the_two_fp2_layouts_agree(api, kind):
    """the one-lane and the lane-split row on the same cases: the same field elements in every output"""
    lst = fc.build()['MILLER1_' + kind]
    assert fc.build()['MILLER2_' + kind] is lst
    one, split = run(api, 'MILLER1_' + kind, lst), run(api, 'MILLER2_' + kind, lst)
    for cs, a, b in zip(lst, one, split):
        fc.check('MILLER1_' + kind, cs, a)
        fc.check('MILLER2_' + kind, cs, b)
        assert [mc.elem_of(v) for v in a] == [mc.elem_of(v) for v in b], '%s, case "%s": the layouts disagree' % (kind, cs['name'])


@pytest.mark.parametrize('op', mc.CHAINS)
def test_chains(api, op):
    """reps = 2, 17, 63: T' of a step as the next step's T, in either form"""
    for reps, stride in fc.CHAIN_REPS:
        cases = [fc.with_pars(cs, first=(i + reps) % 2) for i, cs in enumerate(fc.chain_cases(op, stride))]
        outs = run(api, op, cases, reps)
        for cs, o in zip(cases, outs):
            fc.check(op, cs, o, reps)


# ---------------------------------------------------------------------------------------------------------------------------------
# The shipped line kernels through their door (blsgpu_debug_lines): launched as the library launches them, chunk after chunk, on the
# pairs of field_cases.pairing_cases() -- the largest canonical P and Q, points outside the subgroups, the same pair twice, coordinates
# in their negative representative -- and judged entry by entry against the restated walk: all 68 entries of every live item exact
# modulo p and in the form the producer gives them, every limb of a flagged item the sentinel, no word written beyond a chunk's items.
import random

import util
from util import c, P

FP_ONE = util.limbs_of(util.R392 % P)
_walks, _tables = {}, {}
G2NEG = {1: c.E2.neg(c.G2_GEN), 2: fc.g2_negc()}


def walk_of(q):
    if q not in _walks:
        _walks[q] = mc.walk(q)[0]
    return _walks[q]


def rows_of(q):
    key = ('rows', q)
    if key not in _walks:
        _walks[key] = [mc.norm_row(l) for l in walk_of(q)]
    return _walks[key]


def item_points(vecs):
    """((P, Q), ...) of an item's limb vectors, as field elements (six vectors per pair)"""
    out = []
    for k in range(len(vecs) // 6):
        v = vecs[6 * k:6 * k + 6]
        out.append(((mc.elem_of(v[0]), mc.elem_of(v[1])), (mc.f2_of(v[2:4]), mc.f2_of(v[4:6]))))
    return out


def line3_of(vecs):
    """the 68 plain line values of a one-pair item"""
    key = ('l3', id(vecs))
    if key not in _tables:
        (p, q), = item_points(vecs)
        _tables[key] = [mc.line_at(l, p) for l in walk_of(q)]
    return _tables[key]


def line5_of(cs, form):
    """the 68 merged lines of a two-pair case as k_lines2s (form = fixed_g2) or k_lines2s_keyed (form = 'keyed') computes them"""
    key = ('l5', id(cs), form)
    if key not in _tables:
        (p0, q0), (p1, q1) = item_points(cs['vecs'])
        if form == 0:
            t = [mc.merge(mc.line_at(a, p0), mc.line_at(b, p1)) for a, b in zip(walk_of(q0), walk_of(q1))]
        elif form == 'keyed':
            t = [mc.merge_yy(a[0], c.f2_muls(a[1], p0[0]), p0[1], b[0], c.f2_muls(b[1], p1[0]), p1[1]) for a, b in zip(rows_of(q0), rows_of(G2NEG[2]))]
        else:
            t = [mc.merge_y(mc.line_at(a, p0), b[0], c.f2_muls(b[1], p1[0]), p1[1]) for a, b in zip(walk_of(q0), rows_of(G2NEG[form]))]
        _tables[key] = [list(x) for x in t]
    return _tables[key]


def is_sentinel(entries, api):
    return all(x == api.COOP_SENTINEL for e in entries for co in e for v in co for x in v)


def check_line5(tag, want, got, skip_form=False):
    """one item's 68 entries of five coefficients: exact, c0, c2, c3, c5 reduced and c4 a product (a line that passed a skipped
    partner: c4 = c5 = 0 limb for limb)"""
    assert len(got) == 68
    for e, (w, g) in enumerate(zip(want, got)):
        for k, nm in enumerate(('c0', 'c2', 'c4', 'c3', 'c5')):
            vs = [list(g[k][0]), list(g[k][1])]
            assert mc.f2_of(vs) == tuple(w[k]), '%s, entry %d: %s differs' % (tag, e, nm)
            if skip_form == 'one':                 # both skipped: the constant 1 (fp_one: R mod p in exact limbs) and zeros
                assert vs == ([FP_ONE, mc.ZERO] if k == 0 else [mc.ZERO, mc.ZERO]), '%s, entry %d: %s of the line 1, limb for limb' % (tag, e, nm)
            elif skip_form and k in (2, 4):
                assert vs == [mc.ZERO, mc.ZERO], '%s, entry %d: %s is not zero limb for limb' % (tag, e, nm)
            else:
                assert mc._form('split', 'mult' if k == 2 else 'reduced', vs), '%s, entry %d: %s is not a %s: %s' % (tag, e, nm, 'product' if k == 2 else 'reduced value', vs)


def check_line3(tag, want, got, walked=True, y=None):
    """one item's 68 entries of three coefficients: exact; of a walked point l0 normalised and l2, l3 multiplier outputs, of a table
    row l2 a multiplier output and l3 = (y, 0) limb for limb"""
    assert len(got) == 68
    for e, (w, g) in enumerate(zip(want, got)):
        vs = [[list(g[k][0]), list(g[k][1])] for k in range(3)]
        for k, nm in enumerate(('l0', 'l2', 'l3')):
            assert mc.f2_of(vs[k]) == tuple(w[k]), '%s, entry %d: %s differs' % (tag, e, nm)
        assert mc._form('split', 'mult', vs[1]), '%s, entry %d: l2 is not a pair of multiplier outputs' % (tag, e)
        if walked:
            b = mc.L0_BOUND[('split', 'ADD' if e in mc.ADD_ENTRIES else 'DBL')]
            assert mc._is_norm(vs[0][0], b[0]) and mc._is_norm(vs[0][1], b[1]), '%s, entry %d: l0 is not normalised within %s p' % (tag, e, b[0])
            assert mc._form('split', 'mult', vs[2]), '%s, entry %d: l3 is not a pair of multiplier outputs' % (tag, e)
        else:
            assert vs[2] == [list(y), mc.ZERO], '%s, entry %d: l3 is not (y, 0) limb for limb' % (tag, e)


def two_pair_cases(form):
    return [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == (2 if form == 'keyed' else form)]


_one = []


def one_pair_items():
    """the pairs of field_cases.pairing_cases() one by one (six vectors each), a subgroup filler wherever two neighbours would be the
    same record, the wrap-around included"""
    if not _one:
        rng = random.Random(6868)
        for cs in fc.pairing_cases():
            for k in (0, 1):
                v = cs['vecs'][6 * k:6 * k + 6]
                if _one and _one[-1] == v:
                    _one.append(fc.pair_vecs([(mc._g1(rng), mc._g2(rng))]))
                _one.append(v)
        if _one[0] == _one[-1]:
            _one.append(fc.pair_vecs([(mc._g1(rng), mc._g2(rng))]))
        assert all(a != b for a, b in zip(_one, _one[1:] + _one[:1]))
    return _one


def flags_for(n):
    """flagged items at item 0, at n - 1 and inside a quad beside live ones"""
    return {0, 5, 18, n - 1} if n >= 31 else {0} if n == 2 else set()


def runs():
    """(n, start, flagged, chunk): every count plain, the larger ones again with flagged items, 65 again in chunks of 32"""
    out = []
    for k, n in enumerate(COUNTS):
        out.append((n, 7 * k, set(), 0))
        if flags_for(n):
            out.append((n, 7 * k + 3, flags_for(n), 0))
    out.append((65, 11, set(), 32))
    out.append((65, 13, flags_for(65) | {32, 63, 64}, 32))
    return out


def consume(api, kernel, cases, outs, status, flagged, form, easy):
    """the producer meets the consumer, on EVERY run of a line5 kernel (every count, flagged or not, chunked or not): its output goes
    into k_millerf2s limbs unchanged (a flagged item's sentinel entries too: the consumer skips it by its status); every live value is
    field_cases.miller_expected of the restated table, exact and reduced, and its verdict through the batch final exponentiation the
    status the oracle gives the case.  easy: also the easy part in Python integers against the oracle's -- the 31-item runs only (with
    and without flagged items; 31 items cycle every case of a form), an Fp12 inversion per item being what it costs"""
    vals = api.debug_millerf(outs, status)
    live = [(cs, v) for i, (cs, v) in enumerate(zip(cases, vals)) if i not in flagged]
    for cs, v in live:
        fc.check_miller('%s (lines of %s)' % (cs['name'], kernel), line5_of(cs, form), v)
        if easy:
            assert fc.cyclotomic(fc.f12_of_vecs(v)) == fc.pairing_expected(cs)[1], '%s: easy part, case "%s"' % (kernel, cs['name'])
    if live:
        got = api.debug_finalexp_batch([util.f12_record(fc.f12_of_vecs(v)) for cs, v in live], 0)
        assert got == [fc.pairing_expected(cs)[2] for cs, v in live], kernel


@pytest.mark.parametrize('form', (0, 1, 2))
def test_lines2s_through_the_door_and_into_the_consumer(api, form):
    """k_lines2s (fixed_g2 = 1, 2: one launch; 0: passes 1 then 2), every entry against the restated walk; then into the consumer
    (consume(), above)"""
    lst = two_pair_cases(form)
    for n, start, flagged, chunk in runs():
        cases = take(lst, n, start)
        status = [7 if i in flagged else 0 for i in range(n)]
        outs, stray = api.debug_lines('lines2s', [cs['vecs'] for cs in cases], form, status, chunk)
        assert stray == 0 and len(outs) == n
        for i, (cs, o) in enumerate(zip(cases, outs)):
            tag = 'k_lines2s fixed_g2 = %d, %d items, chunk %d, item %d "%s"' % (form, n, chunk, i, cs['name'])
            if i in flagged:
                assert is_sentinel(o, api), tag + ': flagged, and its entries were written'
            else:
                check_line5(tag, line5_of(cs, form), o)
        consume(api, 'k_lines2s', cases, outs, status, flagged, form, easy=(n == 31))


def keyed_cases():
    return two_pair_cases('keyed')


def test_lines2s_keyed_through_the_door(api):
    """k_lines2s_keyed: pair 0's rows from a registered set (one entry per case, named out of order), pair 1's from the constant table;
    merged with lines_merge_yy; then into the consumer (consume(), above)"""
    lst = keyed_cases()
    keys = [util.g2_aff_raw(cs['pairs'][0][1]) for cs in lst]
    with api.KeySet.create(1, keys, api.FMT_RAW_AFFINE, lines=True) as ks:
        for n, start, flagged, chunk in runs():
            pos = [(start + i) % len(lst) for i in range(n)]
            cases = [lst[p] for p in pos]
            status = [7 if i in flagged else 0 for i in range(n)]
            other = lst[0]['vecs'][2:6]                    # the record's own Q0 is not read
            outs, stray = api.debug_lines('lines2s_keyed', [cs['vecs'][:2] + other + cs['vecs'][6:] for cs in cases], 0, status, chunk, ks, pos)
            assert stray == 0 and len(outs) == n
            for i, (cs, o) in enumerate(zip(cases, outs)):
                tag = 'k_lines2s_keyed, %d items, chunk %d, item %d "%s"' % (n, chunk, i, cs['name'])
                if i in flagged:
                    assert is_sentinel(o, api), tag + ': flagged, and its entries were written'
                else:
                    check_line5(tag, line5_of(cs, 'keyed'), o)
            consume(api, 'k_lines2s_keyed', cases, outs, status, flagged, 'keyed', easy=(n == 31))


@pytest.mark.parametrize('kernel', ('linesp1', 'linesp4'))
def test_plain_lines_of_the_product_kernels(api, kernel):
    """k_linesp pass 1 (two lanes per item) and k_linesp4 (four lanes, the doubling shared by two lane pairs): the three coefficients
    of every entry of every live item"""
    lst = one_pair_items()
    for n, start, flagged, chunk in runs():
        items = take(lst, n, start)
        status = [1 if i in flagged else 0 for i in range(n)]
        outs, stray = api.debug_lines(kernel, items, 0, status, chunk)
        assert stray == 0 and len(outs) == n
        for i, (v, o) in enumerate(zip(items, outs)):
            tag = '%s, %d items, chunk %d, item %d (case list position %d)' % (kernel, n, chunk, i, (start + i) % len(lst))
            if i in flagged:
                assert is_sentinel(o, api), tag + ': flagged, and its entries were written'
            else:
                check_line3(tag, line3_of(v), o)


def test_the_four_lane_kernel_gives_the_two_lane_kernels_lines(api):
    """k_linesp4's comment promises the same field elements as the two-lane form: entry for entry, on the whole item list"""
    lst = one_pair_items()
    a, _ = api.debug_lines('linesp1', lst)
    b, _ = api.debug_lines('linesp4', lst)
    for i, (x, y) in enumerate(zip(a, b)):
        for e in range(68):
            assert [mc.f2_of(co) for co in x[e]] == [mc.f2_of(co) for co in y[e]], 'item %d, entry %d' % (i, e)
        check_line3('k_linesp4, item %d' % i, line3_of(lst[i]), y)


@pytest.mark.parametrize('mm', (1, 2, 31, 32, 33, 65))
def test_linesp_both_passes(api, mm):
    """k_linesp passes 1 and 2 with half = ceil(mm / 2): virtual item v merges item v with item v + half.  mm odd leaves the last
    virtual item without a partner; skip_a / skip_b in every combination next to live virtual items: the other item's line reduced,
    the line 1 when both are skipped, c4 = c5 = 0"""
    lst = one_pair_items()
    half = (mm + 1) // 2
    for flagged in (set(), {0, 2 + half, 3, 3 + half, mm - 1} & set(range(mm))):
        items = take(lst, mm, 5 + mm)
        status = [1 if i in flagged else 0 for i in range(mm)]
        outs, stray = api.debug_lines('linesp12', items, 0, status)
        assert stray == 0 and len(outs) == half
        seen = set()
        for v, o in enumerate(outs):
            ib = v + half
            skip_a, skip_b = v in flagged, ib >= mm or ib in flagged
            seen.add((skip_a, skip_b))
            tag = 'k_linesp 1 + 2, mm = %d, virtual item %d (skip_a %d, skip_b %d)' % (mm, v, skip_a, skip_b)
            la = line3_of(items[v])
            lb = line3_of(items[ib]) if ib < mm else None
            if not skip_a and not skip_b:
                check_line5(tag, [mc.merge(a, b) for a, b in zip(la, lb)], o)
            else:
                z = mc.F2_ZERO
                keep = [(mc.F2_ONE, z, z)] * 68 if skip_a and skip_b else lb if skip_a else la
                check_line5(tag, [(l[0], l[1], z, l[2], z) for l in keep], o, skip_form='one' if skip_a and skip_b else True)
        if flagged and mm >= 31:
            assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_table_rows_of_the_product_kernels(api):
    """k_linesp_keyed: items below T_b read the rows of their key, the others the constant's; k_lines_fixed is item 0 of the signature
    branch.  Exact, l0 the row's limbs, l3 = (y, 0)"""
    lst = keyed_cases()
    keys = [util.g2_aff_raw(cs['pairs'][0][1]) for cs in lst]
    ones = one_pair_items()
    with api.KeySet.create(1, keys, api.FMT_RAW_AFFINE, lines=True) as ks:
        for n, start, flagged, chunk in runs():
            t_b = n // 2
            pos = [(start + 3 * i) % len(lst) for i in range(n)]
            items = take(ones, n, start)
            status = [1 if i in flagged else 0 for i in range(n)]
            outs, stray = api.debug_lines('linesp_keyed', items, 0, status, chunk, ks, pos, t_b)
            assert stray == 0 and len(outs) == n
            for i, (v, o) in enumerate(zip(items, outs)):
                tag = 'k_linesp_keyed, %d items, T_b %d, chunk %d, item %d' % (n, t_b, chunk, i)
                if i in flagged:
                    assert is_sentinel(o, api), tag + ': flagged, and its entries were written'
                    continue
                p = (mc.elem_of(v[0]), mc.elem_of(v[1]))
                rows = rows_of(lst[pos[i]]['pairs'][0][1]) if i < t_b else rows_of(G2NEG[2])
                check_line3(tag, [mc.line3_row(r[0], r[1], p[0], p[1]) for r in rows], o, walked=False, y=v[1])
        # k_lines_fixed against the signature branch (T_b = 0) and against the restated rows, both constants
        for fx in (1, 2):
            for v in (ones[0], ones[9]):
                fixed, stray = api.debug_lines('lines_fixed', [v, ones[1]], fx)
                assert stray == 0 and len(fixed) == 1
                p = (mc.elem_of(v[0]), mc.elem_of(v[1]))
                check_line3('k_lines_fixed, fixed_g2 = %d' % fx, [mc.line3_row(r[0], r[1], p[0], p[1]) for r in rows_of(G2NEG[fx])], fixed[0], walked=False, y=v[1])
                if fx == 2:
                    sig, _ = api.debug_lines('linesp_keyed', [v, ones[1]], 0, None, 0, ks, [0, 0], 0)
                    assert fixed[0] == sig[0], 'k_lines_fixed and item 0 of the signature branch of k_linesp_keyed differ'
        flagged, _ = api.debug_lines('lines_fixed', [ones[0]], 1, [1])
        assert is_sentinel(flagged[0], api)


@pytest.mark.parametrize('form', (0, 1, 2))
def test_miller2s_the_one_kernel_fallback(api, form):
    """k_miller2s, what run_pairing2 takes when the line workspace cannot be reserved, at every count, with and without flagged items:
    the value is reduced (c1 negated limb-wise by the conjugation), as check_miller asserts it, and a flagged item's slot keeps the
    sentinel.  The easy part in Python integers against the oracle's at 1 and 33 items (with and without flagged items; 33 items cycle
    every case of a form)"""
    lst = two_pair_cases(form)
    for n, start, flagged, _ in runs()[:-2]:          # (the kernel takes the whole batch in one launch: no chunked runs)
        cases = take(lst, n, start)
        status = [7 if i in flagged else 0 for i in range(n)]
        outs, _ = api.debug_lines('miller2s', [cs['vecs'] for cs in cases], form, status)
        for i, (cs, o) in enumerate(zip(cases, outs)):
            tag = 'k_miller2s fixed_g2 = %d, %d items, item %d "%s": ' % (form, n, i, cs['name'])
            if i in flagged:
                assert all(x == api.COOP_SENTINEL for v in o for x in v), tag + 'flagged, and its value was written'
                continue
            for k, v in enumerate(o):
                l = v if k < 6 else [-x for x in v]
                assert mc._is_reduced(l), tag + 'vector %d is not a (negated) reduced value: %s' % (k, v)
            if n in (1, 33):
                assert fc.cyclotomic(fc.f12_of_vecs(o)) == fc.pairing_expected(cs)[1], tag + 'easy part'
