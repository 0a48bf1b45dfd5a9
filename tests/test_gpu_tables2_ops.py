"""The two kernels whose pairs BOTH read their rows from one table in global memory (blsgpu_signcrypt_share_verify_indexed_batch,
Bls12381G2Impl), through their hook (blsgpu_debug_tables2): k_lines2s_tables2 and k_pairing_coop_tables2 on the crafted two-general-pair
cases of field_cases.pairing_cases() -- the largest canonical P and Q, points outside the subgroups, the same pair twice, coordinates in
their negative representative.  The G2 members of all cases form ONE table, built by the library's row builder, and every item names
its Q0 and Q1 by position, out of order.  Judging as in tests/test_gpu_miller_ops.py and tests/test_gpu_keyset_lines_coop.py: every
line5 entry exact against the restated rows, sentinels for flagged items, the stream into k_millerf2s and the batch final
exponentiation; easy-part values exact and verdicts the oracle's."""
import ctypes
import random

import pytest

import field_cases as fc
import miller_cases as mc
import test_gpu_miller_ops as mo
import util
from util import c

pytestmark = pytest.mark.gpu

E_ARG = -3
CASES = [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == 0]
FORM = 'tables2'


def table_points():
    """the distinct G2 members of the cases, shuffled: (points, RAW_AFFINE records)"""
    qs = []
    for cs in CASES:
        for _, q in cs['pairs']:
            if q not in qs:
                qs.append(q)
    random.Random(22).shuffle(qs)
    return qs, [util.g2_aff_raw(q) for q in qs]


def entries(qs, cases):
    return [qs.index(cs['pairs'][0][1]) for cs in cases], [qs.index(cs['pairs'][1][1]) for cs in cases]


def line5_tables2(cs):
    """the 68 merged lines as k_lines2s_tables2 computes them: both rows evaluated at their G1 point, lines_merge_yy; left where
    test_gpu_miller_ops.line5_of looks first, so that its consume() judges the stream of this kernel"""
    key = ('l5', id(cs), FORM)
    if key not in mo._tables:
        (p0, q0), (p1, q1) = mo.item_points(cs['vecs'])
        q0, q1 = cs['pairs'][0][1], cs['pairs'][1][1]           # the table holds the canonical points
        mo._tables[key] = [list(mc.merge_yy(a[0], c.f2_muls(a[1], p0[0]), p0[1], b[0], c.f2_muls(b[1], p1[0]), p1[1]))
                           for a, b in zip(mo.rows_of(q0), mo.rows_of(q1))]
    return mo._tables[key]


def other_q(cases):
    """the records with another point in the place of both Q members: the kernels read the table, not the record"""
    other = CASES[5]['vecs'][2:6]
    return [cs['vecs'][:2] + other + cs['vecs'][6:8] + other for cs in cases]


RUNS = [(1, 0, set(), 0), (2, 3, set(), 0), (2, 5, {0}, 0), (31, 7, set(), 0), (31, 9, {0, 5, 18, 30}, 0), (33, 2, {0, 5, 18, 32}, 0),
        (65, 11, set(), 0), (65, 11, set(), 32), (65, 13, {0, 5, 18, 32, 63, 64}, 32)]


def test_lines2s_tables2_through_the_door_and_into_the_consumer(api):
    qs, pts = table_points()
    assert len(qs) >= 5
    for n, start, flagged, chunk in RUNS:
        cases = mo.take(CASES, n, start)
        t0, t1 = entries(qs, cases)
        assert n < 31 or (t0 != sorted(t0) and len(set(t0)) > 1 and len(set(t1)) > 1)
        status = [7 if i in flagged else 0 for i in range(n)]
        outs, stray = api.debug_lines_tables2(pts, t0, t1, other_q(cases), status, chunk)
        assert stray == 0 and len(outs) == n
        for i, (cs, o) in enumerate(zip(cases, outs)):
            tag = 'k_lines2s_tables2, %d items, chunk %d, item %d "%s"' % (n, chunk, i, cs['name'])
            if i in flagged:
                assert mo.is_sentinel(o, api), tag + ': flagged, and its entries were written'
            else:
                mo.check_line5(tag, line5_tables2(cs), o)
        mo.consume(api, 'k_lines2s_tables2', cases, outs, status, flagged, FORM, easy=(n == 31))


def test_coop_tables2_easy_part_and_verdict(api):
    """1, 2, 31, 33 and 65 items: the exported easy-part value is the oracle's miller_loop(pairs)^((p^6 - 1)(p^2 + 1)) exactly, and the
    verdict is OK exactly where its pairing product is one; flagged items at 0, inside and at n - 1 keep status and sentinel; the
    records carry another point in the place of their Q members"""
    qs, pts = table_points()
    for n, start, flagged, _ in RUNS[:7]:
        cases = mo.take(CASES, n, start)
        t0, t1 = entries(qs, cases)
        status = [7 if i in flagged else 0 for i in range(n)]
        vecs = other_q(cases)
        outs = api.debug_coop_pairing_tables2(0, pts, t0, t1, vecs, status)
        assert len(outs) == n
        for i, (cs, o) in enumerate(zip(cases, outs)):
            if i in flagged:
                assert all(x == api.COOP_SENTINEL for v in o for x in v), 'item %d was flagged and its easy-part slot was written' % i
            else:
                fc.check_easy(cs, o)
        got = api.debug_coop_pairing_tables2(1, pts, t0, t1, vecs, status)
        want = [7 if i in flagged else fc.pairing_expected(cs)[2] for i, cs in enumerate(cases)]
        assert got == want, [cs['name'] for cs, g, w in zip(cases, got, want) if g != w]
        # ... and with the records' own Q members in place: the same values
        assert api.debug_coop_pairing_tables2(0, pts, t0, t1, [cs['vecs'] for cs in cases], status) == outs
    assert {fc.pairing_expected(cs)[2] for cs in CASES} == {fc.BLS_OK, fc.BLS_INVALID}


def test_hook_argument_errors(api):
    qs, pts = table_points()
    vecs = [CASES[0]['vecs']]
    t0, t1 = entries(qs, CASES[:1])
    with pytest.raises(Exception):
        api._debug_tables2(3, pts, t0, t1, vecs, None, 0)                              # another mode
    for mode in (0, 1):
        with pytest.raises(Exception):
            api.debug_coop_pairing_tables2(mode, pts, [len(pts)], t1, vecs)            # an index outside the table
        with pytest.raises(Exception):
            api.debug_coop_pairing_tables2(mode, pts, t0, [2 ** 32 - 1], vecs)
    with pytest.raises(Exception):
        api.debug_lines_tables2(pts, t0 * 4097, t1 * 4097, vecs * 4097)
    with pytest.raises(Exception):
        api.debug_lines_tables2([], [0], [0], vecs)                                    # no table
    with pytest.raises(Exception):
        api.debug_lines_tables2(pts + [pts[0][:96] + bytes(96)], t0, t1, vecs)         # (x, 0): its walk meets h = 0, no usable rows
    with pytest.raises(Exception):
        api.debug_lines_tables2(pts + [bytes(192)], t0, t1, vecs)                      # the identity has no rows
    lib = api.init()
    st, a0, a1 = (ctypes.c_int32 * 1)(0), (ctypes.c_uint32 * 1)(t0[0]), (ctypes.c_uint32 * 1)(t1[0])
    arr = (ctypes.c_int32 * 168)(*[x for v in vecs[0] for x in v])
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    blob = b''.join(pts)
    assert lib.blsgpu_debug_tables2(1, api._ptr(blob), len(pts), p(a0), p(a1), p(arr), 1, p(st), 0, None, None) == 0 and st[0] == fc.pairing_expected(CASES[0])[2]
    assert lib.blsgpu_debug_tables2(2, api._ptr(blob), len(pts), p(a0), p(a1), p(arr), 1, p(st), 0, None, None) == E_ARG
    assert lib.blsgpu_debug_tables2(1, None, len(pts), p(a0), p(a1), p(arr), 1, p(st), 0, None, None) == E_ARG
