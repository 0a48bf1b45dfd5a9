"""Registered signature sets on the GPU: blsgpu_sigset_*, blsgpu_pairing_sigset_batch and blsgpu_timecrypt_open_indexed_batch against
the lists of tests/timecrypt_cases.py and tests/sigset_cases.py -- byte for byte, status for status, and byte for byte against
blsgpu_pairing_batch / blsgpu_timecrypt_open_batch on the same pairs --, with and without BLSGPU_SIGSET_LINES, both impls, all four
formats, the plan through blsgpu_profile_get (k_pairing_value_rows over a Bls12381G2Impl set with rows, k_pairing_value otherwise
and whenever a named entry has no usable rows), the shapes at which the code takes another path, append, and the handle rules.
Every expectation comes from the case lists (the oracle); each test runs its calls in a fresh child process (tests/sigset_worker.py)."""
import os
import pickle
import subprocess
import sys

import pytest

import sigset_cases as sc
import timecrypt_cases as tc
import timecrypt_ref as tr
import util

pytestmark = pytest.mark.gpu

ROWS, WALK = 'k_pairing_value_rows', 'k_pairing_value'
IMPL_FMT = [(sg, fmt) for sg in (1, 2) for fmt in tc.FMTS]
IMPL_FMT_IDS = ['sg%d-%s' % (sg, tc.FMT_IDS[fmt]) for sg, fmt in IMPL_FMT]


def run_worker(tmp_path, name, calls, timeout=300, env=None):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    spec, out = str(tmp_path / (name + '.spec.pickle')), str(tmp_path / (name + '.out.pickle'))
    with open(spec, 'wb') as f:
        pickle.dump({'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'sigset_worker.py'), spec, out], env=dict(keep, **(env or {})), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
    with open(out, 'rb') as f:
        return pickle.load(f)


def split(blob, n):
    assert len(blob) == tr.GT_BYTES * n
    return [blob[tr.GT_BYTES * i:tr.GT_BYTES * (i + 1)] for i in range(n)]


def diff(names, got, want):
    return [(i, names[i % len(names)] if names else '', got[i], want[i]) for i in range(len(want)) if i >= len(got) or got[i] != want[i]][:8]


def plan(head, rows):
    """the pairing kernel of a call, from its launches"""
    k = head['kernels']
    return (ROWS in k and WALK not in k) if rows else (WALK in k and ROWS not in k)


def the_set(sg, entries, fmt, lines, **more):
    return dict({'sg': sg, 'sigs': [b for b, _ in entries], 'tags': [t for _, t in entries], 'fmt': fmt, 'lines': lines}, **more)


# ------------------------------------------------------------------ values
@pytest.mark.parametrize('sg,fmt', IMPL_FMT, ids=IMPL_FMT_IDS)
def test_pairing_values_by_index(tmp_path, sg, fmt):
    """the pairs of items(fmt, 13) and special_items(fmt): the signature-group members as the entries, the indices in reverse order.
    Bytes and statuses are the lists', and blsgpu_pairing_batch's on the same pairs; with and without rows.  The thirteen plain
    entries alone, with rows, run k_pairing_value_rows under Bls12381G2Impl."""
    g1s, g2s, want, st = tc.items(fmt, 13)
    names, a1, a2, w, s = tc.special_items(fmt)
    g1s, g2s, want, st = g1s + a1, g2s + a2, want + w, st + s
    n = len(want)
    ents, pts = (g1s, g2s) if sg == 1 else (g2s, g1s)
    entries = [(b, 0) for b in ents]
    idx = list(range(n))[::-1]
    rev = lambda xs: [xs[k] for k in idx]  # noqa: E731
    call = {'op': 'sigset_pairing', 'idx': idx, 'points': rev(pts), 'fmt': fmt}
    got = run_worker(tmp_path, 'values', [
        {'op': 'pairing', 'g1s': rev(g1s), 'g2s': rev(g2s), 'fmt': fmt},
        dict(call, set=the_set(sg, entries, fmt, False)),
        dict(call, set=the_set(sg, entries, fmt, True)),
        dict(call, idx=idx[-13:], points=rev(pts)[-13:], set=the_set(sg, entries[:13], fmt, True))])
    by_value = got[0]
    assert by_value[1] == rev(st) and split(by_value[0], n) == rev(want)
    wire = fmt in (tc.COMPRESSED, tc.LEGACY)
    for (head, blob, gst), lines in zip(got[1:3], (False, True)):
        assert head['status'] == [tc.decode_status(sg, b, fmt) if wire else tc.OK for b in ents], (sg, fmt, lines)
        assert head['info'] == dict(head['info'], sig_group=sg, n=n, has_lines=lines and sg == 2)
        assert gst == rev(st), (sg, fmt, lines, diff([], gst, rev(st)))
        assert blob == by_value[0], (sg, fmt, lines, diff([], split(blob, n), rev(want)))
        assert plan(head, False)                 # an identity entry is named: every item walks
    head, blob, gst = got[3]
    assert gst == [tc.OK] * 13 and split(blob, 13) == rev(want)[-13:] and blob == by_value[0][-13 * tr.GT_BYTES:]
    assert plan(head, sg == 2)


# ------------------------------------------------------------------ opening
@pytest.mark.parametrize('sg', [1, 2])
def test_every_case_by_index_in_every_format(tmp_path, sg):
    """the case list of tests/sigset_cases.py as ONE call per format, with and without rows; once with every pointer in device memory,
    where a failed item's range is (0, 0)"""
    rendered = {fmt: sc.render(sg, fmt) for fmt in tc.FMTS}
    calls = [{'op': 'sigset_open', 'items': rendered[fmt][2], 'fmt': fmt, 'set': the_set(sg, rendered[fmt][0], fmt, lines)} for fmt in tc.FMTS for lines in (False, True)]
    dfmt = tc.COMPRESSED if sg == 1 else tc.RAW_PROJ
    calls.append({'op': 'sigset_open_device', 'items': rendered[dfmt][2], 'fmt': dfmt, 'set': the_set(sg, rendered[dfmt][0], dfmt, True)})
    got = run_worker(tmp_path, 'cases%d' % sg, calls)
    assert len(got) == len(calls)
    for cl, res in zip(calls, got):
        fmt, lines = cl['fmt'], cl['set']['lines']
        entries, est, items, want_msgs, want_sts, names = rendered[fmt]
        head, msgs, sts = res[:3]
        assert head['status'] == est and head['info']['n'] == len(entries) and head['info']['has_lines'] == (lines and sg == 2)
        assert sts == want_sts, (sg, fmt, lines, diff(names, sts, want_sts))
        assert msgs == want_msgs, (sg, fmt, lines, diff(names, msgs, want_msgs))
        assert all((m is not None) == (s == tc.OK) for m, s in zip(msgs, sts))
        assert plan(head, False)                 # the identity entry is named: every item walks, the statuses are the same
        assert 'k_timecrypt_open' in head['kernels'] and 'k_sigset_prepare' in head['kernels'] and 'k_timecrypt_prepare' not in head['kernels']
    rng, sts = got[-1][3], got[-1][2]
    assert all(r == (0, 0) for r, s in zip(rng, sts) if s != tc.OK) and any(r != (0, 0) for r in rng)


# ------------------------------------------------------------------ plan
def test_which_pairing_kernel_runs(tmp_path):
    """a Bls12381G2Impl set with rows launches k_pairing_value_rows and not k_pairing_value; the same set without the flag, and a
    Bls12381G1Impl set with the flag, do the reverse; info reports has_lines accordingly; the statuses and messages are the list's
    every time (the entries with usable rows, the two items that name no entry included)"""
    calls, want = [], []
    for sg, lines, rows in ((2, True, True), (2, False, False), (1, True, False)):
        entries, est, items, msgs, sts, names = sc.render(sg, tc.RAW_AFFINE, groups=sc.rows_groups(sg))
        calls.append({'op': 'sigset_open', 'items': items, 'fmt': tc.RAW_AFFINE, 'set': the_set(sg, entries, tc.RAW_AFFINE, lines)})
        want.append((rows, lines and sg == 2, msgs, sts, names))
    got = run_worker(tmp_path, 'plan', calls)
    for (head, msgs, sts), (rows, has_lines, want_msgs, want_sts, names) in zip(got, want):
        assert head['info']['has_lines'] == has_lines
        assert plan(head, rows), head['kernels']
        assert sts == want_sts and msgs == want_msgs, diff(names, sts, want_sts)
        assert sc.E_ARG in sts and tc.OK in sts


# ------------------------------------------------------------------ shapes
def test_shapes(tmp_path):
    """1 item; 65 items over 3 entries (the prepare kernel crosses its 64-lane block); a set of 0 entries, where every index is
    BLSGPU_E_ARG; n == 0 -- Bls12381G2Impl with rows"""
    sg, fmt = 2, tc.RAW_PROJ
    entries, items, msgs, sts = sc.tiled(sg, fmt, 20)
    ent3, it65, m65, s65 = sc.tiled(sg, fmt, 65, groups=sc.three_groups(sg))
    one = next(i for i, s in enumerate(sts) if s == tc.OK)
    nowhere = [(k,) + items[one][1:] for k in (0, 5, sc.NO_ENTRY)]
    got = run_worker(tmp_path, 'shapes', [
        {'op': 'sigset_open', 'items': [items[one]], 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)},
        {'op': 'sigset_open', 'items': it65, 'fmt': fmt, 'set': the_set(sg, ent3, fmt, True)},
        {'op': 'sigset_open', 'items': nowhere, 'fmt': fmt, 'set': the_set(sg, [], fmt, True)},
        {'op': 'sigset_pairing', 'idx': [0, 1], 'points': [items[one][1]] * 2, 'fmt': fmt, 'set': the_set(sg, [], fmt, True)},
        {'op': 'sigset_open', 'items': [], 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)},
        {'op': 'sigset_pairing', 'idx': [], 'points': [], 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)},
        {'op': 'sigset_pairing', 'idx': [1, 0, sc.NO_ENTRY], 'points': [items[one][1]] * 3, 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)},
        {'op': 'sigset_pairing_device', 'idx': [1, 0, sc.NO_ENTRY], 'points': [items[one][1]] * 3, 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)}])
    head, m, s = got[0]
    assert (m, s) == ([msgs[one]], [tc.OK]) and plan(head, True)
    head, m, s = got[1]
    assert len(set(k for k, *_ in it65)) == 3 and head['info']['n'] == 3 and {tc.OK, tc.INVALID_SIGNATURE} <= set(s65)
    assert s == s65 and m == m65 and plan(head, True)
    head, m, s = got[2]
    assert head['info'] == dict(head['info'], n=0, has_lines=False) and s == [sc.E_ARG] * 3 and m == [None] * 3
    head, blob, s = got[3]
    assert s == [sc.E_ARG] * 2 and blob == bytes(2 * tr.GT_BYTES)
    assert got[4][1:] == ([], []) and got[5][1:] == (b'', [])
    assert ROWS not in got[4][0]['kernels'] and WALK not in got[4][0]['kernels']
    assert got[7][1:] == got[6][1:] and got[6][2] == [tc.OK, tc.OK, sc.E_ARG] and plan(got[7][0], True)       # every pointer in device memory


def test_chunk_boundary_with_rows(tmp_path):
    """one call of 4,097 items tiled from the list over the entries with usable rows, Bls12381G2Impl with rows: the last item sits
    alone in the second chunk of k_pairing_value_rows"""
    n = 4097
    entries, items, want_msgs, want_sts = sc.tiled(2, tc.RAW_AFFINE, n)
    (head, msgs, sts), = run_worker(tmp_path, 'chunk', [{'op': 'sigset_open', 'items': items, 'fmt': tc.RAW_AFFINE, 'set': the_set(2, entries, tc.RAW_AFFINE, True)}])
    assert len(sts) == n and sts == want_sts and msgs == want_msgs
    assert plan(head, True) and head['kernels'][ROWS] == 2


# ------------------------------------------------------------------ append
def test_append(tmp_path):
    """3 entries, then 4 more (one undecodable on the wire), then none: *out_first is 3, then 7; info.n is 7; statuses and bytes
    equal those of a set created from the final list; the new entries have rows"""
    sg, fmt = 2, tc.COMPRESSED
    g1s, g2s, want, _ = tc.items(fmt, 7)
    bad = 5
    g2s = g2s[:bad] + [tc.bad_wire(2, 'curve', fmt)] + g2s[bad + 1:]
    bad_st = tc.decode_status(2, g2s[bad], fmt)
    entries = [(b, k % 3) for k, b in enumerate(g2s)]
    est = [bad_st if k == bad else tc.OK for k in range(7)]
    idx = [6, 5, 4, 3, 2, 1, 0, 7]
    pts = [g1s[k] for k in idx[:7]] + [g1s[0]]
    grown = the_set(sg, entries[:3], fmt, True, append=[([b for b, _ in entries[3:]], [t for _, t in entries[3:]], fmt), ([], [], fmt)])
    new_good = [3, 4, 6]
    got = run_worker(tmp_path, 'append', [
        {'op': 'sigset_pairing', 'idx': idx, 'points': pts, 'fmt': fmt, 'set': grown},
        {'op': 'sigset_pairing', 'idx': idx, 'points': pts, 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)},
        {'op': 'sigset_pairing', 'idx': new_good, 'points': [g1s[k] for k in new_good], 'fmt': fmt, 'set': grown}])
    (h_grown, blob_grown, st_grown), (h_whole, blob_whole, st_whole), (h_new, blob_new, st_new) = got
    assert h_grown['status'] == est[:3] and h_grown['appended'] == [(3, est[3:]), (7, [])] and h_whole['status'] == est
    assert h_grown['info'] == h_whole['info'] == dict(h_whole['info'], sig_group=2, n=7, has_lines=True)
    want_st = [bad_st if k == bad else tc.OK for k in idx[:7]] + [sc.E_ARG]
    want_b = [tc.ZERO_GT if k == bad else want[k] for k in idx[:7]] + [tc.ZERO_GT]
    assert st_grown == st_whole == want_st and blob_grown == blob_whole and split(blob_grown, 8) == want_b
    assert plan(h_grown, False) and plan(h_whole, False)          # the undecodable entry is named
    assert st_new == [tc.OK] * 3 and split(blob_new, 3) == [want[k] for k in new_good] and plan(h_new, True)


def test_append_onto_an_empty_set_builds_the_rows(tmp_path):
    """a Bls12381G2Impl set created empty with lines=True has no rows; the first append builds them whole, as creation would: info
    equals that of the set created from the same list, and a call over the new entries reads their rows"""
    sg, fmt = 2, tc.RAW_AFFINE
    entries, items, msgs, sts = sc.tiled(sg, fmt, 9)
    sigs, tags = [b for b, _ in entries], [t for _, t in entries]
    call = {'op': 'sigset_open', 'items': items, 'fmt': fmt}
    (h_empty, m_empty, s_empty), (h_grown, m_grown, s_grown), (h_whole, m_whole, s_whole) = run_worker(tmp_path, 'empty', [
        dict(call, set=the_set(sg, [], fmt, True)),
        dict(call, set=the_set(sg, [], fmt, True, append=[(sigs, tags, fmt)])),
        dict(call, set=the_set(sg, entries, fmt, True))])
    assert h_empty['info'] == dict(h_empty['info'], n=0, has_lines=False) and s_empty == [sc.E_ARG] * 9 and m_empty == [None] * 9
    assert h_grown['appended'] == [(0, [tc.OK] * len(entries))]
    assert h_grown['info'] == h_whole['info'] == dict(h_whole['info'], sig_group=2, n=len(entries), has_lines=True)
    assert s_grown == s_whole == sts and m_grown == m_whole == msgs and tc.OK in sts
    assert plan(h_grown, True) and plan(h_whole, True)


def test_append_across_the_row_cap(tmp_path):
    """BLSGPU_KEYSET_TABLE_MB=1: an entry's rows are 15,232 bytes, so 68 entries' rows fit in 1,048,576 bytes and 69 entries' do not.
    64 entries with rows; 4 appended: the rows grow; 1 more: the rows are dropped and the set works without them.  After each step
    info equals that of a set created whole from the same list in the same process, and a call naming the first, the last old, the
    first new and the last entry gives the list's messages and statuses, and the whole set's Gt bytes.  The entries are the list's,
    repeated: entry p holds what entry p mod E of the list holds, so an item of the list that names p mod E may name p."""
    sg, fmt = 2, tc.RAW_AFFINE
    base, items, msgs, sts = sc.tiled(sg, fmt, 40)
    E = len(base)
    entries = [base[p % E] for p in range(69)]
    assert 68 * 15232 <= 1 << 20 < 69 * 15232
    at = lambda p: next(i for i, it in enumerate(items) if it[0] == p % E and sts[i] == tc.OK)  # noqa: E731
    calls, want = [], []
    for n, appends, named in ((64, (), (0, 63)), (68, (4,), (0, 63, 64, 67)), (69, (4, 1), (0, 67, 68))):
        pick = [at(p) for p in named]
        its = [(p,) + items[i][1:] for p, i in zip(named, pick)] + [(n,) + items[pick[0]][1:]]
        app, k = [], 64
        for c in appends:
            app.append(([b for b, _ in entries[k:k + c]], [t for _, t in entries[k:k + c]], fmt))
            k += c
        for s in (the_set(sg, entries[:64], fmt, True, append=app), the_set(sg, entries[:n], fmt, True)):
            calls.append({'op': 'sigset_open', 'items': its, 'fmt': fmt, 'set': s})
            calls.append({'op': 'sigset_pairing', 'idx': [it[0] for it in its], 'points': [it[1] for it in its], 'fmt': fmt, 'set': s})
        want.append((n, n <= 68, [msgs[i] for i in pick] + [None], [sts[i] for i in pick] + [sc.E_ARG], [(f, [tc.OK] * c) for f, c in zip((64, 68), appends)]))
    got = run_worker(tmp_path, 'cap', calls, env={'BLSGPU_KEYSET_TABLE_MB': '1'})
    for k, (n, rows, want_msgs, want_sts, appended) in enumerate(want):
        (h_go, m_go, s_go), (h_gp, b_gp, s_gp), (h_wo, m_wo, s_wo), (h_wp, b_wp, s_wp) = got[4 * k:4 * k + 4]
        assert h_go['appended'] == h_gp['appended'] == appended, n
        assert h_go['info'] == h_gp['info'] == h_wo['info'] == h_wp['info'] == dict(h_wo['info'], sig_group=2, n=n, has_lines=rows), (n, h_go['info'], h_wo['info'])
        assert s_go == s_wo == want_sts and m_go == m_wo == want_msgs, (n, s_go, s_wo)
        assert s_gp == s_wp == want_sts and b_gp == b_wp and b_gp[-tr.GT_BYTES:] == tc.ZERO_GT and tc.ZERO_GT not in split(b_gp, len(want_sts))[:-1], (n, s_gp, s_wp)
        for h in (h_go, h_gp, h_wo, h_wp):
            assert plan(h, rows), (n, h['kernels'])


# ------------------------------------------------------------------ handles
def test_handles_and_a_u_of_the_wrong_width(tmp_path):
    """a destroyed id, a key set's id, a message set's id and 0 give BLSGPU_E_ARG at every entry point; a signature set's id is no key
    set's or message set's, and every kind's destroy, info, update and append refuse the live ids of the other two kinds and leave the
    three sets as they were.  Then a Bls12381G1Impl set under RAW_AFFINE with us that are 96-byte G1 records, two per 192-byte slot:
    the indexed call reads the bytes the by-value call reads and answers as it does"""
    sg, fmt = 1, tc.RAW_AFFINE
    entries, est, items, msgs, sts, names = sc.render(sg, fmt, groups=sc.three_groups(sg))
    inside = [it for it in items if it[0] < len(entries)][:6]
    narrow = tc.render_point(1, tc.g1_mul(5), fmt, None) + tc.render_point(1, tc.g1_mul(7), fmt, None)
    assert len(narrow) == 192
    odd = [(k, narrow, v, w, t) for k, _, v, w, t in inside]
    groups = [(entries[k][0], entries[k][1], [(narrow, v, w, t)]) for k, _, v, w, t in inside]
    got = run_worker(tmp_path, 'handles', [{'op': 'handles'}, {'op': 'open', 'sg': sg, 'groups': groups, 'fmt': fmt},
                                           {'op': 'sigset_open', 'items': odd, 'fmt': fmt, 'set': the_set(sg, entries, fmt, True)}])
    rcs, = got[0]
    for name in ('destroyed', 'key set', 'message set', 'zero'):
        assert rcs[name] == [-3] * 5, (name, rcs[name])
    assert rcs['as key set'] == [-3, -3] and rcs['live'] == [0, 0]
    # destroy, info, update (key and message sets) and append of every kind on the live ids of the other two
    assert sorted(rcs['wrong kind']) == sorted((a, b) for a in ('key set', 'message set', 'signature set') for b in ('key set', 'message set', 'signature set') if a != b)
    for pair, codes in rcs['wrong kind'].items():
        assert codes == [-3] * (3 if pair[0] == 'signature set' else 4), (pair, codes)
    assert rcs['intact'] is True
    assert got[2][1:] == tuple(got[1]) and all(s != tc.OK for s in got[1][1])
