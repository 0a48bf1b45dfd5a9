"""Registered message sets on the GPU (blsgpu_msgset_*, blsgpu_verify_msgset_batch, blsgpu_verify_msgset_indexed_batch): a message is
hashed once, at registration, and groups of (key, signature) items name it by position.  Expected statuses are the oracle's -- one
verification per item under the message its group's entry holds (tests/msgset_cases.py, which tests/test_msgset_cases.py checks on
the CPU; the 130-item shape of tests/test_gpu_verify_shared.py with the C oracle on every item) -- never another GPU call's.  The
one-wave kernel that reads an entry's rows (k_pairing_coop_rows) goes through its hook on the crafted pairs of field_cases: exact
easy-part values and verdicts.  Which kernel ran is decided by the launch counts of the profile, so no run can pass by falling back,
and every run of the calls asserts that nothing was hashed and no per-call table was built.  Runs that need their own process (the
knobs are read once) go through tests/msgset_worker.py: one attempt each, with its own time limit."""
import ctypes
import functools
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

import field_cases as fc
import msgset_cases as mc
import test_gpu_keyset_lines as kl
import test_gpu_verify_shared as vs
import util
import verify_shared_cases as vc
from util import ref

pytestmark = pytest.mark.gpu

E_ARG = -3
OK, INVALID, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
ENTRY_LINE_BYTES = 68 * 4 * 14 * 4                # 15,232
ONE_WAVE = {'BLSGPU_WIDE_MAX': '0'}
LANE_SPLIT = {'BLSGPU_WIDE_MAX': '0', 'BLSGPU_COOP_MAX': '0'}
SIZES_130 = (1, 0, 64, 65)
PAIR_COUNTS = (1, 2, 33, 65)
GENERAL = [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == 0]
SCHEMES = [(ref.BASIC, 'basic'), (ref.POP, 'pop')]


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


def flat(groups_of_statuses):
    return [s for g in groups_of_statuses for s in g]


def run_worker(tmp_path, name, env, msgsets, keysets, steps, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'msgsets': msgsets, 'keysets': keysets, 'steps': steps}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'msgset_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])['steps']


def nothing_hashed_nothing_built(launches):
    """no hash kernel (k_hash_to_point counts the lane, wave and engine forms alike), no k_group_lines; k_prepare_shared counts
    k_group_affine as well, so exactly one launch of it says that the groups' points were not made affine again"""
    assert not any('hash' in k for k in launches), launches
    assert launches.get('k_group_lines', 0) == 0 and launches.get('k_prepare_shared', 0) == 1, launches
    assert launches.get('k_keyset_lines', 0) == 0 and launches.get('k_msgset_seal', 0) == 0, launches


def pairing_launches(launches):
    return {k: launches.get(k, 0) for k in ('k_pairing_coop_rows', 'k_pairing_coop', 'k_pairing_coop_keyed', 'k_lines2s', 'k_lines2s_keyed', 'k_millerf2s', 'k_wide')}


# ------------------------------------------------------------------ 1. the kernel through its hook
def case_points():
    """the cases' Q0 as RAW_AFFINE G2 records, one entry per case (points outside the subgroup among them)"""
    return [util.g2_aff_raw(cs['pairs'][0][1]) for cs in GENERAL]


def test_hook_easy_part_and_verdict(api):
    """1, 2, 33 and 65 items (the list cycles, so entries repeat and their order is not the items'): the exported easy-part value is
    the oracle's miller_loop(pairs)^((p^6 - 1)(p^2 + 1)) exactly, and the verdict is OK exactly where its pairing product is one"""
    with api.debug_msgset_from_points(2, case_points(), lines=True) as ms:
        info = ms.info()
        assert info['has_lines'] is True and info['n'] == len(GENERAL) and info['sig_group'] == 2
        for k, n in enumerate(PAIR_COUNTS):
            pos = [(3 * k + i) % len(GENERAL) for i in range(n)]
            cases = [GENERAL[p] for p in pos]
            outs = api.debug_coop_pairing_rows(0, ms, pos, [cs['vecs'] for cs in cases])
            assert len(outs) == n
            for cs, o in zip(cases, outs):
                fc.check_easy(cs, o)
            got = api.debug_coop_pairing_rows(1, ms, pos, [cs['vecs'] for cs in cases])
            want = [fc.pairing_expected(cs)[2] for cs in cases]
            assert got == want, [cs['name'] for cs, g, w in zip(cases, got, want) if g != w]
        assert {fc.pairing_expected(cs)[2] for cs in GENERAL} == {fc.BLS_OK, fc.BLS_INVALID}


def test_hook_skips_flagged_items_and_reads_the_set_not_the_record(api):
    """items that are not OK on entry are skipped (status kept, sentinel kept); the record's own Q0 is not read: with another point in
    its place the values are those of the entry"""
    n = 9
    pos = [(2 + i) % len(GENERAL) for i in range(n)]
    cases = [GENERAL[p] for p in pos]
    other = GENERAL[3]['vecs'][2:6]
    assert all(cs['vecs'][2:6] != other for cs in cases if cs is not GENERAL[3])
    vecs = [cs['vecs'][:2] + other + cs['vecs'][6:] for cs in cases]
    flagged = {0, 4, n - 1}
    status = [7 if i in flagged else OK for i in range(n)]
    with api.debug_msgset_from_points(2, case_points(), lines=True) as ms:
        outs = api.debug_coop_pairing_rows(0, ms, pos, vecs, status)
        for i, (cs, o) in enumerate(zip(cases, outs)):
            if i in flagged:
                assert all(x == api.COOP_SENTINEL for v in o for x in v), 'item %d was flagged and its easy-part slot was written' % i
            else:
                fc.check_easy(cs, o)
        got = api.debug_coop_pairing_rows(1, ms, pos, vecs, status)
        assert got == [7 if i in flagged else fc.pairing_expected(cs)[2] for i, cs in enumerate(cases)]


def test_hook_argument_errors(api):
    vecs = [GENERAL[0]['vecs']]
    with api.debug_msgset_from_points(2, case_points()) as plain, api.debug_msgset_from_points(2, case_points(), lines=True) as ms:
        assert plain.info()['has_lines'] is False
        for mode in (0, 1):
            with pytest.raises(Exception):
                api.debug_coop_pairing_rows(mode, plain, [0], vecs)                   # a set without rows
            with pytest.raises(Exception):
                api.debug_coop_pairing_rows(mode, ms, [len(GENERAL)], vecs)           # an index outside the set
        with pytest.raises(Exception):
            api.debug_coop_pairing_rows(2, ms, [0], vecs)
        with pytest.raises(Exception):
            api.debug_coop_pairing_rows(1, ms, [0] * 4097, vecs * 4097)
        lib = api.init()
        st, idx, arr = (ctypes.c_int32 * 1)(0), (ctypes.c_uint32 * 1)(0), (ctypes.c_int32 * 168)(*[x for v in vecs[0] for x in v])
        p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
        assert lib.blsgpu_debug_coop_pairing_rows(1, plain.handle, p(idx), p(arr), 1, p(st), None) == E_ARG
        assert lib.blsgpu_debug_coop_pairing_rows(1, ms.handle, p(idx), p(arr), 1, p(st), None) == 0 and st[0] == fc.pairing_expected(GENERAL[0])[2]


# ------------------------------------------------------------------ 2. the 130 items of the one-wave and lane-split runs
@functools.lru_cache(maxsize=None)
def reference_130(sg, scheme):
    """130 items in groups of 1, 0, 64, 65 (signed on the device, tampered by the pattern of tests/test_gpu_verify_shared.py) and the
    ORACLE's status of every item; the set holds the groups' messages in reverse order between two entries nobody names, so a
    group's index is not its number.  Returns (entries, by-value groups, indexed groups, the keys, expected statuses)."""
    groups, expect = vs.signed_batch(sg, scheme, SIZES_130)
    want = vc.oracle_statuses(util.load_c_oracle(), sg, scheme, groups)
    assert want == expect and {OK, INVALID, SIG_IDENTITY, PK_IDENTITY} <= set(want)
    n_groups = len(groups)
    entries = [b'nobody names this entry'] + [groups[n_groups - 1 - k][0] for k in range(n_groups)] + [b'nor this one']
    midx = [n_groups - g for g in range(n_groups)]
    assert all(entries[midx[g]] == groups[g][0] for g in range(n_groups)) and b'' in entries
    by_value = [(midx[g], pks, sigs) for g, (_, pks, sigs) in enumerate(groups)]
    keys = [p for _, pks, _ in groups for p in pks]
    at, indexed = 0, []
    for g, (_, pks, sigs) in enumerate(groups):
        indexed.append((midx[g], list(range(at, at + len(pks))), sigs))
        at += len(pks)
    return entries, by_value, indexed, keys, want


def steps_130(sg):
    msgsets, keysets, steps, wants = {}, {}, [], []
    for scheme, sid in SCHEMES:
        entries, by_value, indexed, keys, want = reference_130(sg, scheme)
        for lines in (True, False):
            msgsets['%s_%d' % (sid, lines)] = {'sg': sg, 'scheme': scheme, 'msgs': entries, 'lines': lines}
        keysets[sid] = {'sg': sg, 'keys': keys, 'fmt': 0, 'lines': True}
        for lines in (True, False):
            steps.append({'msgset': '%s_%d' % (sid, lines), 'groups': by_value})
            steps.append({'msgset': '%s_%d' % (sid, lines), 'keyset': sid, 'groups': indexed})
            wants += [(want, lines, False), (want, lines, True)]
    return msgsets, keysets, steps, wants


@pytest.mark.parametrize('sg', [1, 2])
def test_one_wave_path(api, tmp_path, sg):
    """BLSGPU_WIDE_MAX=0, Basic and ProofOfPossession, by value and indexed.  Bls12381G2Impl: over a set with rows
    k_pairing_coop_rows runs once and k_pairing_coop not at all; over a set without rows the reverse.  Bls12381G1Impl: k_pairing_coop
    by value, and k_pairing_coop_keyed over the key set with lines (such an item then needs nothing but its signature)."""
    msgsets, keysets, steps, wants = steps_130(sg)
    got = run_worker(tmp_path, 'one_wave_%d' % sg, ONE_WAVE, msgsets, keysets, steps)
    for g, (want, lines, indexed) in zip(got, wants):
        print(sg, lines, indexed, g['launches'])
        assert g['st'] == want
        nothing_hashed_nothing_built(g['launches'])
        pl = pairing_launches(g['launches'])
        if sg == 2:
            assert (pl['k_pairing_coop_rows'], pl['k_pairing_coop']) == ((1, 0) if lines else (0, 1)), pl
            assert pl['k_pairing_coop_keyed'] == 0
        else:
            assert pl['k_pairing_coop_rows'] == 0 and (pl['k_pairing_coop'], pl['k_pairing_coop_keyed']) == ((0, 1) if indexed else (1, 0)), pl
        assert pl['k_lines2s'] == 0 and pl['k_lines2s_keyed'] == 0 and pl['k_wide'] == 0, pl


@pytest.mark.parametrize('sg', [1, 2])
def test_lane_split_path(api, tmp_path, sg):
    """BLSGPU_WIDE_MAX=0 BLSGPU_COOP_MAX=0.  Bls12381G2Impl over a set with rows: the table form of the line kernel, ONE k_lines2s
    launch (k_lines2s_shared counts there) where the set without rows takes two; Bls12381G1Impl: one launch, of k_lines2s_keyed over
    the key set with lines"""
    msgsets, keysets, steps, wants = steps_130(sg)
    got = run_worker(tmp_path, 'lane_split_%d' % sg, LANE_SPLIT, msgsets, keysets, steps)
    for g, (want, lines, indexed) in zip(got, wants):
        print(sg, lines, indexed, g['launches'])
        assert g['st'] == want
        nothing_hashed_nothing_built(g['launches'])
        pl = pairing_launches(g['launches'])
        assert pl['k_pairing_coop_rows'] == 0 and pl['k_pairing_coop'] == 0 and pl['k_pairing_coop_keyed'] == 0 and pl['k_wide'] == 0, pl
        assert pl['k_millerf2s'] == 1
        if sg == 2:
            assert (pl['k_lines2s'], pl['k_lines2s_keyed']) == ((1, 0) if lines else (2, 0)), pl
        else:
            assert (pl['k_lines2s'], pl['k_lines2s_keyed']) == ((0, 1) if indexed else (1, 0)), pl


# ------------------------------------------------------------------ 3. the case list
def case_keyset(api, sg, groups):
    """the case list's keys as a wire-format key set with one blob more that does not decode: (blobs, indexed groups, position of the
    bad blob)"""
    raw = mc.raw_groups(sg, groups)
    keys = [p for _, pks, _ in raw for p in pks]
    blobs = api.serialize(3 - sg, keys)
    w = len(blobs[0])
    blobs.append(bytes([blobs[0][0] & 0x9f | 0x1f]) + b'\xff' * (w - 1))          # x >= p
    at, indexed = 0, []
    for idx, pks, sigs in raw:
        indexed.append((idx, list(range(at, at + len(pks))), sigs))
        at += len(pks)
    return blobs, indexed, len(keys)


@pytest.mark.parametrize('sg,scheme', mc.COMBOS, ids=mc.COMBO_IDS)
def test_case_list_default_knobs(api, sg, scheme):
    """the row-wide engine (18 items), by value in both raw formats and indexed, over a set with rows and one without: the oracle's
    status for every item; in the indexed form the message index outranks the key set's two rules"""
    entries, groups, expect = mc.batch(sg, scheme)
    rng = random.Random(7 * sg + scheme)
    nm = mc.names()
    for lines in (False, True):
        with api.MessageSet.create(sg, scheme, entries, lines=lines) as ms:
            info = ms.info()
            assert info == dict(info, sig_group=sg, scheme=scheme, n=len(entries), has_lines=lines and sg == 2)
            assert info['device_bytes'] >= len(entries) * (96 * sg + (ENTRY_LINE_BYTES if info['has_lines'] else 0))
            got, launches = kl.profiled(api, lambda: flat(api.verify_msgset_batch(ms, mc.raw_groups(sg, groups, rng))))
            assert got == expect
            nothing_hashed_nothing_built(launches)
            pl = pairing_launches(launches)
            assert pl == dict(pl, k_wide=1, k_pairing_coop=0, k_pairing_coop_rows=0, k_lines2s=0), pl
            z1 = mc.raw_groups(sg, groups)
            affine = [(i, [vs.aff(3 - sg, p) for p in pks], [vs.aff(sg, s) for s in sigs]) for i, pks, sigs in z1]
            assert flat(api.verify_msgset_batch(ms, affine, fmt=api.FMT_RAW_AFFINE)) == expect
            blobs, indexed, bad = case_keyset(api, sg, groups)
            with api.KeySet.create(sg, blobs, lines=True) as ks:
                assert ks.statuses[bad] == api.BAD_ENCODING
                assert flat(api.verify_msgset_indexed_batch(ms, ks, indexed)) == expect
                # the key set's rules, below the message index: a position outside the table and the undecodable entry, in a group that
                # names an entry and in one that names none
                inside, outside = nm.index('a group of one'), nm.index('entry index past the end')
                for at, pos, want in ((inside, bad + 1, E_ARG), (inside, bad, api.BAD_ENCODING), (outside, bad, E_ARG), (outside, 2 ** 32 - 1, E_ARG)):
                    moved, k = [], 0
                    for idx, ix, sigs in indexed:
                        moved.append((idx, [pos if k + j == at else i for j, i in enumerate(ix)], sigs))
                        k += len(ix)
                    st = flat(api.verify_msgset_indexed_batch(ms, ks, moved))
                    assert st == expect[:at] + [want] + expect[at + 1:], (at, pos)
            assert api.verify_msgset_batch(ms, []) == [] and api.verify_msgset_batch(ms, [(0, [], []), (99, [], [])]) == [[], []]


@pytest.mark.parametrize('env,name', [(ONE_WAVE, 'one_wave'), (LANE_SPLIT, 'lane_split')], ids=['one_wave', 'lane_split'])
def test_case_list_on_the_other_paths_and_after_update_and_append(api, bo, tmp_path, env, name):
    """Bls12381G2Impl with rows and Bls12381G1Impl, ProofOfPossession.  The case list (two groups on one entry, the empty message, an
    index past the end) on the one-wave and the lane-split kernels; then over a set that STARTS with other messages at entries 2
    and 3 and without its last entry, with the group of one moved to that last entry: before, the oracle's statuses under the
    messages the set holds THEN (nothing verifies under a replaced entry's old message; the missing entry is E_ARG); after
    update([3, 2]) and append -- of entry 0's message, so the group of one verifies at its new place -- the statuses of the case
    list, and info reports the grown set, rows included"""
    msgsets, steps, wants = {}, [], {}
    last = len(mc.ENTRIES) - 1
    for sg in (2, 1):
        entries, groups, expect = mc.batch(sg, ref.POP)
        raw = mc.raw_groups(sg, groups, random.Random(sg))
        start = list(entries[:last])
        start[2], start[3] = b'the message entry 2 held before', b'and entry 3'
        moved = [(last if idx == 0 and pks else idx, pks, sigs) for idx, pks, sigs in raw]
        assert sum(1 for (i, _, _), (j, _, _) in zip(raw, moved) if i != j) == 1
        want_before = [E_ARG if idx >= len(start) else bo.bo_verify(sg, ref.POP, pk, sig, start[idx], len(start[idx]))
                       for idx, pks, sigs in moved for pk, sig in zip(pks, sigs)]
        msgsets['final_%d' % sg] = {'sg': sg, 'scheme': ref.POP, 'msgs': entries, 'lines': True}
        msgsets['grown_%d' % sg] = {'sg': sg, 'scheme': ref.POP, 'msgs': start, 'lines': True}
        steps += [{'msgset': 'final_%d' % sg, 'groups': raw}, {'msgset': 'grown_%d' % sg, 'groups': moved}, {'msgset': 'grown_%d' % sg, 'info': True},
                  {'msgset': 'grown_%d' % sg, 'update': ([3, 2], [entries[3], entries[2]])}, {'msgset': 'grown_%d' % sg, 'append': [entries[0]]},
                  {'msgset': 'grown_%d' % sg, 'info': True}, {'msgset': 'grown_%d' % sg, 'groups': moved}, {'msgset': 'grown_%d' % sg, 'groups': raw}]
        wants[sg] = (expect, want_before)
    got = run_worker(tmp_path, 'cases_' + name, env, msgsets, {}, steps)
    nm = mc.names()
    one = nm.index('a group of one')
    for k, sg in enumerate((2, 1)):
        expect, want_before = wants[sg]
        final, before, info0, info1, first, info2, after_moved, after = got[8 * k:8 * (k + 1)]
        for g in (final, before, after_moved, after):
            nothing_hashed_nothing_built(g['launches'])
            pl = pairing_launches(g['launches'])
            if 'BLSGPU_COOP_MAX' in env:
                assert pl['k_lines2s'] == 1 and pl['k_pairing_coop_rows'] == 0 and pl['k_pairing_coop'] == 0 and pl['k_wide'] == 0, pl
            else:
                assert (pl['k_pairing_coop_rows'], pl['k_pairing_coop'], pl['k_wide']) == ((1, 0, 0) if sg == 2 else (0, 1, 0)), pl
        assert final['st'] == expect and after['st'] == expect and after_moved['st'] == expect
        assert before['st'] == want_before
        assert want_before[one] == E_ARG and expect[one] == OK
        changed = [i for i, (a, b) in enumerate(zip(want_before, expect)) if a != b]
        # the group of one, and the four valid items of the groups on entries 2 and 3
        assert len(changed) == 5 and all(want_before[i] in (INVALID, E_ARG) and expect[i] == OK for i in changed)
        assert first == last
        assert (info0['n'], info1['n'], info2['n']) == (last, last, last + 1)
        assert info0['has_lines'] is (sg == 2) and info1['has_lines'] is (sg == 2) and info2['has_lines'] is (sg == 2)
        assert info2['device_bytes'] == info0['device_bytes'] + 96 * sg + (ENTRY_LINE_BYTES + 4 if sg == 2 else 0)


def test_append_across_the_row_cap(api, tmp_path):
    """BLSGPU_KEYSET_TABLE_MB=1 (and the one-wave path, which reads rows): an entry's rows are 15,232 bytes, so 68 entries' rows fit in
    1,048,576 bytes and 69 entries' do not.  64 entries with rows; 4 appended: the rows grow; 1 more: the rows are dropped and the set
    works without them.  After each step info equals that of a set created whole from the same list in the same process, and the
    case list with its groups on the first, the last old, the first new and the last entry gives the oracle's statuses on both sets.
    Entry p holds what entry (p + 3) mod 5 of the case list holds, which keeps the entry no group names off those four."""
    sg, E = 2, len(mc.ENTRIES)
    _, groups, expect = mc.batch(sg, ref.POP)
    raw = mc.raw_groups(sg, groups, random.Random(5))
    entries = [mc.ENTRIES[(p + 3) % E] for p in range(69)]
    assert 68 * ENTRY_LINE_BYTES <= 1 << 20 < 69 * ENTRY_LINE_BYTES

    def moved(n, named):
        """the case list's groups over the first n entries: a group on entry e names one of `named` that holds e's message (the groups
        of an entry taking turns), else the first such entry; the index past the end is n"""
        out, turn = [], {}
        for idx, pks, sigs in raw:
            if idx == mc.PAST_END:
                out.append((n, pks, sigs))
            elif idx >= E:
                out.append((idx, pks, sigs))
            else:
                at = [p for p in named if (p + 3) % E == idx] or [next(p for p in range(n) if (p + 3) % E == idx)]
                out.append((at[turn.get(idx, 0) % len(at)], pks, sigs))
                turn[idx] = turn.get(idx, 0) + 1
        return out

    steps_of = ((64, (0, 63)), (68, (0, 63, 64, 67)), (69, (0, 67, 68)))
    for n, named in steps_of:
        assert set(named) <= {idx for idx, pks, _ in moved(n, named) if pks}, (n, named)
    msgsets = {'grown': {'sg': sg, 'scheme': ref.POP, 'msgs': entries[:64], 'lines': True}}
    steps = []
    for n, named in steps_of:
        msgsets['whole_%d' % n] = {'sg': sg, 'scheme': ref.POP, 'msgs': entries[:n], 'lines': True}
        if n > 64:
            steps.append({'msgset': 'grown', 'append': entries[n - (4 if n == 68 else 1):n]})
        for name in ('grown', 'whole_%d' % n):
            steps += [{'msgset': name, 'info': True}, {'msgset': name, 'groups': moved(n, named)}]
    got = run_worker(tmp_path, 'cap', dict(ONE_WAVE, BLSGPU_KEYSET_TABLE_MB='1'), msgsets, {}, steps)
    assert got[4] == 64 and got[9] == 68
    for (n, _), (i_g, v_g, i_w, v_w) in zip(steps_of, (got[0:4], got[5:9], got[10:14])):
        assert i_g == i_w == dict(i_w, sig_group=2, scheme=ref.POP, n=n, has_lines=n <= 68), (n, i_g, i_w)
        assert i_g['device_bytes'] == n * (192 + (ENTRY_LINE_BYTES + 4 if n <= 68 else 0))
        for v in (v_g, v_w):
            assert v['st'] == expect, n
            nothing_hashed_nothing_built(v['launches'])
            pl = pairing_launches(v['launches'])
            assert (pl['k_pairing_coop_rows'], pl['k_pairing_coop']) == ((1, 0) if n <= 68 else (0, 1)), (n, pl)


# ------------------------------------------------------------------ 4. default knobs, every size branch
@pytest.mark.parametrize('n', [1, 3, 65])
@pytest.mark.parametrize('sg', [1, 2])
def test_engine_sizes(api, bo, sg, n):
    """1, 3 and 65 items in three groups over a set with rows: the row-wide engine runs, which reads no rows"""
    groups, expect = vs.signed_batch(sg, ref.BASIC, (n - n // 2 - n // 3, n // 3, n // 2))
    vs.oracle_sample(bo, sg, ref.BASIC, groups, expect)
    with api.MessageSet.create(sg, ref.BASIC, [m for m, _, _ in groups], lines=True) as ms:
        got, launches = kl.profiled(api, lambda: flat(api.verify_msgset_batch(ms, [(g, pks, sigs) for g, (_, pks, sigs) in enumerate(groups)])))
    assert got == expect
    nothing_hashed_nothing_built(launches)
    pl = pairing_launches(launches)
    assert pl == dict(pl, k_wide=1, k_pairing_coop=0, k_pairing_coop_rows=0, k_lines2s=0), pl


def test_513_items_default_knobs(api, bo):
    """513 items of Bls12381G2Impl in three unequal groups, one run: the tamper pattern, confirmed by the oracle on 64 spread items;
    k_pairing_coop_rows ran once"""
    groups, expect = vs.signed_batch(2, ref.BASIC, (171, 172, 170))
    vs.oracle_sample(bo, 2, ref.BASIC, groups, expect)
    with api.MessageSet.create(2, ref.BASIC, [m for m, _, _ in groups], lines=True) as ms:
        assert ms.info()['has_lines'] is True
        got, launches = kl.profiled(api, lambda: flat(api.verify_msgset_batch(ms, [(g, pks, sigs) for g, (_, pks, sigs) in enumerate(groups)])))
    bad = [(i, got[i], expect[i]) for i in range(513) if got[i] != expect[i]][:10]
    assert not bad and len(got) == 513, bad
    nothing_hashed_nothing_built(launches)
    pl = pairing_launches(launches)
    assert pl == dict(pl, k_pairing_coop_rows=1, k_pairing_coop=0, k_lines2s=0, k_wide=0), pl


# ------------------------------------------------------------------ 5. the object and the arguments
def test_create_update_append_arguments(api):
    lib = api.init()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    u64 = lambda v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    h = ctypes.c_uint64(7)
    blob = b'abcdef'
    for sg, scheme, flags in ((1, ref.AUG, 0), (2, ref.AUG, 1), (0, ref.POP, 0), (3, ref.POP, 0), (2, 3, 0), (2, ref.POP, 2), (2, ref.POP, -1)):
        assert lib.blsgpu_msgset_create(sg, scheme, api._ptr(blob), p(u64([0, 3, 6])), 2, flags, ctypes.byref(h)) == E_ARG and h.value == 7, (sg, scheme, flags)
    with pytest.raises(Exception):
        api.MessageSet.create(2, ref.AUG, [b'm'])                                    # MessageAugmentation: nothing to register
    assert lib.blsgpu_msgset_create(2, ref.POP, api._ptr(blob), p(u64([0, 4, 3])), 2, 0, ctypes.byref(h)) == E_ARG and h.value == 0     # decreasing offsets
    with api.MessageSet.create(2, ref.POP, [], lines=True) as empty:
        assert empty.info() == dict(empty.info(), n=0, has_lines=False)
        assert empty.append([b'x', b'']) == 0
        assert empty.info() == dict(empty.info(), n=2, has_lines=True)                # rows the creator asked for, built once there are entries
    with api.MessageSet.create(1, ref.BASIC, [b'a', b'b'], lines=True) as g1:         # messages in G1 have no lines: accepted, nothing built
        assert g1.info()['has_lines'] is False
    with api.MessageSet.create(2, ref.POP, [b'a', b'b', b'c'], lines=True) as ms:
        before = ms.info()
        for pos, msgs in (([3], [b'x']), ([0, 0], [b'x', b'y']), ([0, 1, 2, 0], [b'x'] * 4)):
            with pytest.raises(Exception):
                ms.update(pos, msgs)                                                  # outside the set, named twice, more positions than entries
        assert lib.blsgpu_msgset_update(ms.handle, p((ctypes.c_uint32 * 2)(0, 1)), api._ptr(blob), p(u64([0, 4, 3])), 2) == E_ARG
        assert lib.blsgpu_msgset_append(ms.handle, api._ptr(blob), p(u64([0, 4, 3])), 2, None) == E_ARG
        assert ms.info() == before
        ms.update([], [])
        assert ms.append([]) == 3 and ms.info() == before
        dead = ms.handle
    assert lib.blsgpu_msgset_destroy(dead) == E_ARG and lib.blsgpu_msgset_destroy(0) == E_ARG
    assert lib.blsgpu_msgset_info(dead, None, None, None, None, None) == E_ARG
    assert lib.blsgpu_msgset_update(dead, p((ctypes.c_uint32 * 1)(0)), api._ptr(blob), p(u64([0, 1])), 1) == E_ARG
    assert lib.blsgpu_msgset_append(dead, api._ptr(blob), p(u64([0, 1])), 1, None) == E_ARG


def test_verify_arguments_write_no_status(api):
    lib = api.init()
    groups, _ = vs.signed_batch(2, ref.POP, (2, 1))
    pkb, sgb = b''.join(x for g in groups for x in g[1]), b''.join(s for g in groups for s in g[2])
    st = (ctypes.c_int32 * 3)(-7, -7, -7)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    u64 = lambda v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    midx = (ctypes.c_uint32 * 2)(0, 1)
    keys1 = [x for g in vs.signed_batch(1, ref.POP, (2, 1))[0] for x in g[1]]
    keys2 = [x for g in groups for x in g[1]]
    with api.MessageSet.create(2, ref.POP, [g[0] for g in groups]) as ms, api.KeySet.create(1, keys1, api.FMT_RAW_PROJ) as other, \
            api.KeySet.create(2, keys2, api.FMT_RAW_PROJ) as ks:

        def call(ioffs, handle=ms.handle, fmt=0, n_groups=2):
            return lib.blsgpu_verify_msgset_batch(handle, p(midx), api._ptr(pkb), api._ptr(sgb), p(u64(ioffs)), n_groups, fmt, p(st))

        def call_indexed(keyset, ioffs=(0, 2, 3), handle=ms.handle):
            return lib.blsgpu_verify_msgset_indexed_batch(handle, p(midx), keyset, p((ctypes.c_uint32 * 3)(0, 1, 2)), api._ptr(sgb), p(u64(ioffs)), 2, 0, p(st))
        assert call([0, 3, 2]) == E_ARG                               # offsets that decrease
        assert call([1, 2, 3]) == E_ARG                               # ... that do not start at 0
        assert call([0, 2, 2 ** 32]) == E_ARG                         # 2^32 items
        assert call([0, 2, 3], fmt=api.FMT_COMPRESSED) == E_ARG
        assert call([0, 2, 3], handle=ks.handle) == E_ARG             # a key set's handle is no message set's
        assert call_indexed(other.handle) == E_ARG                    # a key set of the other orientation
        assert call_indexed(ms.handle) == E_ARG and call_indexed(0) == E_ARG
        assert call_indexed(ks.handle, ioffs=(0, 3, 2)) == E_ARG
        assert lib.blsgpu_verify_msgset_batch(ms.handle, None, None, None, None, 2, 0, None) == E_ARG
        assert list(st) == [-7, -7, -7]
        assert lib.blsgpu_verify_msgset_batch(ms.handle, None, None, None, None, 0, 0, None) == 0      # no groups
        assert call([0, 0, 0]) == 0 and list(st) == [-7, -7, -7]      # no items
        assert call([0, 2, 3]) == 0 and list(st) == [0, 0, 0]
        st[0] = st[1] = st[2] = -7
        assert call_indexed(ks.handle) == 0 and list(st) == [0, 0, 0]
        dead = ms.handle
    st[0] = st[1] = st[2] = -7
    assert call([0, 2, 3], handle=dead) == E_ARG and list(st) == [-7, -7, -7]       # a destroyed handle


@pytest.mark.parametrize('sg', [1, 2])
def test_device_pointers(api, sg):
    """message indices, keys, signatures, offsets and the statuses on the device (TensorOps), by value and over a key set; the set
    itself created from device memory"""
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    entries, by_value, indexed, keys, want = reference_130(sg, ref.POP)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)  # noqa: E731
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)  # noqa: E731
    ioffs, moffs = [0], [0]
    for _, pks, _ in by_value:
        ioffs.append(ioffs[-1] + len(pks))
    for m in entries:
        moffs.append(moffs[-1] + len(m))
    n = ioffs[-1]
    pk_t, sig_t = tens(b''.join(keys)), tens(b''.join(s for g in by_value for s in g[2]))
    msg_t, moff_t = tens(b''.join(entries)), i64(moffs)
    midx = torch.tensor([g[0] for g in by_value], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with api.MessageSet.create_device(sg, ref.POP, msg_t.data_ptr(), moff_t.data_ptr(), len(entries), lines=True) as ms:
        assert ms.info()['n'] == len(entries) and ms.info()['has_lines'] is (sg == 2)
        st = ops.verify_msgset_batch(ms, midx, pk_t, sig_t, i64(ioffs), len(by_value), n)
        assert st.device == dev and st.dtype == torch.int32 and st.cpu().tolist() == want
        with api.KeySet.create(sg, keys, api.FMT_RAW_PROJ) as kset:
            idx = torch.arange(n, dtype=torch.int32, device=dev)
            st = ops.verify_msgset_indexed_batch(ms, midx, kset, idx, sig_t, i64(ioffs), len(by_value), n)
            assert st.device == dev and st.cpu().tolist() == want
