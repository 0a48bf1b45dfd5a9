"""Registered key sets with per-key line tables (BLSGPU_KEYSET_LINES) on the GPU: creation and info, and the one-key-per-item indexed
calls (blsgpu_verify_indexed_batch, blsgpu_verify_shared_indexed_batch) of Bls12381G1Impl, whose lane-split path then reads both
Miller lines from tables (k_lines2s_keyed) where it walked the key (k_lines2s).  Expected statuses are the C oracle's, one
verification per item under the key its position names, with the precedence of the indexed calls for the bad positions; for the
larger batches the pattern the batch was tampered with, confirmed by the oracle on a sample.  The kernel launch counts of the
profile say which line kernel ran, so no test can pass by falling back.  Runs that need their own process (the knobs are read once)
go through tests/keyset_lines_worker.py: one attempt each, with its own time limit."""
import ctypes
import functools
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

import keyset_cases as kc
import util
from util import ref

pytestmark = pytest.mark.gpu

E_ARG = -3
OK, INVALID, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
KEY_LINE_BYTES = 68 * 4 * 14 * 4                  # 15,232
SCHEMES = [(ref.POP, 'pop'), (ref.BASIC, 'basic'), (ref.AUG, 'aug')]
LANE_SPLIT = {'BLSGPU_COOP_MAX': '0'}
GROUP_SIZES = (1, 0, 31, 33, 0, 65)               # group borders inside a wave, on a workgroup border and across it


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


def run_worker(tmp_path, name, env, sets, calls, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'sets': sets, 'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'keyset_lines_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def table_sets(t, **which):
    """worker set specs over the 320-entry table: name -> lines flag"""
    return {name: {'sg': 1, 'keys': t['blobs'], 'fmt': t['fmt'], 'tables': False, 'lines': lines} for name, lines in which.items()}


def sign(api, scheme, secrets, msgs):
    """sk_i H(m_i) (MessageAugmentation: H(pk_i || m_i)), signed on the device"""
    return api.sign_batch(1, scheme, secrets, msgs)[1]


# ------------------------------------------------------------------ the 130 items of the lane-split tests
TAMPERED, WRONG_MSG, ID_SIG, AT_IDENT, AT_BAD, PAST_END, AT_DUP_A, AT_DUP_B, AT_GEN, PAST_END_ID_SIG = 3, 6, 13, 20, 33, 64, 70, 71, 100, 129


def item_indices(t, n, rng):
    idx = [rng.choice(t['valid']) for _ in range(n)]
    idx[AT_IDENT], idx[AT_BAD], idx[PAST_END], idx[AT_DUP_A], idx[AT_DUP_B], idx[AT_GEN], idx[PAST_END_ID_SIG] = \
        kc.IDENT, kc.BAD, kc.N, kc.DUP_A, kc.DUP_B, kc.GEN, kc.N
    return idx


def items_130(api, scheme, msgs):
    """(idx, sigs, msgs as verified): valid items, a tampered signature, a wrong message, the identity signature, the identity entry,
    the invalid entry, an index equal to the table size (once more under an identity signature: the index still decides), the
    duplicated key at both positions, the generator"""
    t = kc.table(api, 1)
    rng = random.Random(130 + scheme)
    idx = item_indices(t, 130, rng)
    secrets = [t['ks'][i] if i < kc.N and t['ks'][i] else 4242 for i in idx]          # entries without a secret: some finite signature
    sigs = sign(api, scheme, secrets, msgs)
    sigs[TAMPERED] = sigs[TAMPERED + 1]
    sigs[ID_SIG] = sigs[PAST_END_ID_SIG] = kc.mb.identity(1)
    return idx, sigs


def oracle_item(bo, api, t, scheme, ix, sig, m):
    """the status of one item: the precedence of the indexed calls, then the C oracle under the entry's key"""
    if ix >= kc.N:
        return E_ARG
    if t['status'][ix]:
        return t['status'][ix]
    return bo.bo_verify(1, scheme, t['points'][ix], sig, m, len(m))


@functools.lru_cache(maxsize=None)
def indexed_reference(scheme):
    """verify_indexed_batch's 130 items and the ORACLE's status of every one (computed once per scheme, shared by the plans)"""
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    t = kc.table(api, 1)
    signed = [b'keyed item %d' % i for i in range(130)]
    idx, sigs = items_130(api, scheme, signed)
    msgs = list(signed)
    msgs[WRONG_MSG] = b'another message'
    bo = util.load_c_oracle()
    want = [oracle_item(bo, api, t, scheme, ix, s, m) for ix, s, m in zip(idx, sigs, msgs)]
    for i, w in ((TAMPERED, INVALID), (WRONG_MSG, INVALID), (ID_SIG, SIG_IDENTITY), (AT_IDENT, PK_IDENTITY), (AT_BAD, api.BAD_ENCODING), (PAST_END, E_ARG),
                 (PAST_END_ID_SIG, E_ARG), (AT_DUP_A, OK), (AT_DUP_B, OK), (AT_GEN, OK)):
        assert want[i] == w, (i, want[i], w)
    assert sum(1 for w in want if w == OK) == 130 - 7
    return {'idx': idx, 'sigs': sigs, 'msgs': msgs}, want


@functools.lru_cache(maxsize=None)
def shared_reference(scheme):
    """the same items in groups of 1, 0, 31, 33, 0, 65 under one message per group, and the oracle's statuses"""
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    t = kc.table(api, 1)
    gmsgs = [b'keyed group %d' % g if g != 2 else b'' for g in range(len(GROUP_SIZES))]
    item_msg = [gmsgs[g] for g, s in enumerate(GROUP_SIZES) for _ in range(s)]
    idx, sigs = items_130(api, scheme, item_msg)
    sigs[WRONG_MSG] = sign(api, scheme, [t['ks'][idx[WRONG_MSG]]], [b'another message'])[0]
    bo = util.load_c_oracle()
    want = [oracle_item(bo, api, t, scheme, ix, s, m) for ix, s, m in zip(idx, sigs, item_msg)]
    assert [want[i] for i in (TAMPERED, WRONG_MSG, ID_SIG, AT_IDENT, AT_BAD, PAST_END)] == [INVALID, INVALID, SIG_IDENTITY, PK_IDENTITY, api.BAD_ENCODING, E_ARG]
    groups, at = [], 0
    for g, s in enumerate(GROUP_SIZES):
        groups.append((gmsgs[g], idx[at:at + s], sigs[at:at + s]))
        at += s
    return groups, want


def line_launches(got):
    return got['launches'].get('k_lines2s_keyed', 0), got['launches'].get('k_lines2s', 0), got['launches'].get('k_millerf2s', 0)


# ------------------------------------------------------------------ 1. create and info
def test_create_and_info(api):
    t1, t2 = kc.table(api, 1), kc.table(api, 2)
    with api.KeySet.create(1, t1['blobs'], t1['fmt']) as plain, api.KeySet.create(1, t1['blobs'], t1['fmt'], lines=True) as ks:
        base, info = plain.info(), ks.info()
        assert base['has_lines'] is False and base['has_tables'] is False
        assert info['has_lines'] is True and info['has_tables'] is False and ks.statuses == plain.statuses
        assert info['device_bytes'] >= base['device_bytes'] + kc.N * KEY_LINE_BYTES
        assert ks.get(list(range(kc.N)), api.FMT_COMPRESSED) == plain.get(list(range(kc.N)), api.FMT_COMPRESSED)
    with api.KeySet.create(1, t1['blobs'], t1['fmt'], tables=True) as tab, api.KeySet.create(1, t1['blobs'], t1['fmt'], tables=True, lines=True) as both:
        a, b = tab.info(), both.info()
        assert a['has_tables'] is True and a['has_lines'] is False and b['has_tables'] is True and b['has_lines'] is True
        assert b['device_bytes'] >= a['device_bytes'] + kc.N * KEY_LINE_BYTES
        mask = ctypes.c_int(0)
        assert api.init().blsgpu_keyset_info(both.handle, None, None, ctypes.byref(mask), None) == 0 and mask.value == 3
        assert api.init().blsgpu_keyset_info(tab.handle, None, None, ctypes.byref(mask), None) == 0 and mask.value == 1       # what flags 1 saw before
    with api.KeySet.create(2, t2['blobs'], t2['fmt'], lines=True) as g1keys:              # keys in G1 have no lines: accepted, nothing built
        assert g1keys.info()['has_lines'] is False and g1keys.info()['has_tables'] is False
    with api.KeySet.create(1, [], lines=True) as empty:
        assert empty.info()['has_lines'] is False and empty.info()['n'] == 0
    h = ctypes.c_uint64(7)
    blob = b''.join(t1['blobs'])
    for flags in (4, 6, 8, -1):
        assert api.init().blsgpu_keyset_create(1, api._ptr(blob), kc.N, t1['fmt'], flags, None, ctypes.byref(h)) == E_ARG and h.value == 7, flags


# ------------------------------------------------------------------ 2. the keyed form on the lane-split path
@pytest.mark.parametrize('scheme,_id', SCHEMES, ids=[s[1] for s in SCHEMES])
def test_keyed_form_on_the_lane_split_path(api, tmp_path, scheme, _id):
    """130 items, BLSGPU_COOP_MAX=0: over the set with lines the keyed kernel runs once and k_lines2s not at all; (a) over the set
    without lines k_lines2s runs once and the keyed kernel not at all; the oracle's statuses both times"""
    call, want = indexed_reference(scheme)
    t = kc.table(api, 1)
    got = run_worker(tmp_path, 'keyed', LANE_SPLIT, table_sets(t, lines=True, plain=False),
                     [dict(call, set='lines', scheme=scheme), dict(call, set='plain', scheme=scheme)])
    assert got['sets']['lines']['has_lines'] is True and got['sets']['plain']['has_lines'] is False
    keyed, plain = got['calls']
    print(keyed['launches'], plain['launches'])
    assert keyed['st'] == want and plain['st'] == want
    assert line_launches(keyed) == (1, 0, 1)
    assert line_launches(plain) == (0, 1, 1)


def test_keyed_form_across_chunk_borders(api, tmp_path):
    """(b) 64-item chunks: three chunks, so a border falls inside the batch -- the key and the record are the item's in the BATCH"""
    call, want = indexed_reference(ref.POP)
    t = kc.table(api, 1)
    env = dict(LANE_SPLIT, BLSGPU_AB_KNOBS='1', BLSGPU_MILLER_CHUNK='64')
    got = run_worker(tmp_path, 'chunks', env, table_sets(t, lines=True), [dict(call, set='lines', scheme=ref.POP)])['calls'][0]
    assert got['st'] == want
    assert line_launches(got) == (3, 0, 3)


def test_refused_lines_change_nothing(api, tmp_path):
    """(c) BLSGPU_KEYSET_TABLE_MB=1: 4.6 MiB of rows are refused, the set works without them"""
    call, want = indexed_reference(ref.POP)
    t = kc.table(api, 1)
    got = run_worker(tmp_path, 'refused', dict(LANE_SPLIT, BLSGPU_KEYSET_TABLE_MB='1'), table_sets(t, lines=True), [dict(call, set='lines', scheme=ref.POP)])
    assert got['sets']['lines']['has_lines'] is False
    assert got['calls'][0]['st'] == want
    assert line_launches(got['calls'][0]) == (0, 1, 1)


# ------------------------------------------------------------------ 3. shared-message verify over a set with lines
def test_shared_indexed_takes_the_keyed_form(api, tmp_path):
    """groups of 1, 0, 31, 33, 0, 65 items on the lane-split path: the hash is shared per group, the key's rows are read per item;
    MessageAugmentation (nothing shared: the items run as verify_batch runs them) reads them as well"""
    t = kc.table(api, 1)
    calls, wants = [], []
    for scheme in (ref.POP, ref.AUG):
        groups, want = shared_reference(scheme)
        calls.append({'set': 'lines', 'scheme': scheme, 'groups': groups})
        wants.append(want)
    got = run_worker(tmp_path, 'shared', LANE_SPLIT, table_sets(t, lines=True), calls)['calls']
    for g, want in zip(got, wants):
        assert g['st'] == want
        assert line_launches(g) == (1, 0, 1)


# ------------------------------------------------------------------ 4, 5. default knobs
def tamper_kind(i):
    """about one item in eight: 1 = the next item's signature, 2 = the identity signature, 3 = the identity entry, 4 = the invalid
    entry, 5 = a position outside the table"""
    return {3: 1, 13: 2, 23: 3, 33: 4, 37: 5}.get(i % 40, 0)


@functools.lru_cache(maxsize=None)
def signed_batch(n):
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    t = kc.table(api, 1)
    rng = random.Random(n)
    idx = [rng.choice(t['valid']) for _ in range(n)]
    msgs = [b'default knobs %d' % (i % 97) for i in range(n)]
    sigs = sign(api, ref.POP, [t['ks'][i] for i in idx], msgs)
    orig = list(sigs)
    expect = []
    for i in range(n):
        k = tamper_kind(i)
        if k == 1:
            sigs[i] = orig[(i + 1) % n]
        elif k == 2:
            sigs[i] = kc.mb.identity(1)
        elif k >= 3:
            idx[i] = {3: kc.IDENT, 4: kc.BAD, 5: kc.N + i}[k]
        expect.append({0: OK, 1: INVALID, 2: SIG_IDENTITY, 3: PK_IDENTITY, 4: api.BAD_ENCODING, 5: E_ARG}[k])
    return idx, sigs, msgs, expect


def spot(bo, api, n, k=24):
    """the C oracle on k items spread over the batch (the first tampered ones and both ends among them): they must equal the pattern"""
    idx, sigs, msgs, expect = signed_batch(n)
    t = kc.table(api, 1)
    pick = sorted(set(range(n)) if n <= k else set(random.Random(n).sample(range(n), k - 9)) | {0, 3, 13, 23, 33, 37, n - 1, n - 2, n // 2})
    for i in pick:
        assert oracle_item(bo, api, t, ref.POP, idx[i], sigs[i], msgs[i]) == expect[i], i


def profiled(api, fn):
    """fn() with the profile on: (result, {kernel: launches of this call})"""
    api.profile_enable(True)
    try:
        before = {k: v[1] for k, v in api.profile_read().items()}
        out = fn()
        now = {k: v[1] for k, v in api.profile_read().items()}
    finally:
        api.profile_enable(False)
    return out, {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def test_default_knobs_past_coop_max(api, bo):
    """4,097 items (just past BLSGPU_COOP_MAX) over a set with lines: the statuses equal the tamper pattern, which the oracle confirms
    on 24 items, and the keyed kernel ran"""
    n = 4097
    idx, sigs, msgs, expect = signed_batch(n)
    spot(bo, api, n)
    t = kc.table(api, 1)
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        assert ks.info()['has_lines'] is True
        got, launches = profiled(api, lambda: api.verify_indexed_batch(ks, ref.POP, idx, sigs, msgs))
    bad = [(i, got[i], expect[i]) for i in range(n) if got[i] != expect[i]][:10]
    assert not bad and len(got) == n, bad
    assert launches.get('k_lines2s_keyed', 0) == 1 and launches.get('k_lines2s', 0) == 0, launches


@pytest.mark.parametrize('n', [64, 1025])
def test_engine_and_wave_paths_ignore_the_table(api, bo, n):
    """default knobs below BLSGPU_COOP_MAX (the row-wide engine at 64 items, one wave per item at 1,025) over a set with lines: the
    tamper pattern, confirmed by the oracle on every item (64) or on 24 of them (1,025); no line kernel runs at all"""
    idx, sigs, msgs, expect = signed_batch(n)
    spot(bo, api, n, k=64 if n == 64 else 24)
    t = kc.table(api, 1)
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        assert ks.info()['has_lines'] is True
        got, launches = profiled(api, lambda: api.verify_indexed_batch(ks, ref.POP, idx, sigs, msgs))
    assert got == expect
    assert launches.get('k_lines2s_keyed', 0) == 0 and launches.get('k_lines2s', 0) == 0, launches


# ------------------------------------------------------------------ 6. an entry without usable rows
def test_fallback_when_a_named_entry_has_no_rows(api, tmp_path):
    """RAW_AFFINE keys (trusted), one entry (x of a real key, 0): finite, and its first tangent is vertical, so it has no rows.  A
    lane-split call that names it walks the keys of ALL its items -- exactly the statuses of the same call on a set without lines,
    by k_lines2s; a call that does not name it takes the keyed kernel"""
    call, want = indexed_reference(ref.POP)
    t = kc.table(api, 1)
    Y0 = next(i for i in t['valid'] if i not in call['idx'] and i not in (kc.GEN, kc.DUP_A, kc.DUP_B))
    aff = [bytes(192) if k in (0, None) else p[:192] for p, k in zip(t['points'], t['ks'])]
    aff[Y0] = aff[Y0][:96] + bytes(96)
    sets = {name: {'sg': 1, 'keys': aff, 'fmt': api.FMT_RAW_AFFINE, 'tables': False, 'lines': lines} for name, lines in (('lines', True), ('plain', False))}
    naming = dict(call, idx=list(call['idx']))
    naming['idx'][50] = naming['idx'][90] = Y0
    got = run_worker(tmp_path, 'fallback', LANE_SPLIT, sets, [dict(naming, set='lines', scheme=ref.POP), dict(naming, set='plain', scheme=ref.POP),
                                                              dict(call, set='lines', scheme=ref.POP)])
    assert got['sets']['lines']['has_lines'] is True
    walked, plain, keyed = got['calls']
    # raw input is trusted: the undecodable blob of the wire table is the zero record here, an identity entry
    want_raw = [PK_IDENTITY if i == AT_BAD else w for i, w in enumerate(want)]
    assert walked['st'] == plain['st']
    assert [s for i, s in enumerate(walked['st']) if i not in (50, 90)] == [s for i, s in enumerate(want_raw) if i not in (50, 90)]
    assert walked['st'][50] != OK and walked['st'][90] != OK
    assert line_launches(walked) == (0, 1, 1) and line_launches(plain) == (0, 1, 1)
    assert keyed['st'] == want_raw
    assert line_launches(keyed) == (1, 0, 1)
