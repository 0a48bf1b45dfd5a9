"""Registered key sets that change in place (blsgpu_keyset_update, blsgpu_keyset_append) on the GPU.  The specification is one
equivalence: after either call the set is indistinguishable, through every existing call, from a set freshly created from the final
key list with the same flags.  So every test builds both sets and compares them -- entries in two formats, statuses, info(), scalar
multiples, every indexed entry point -- and holds the results against something that does not come from a key set at all: the C
oracle under the entry's key, the closed-form multiple of a known secret, the by-value call on the gathered keys.  The kernel launch
counts of the profile say which form ran (the positional k_keyset_*_at kernels, the keyed or the walking line kernel).  Runs that need
their own knobs go through tests/keyset_update_worker.py: one attempt each, with its own time limit."""
import ctypes
import functools
import itertools
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

import keyset_cases as kc
import util
from secure_coeffs import aggregate_secret
from util import ref

pytestmark = pytest.mark.gpu

E_ARG = -3
OK, INVALID, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
R = kc.R
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
FLAG_IDS = ['plain', 'tables', 'lines', 'both']
LANE_SPLIT = {'BLSGPU_COOP_MAX': '0'}
TO_IDENT, TO_BAD = 100, 150                        # finite entries of kc.table that an update turns into the identity / an undecodable blob
# one update, unsorted: the generator, the last entry, a run across a wave border, and the five transitions
POS = [65, kc.GEN, kc.N - 1, 63, kc.IDENT, TO_BAD, 64, kc.BAD, TO_IDENT, kc.DUP_B]
NEIGHBOURS = sorted({p + d for p in POS for d in (-1, 1) if 0 <= p + d < kc.N} - set(POS))


def ident_blob(g):
    return b'\xc0' + bytes(48 * g - 1)


def bad_blob(g):
    return b'\x9f' + b'\xff' * (48 * g - 1)       # compressed, finite, x >= p


def get_api():
    from __graft_entry__ import import_pkg
    return import_pkg().api


@functools.lru_cache(maxsize=None)
def final(sg):
    """kc.table(sg) after the update POS: dict(pos, keys: the blobs handed to update, and ks, blobs, fmt, status, points, valid of
    the FINAL table, as kc.table has them).  Computed once per key group and never changed."""
    api = get_api()
    t = kc.table(api, sg)
    g = 3 - sg
    rng = random.Random(2000 + sg)
    ks = list(t['ks'])
    for p in POS:
        ks[p] = rng.randrange(2, R)
    ks[TO_IDENT], ks[TO_BAD] = 0, None
    assert t['ks'][TO_IDENT] and t['ks'][TO_BAD] and ks[kc.DUP_B] != ks[kc.DUP_A]
    finite = [p for p in POS if ks[p]]
    made = dict(zip(finite, api.serialize(g, kc.mb.key_points(api, sg, [ks[p] for p in finite]))))
    made[TO_IDENT], made[TO_BAD] = ident_blob(g), bad_blob(g)
    blobs = list(t['blobs'])
    for p in POS:
        blobs[p] = made[p]
    pts, status = api.deserialize(g, blobs)
    assert [i for i, s in enumerate(status) if s] == [TO_BAD] and status[TO_BAD] == api.BAD_ENCODING
    return dict(pos=list(POS), keys=[made[p] for p in POS], ks=ks, blobs=blobs, fmt=api.FMT_COMPRESSED, status=status, points=pts,
                valid=[i for i, k in enumerate(ks) if k])


def same_set(api, a, b, n):
    """every entry in two formats, the statuses and info(): a and b are one set"""
    everything = list(range(n))
    for fmt in (api.FMT_COMPRESSED, api.FMT_RAW_AFFINE):
        assert a.get(everything, fmt) == b.get(everything, fmt), fmt
    assert a.statuses == b.statuses
    ia, ib = a.info(), b.info()
    assert ia == ib and ia['n'] == n, (ia, ib)
    return ia


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


def run_worker(tmp_path, name, env, sets, steps, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'sets': sets, 'steps': steps}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'keyset_update_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])['steps']


def line_launches(got):
    return got['launches'].get('k_lines2s_keyed', 0), got['launches'].get('k_lines2s', 0)


# ------------------------------------------------------------------ 1. equivalence with fresh creation
@pytest.mark.parametrize('tables,lines', FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize('sg', [1, 2])
def test_update_is_fresh_creation(api, sg, tables, lines):
    t, f = kc.table(api, sg), final(sg)
    with api.KeySet.create(sg, t['blobs'], t['fmt'], tables=tables, lines=lines) as ks, \
            api.KeySet.create(sg, f['blobs'], f['fmt'], tables=tables, lines=lines) as fresh:
        st, launches = profiled(api, lambda: ks.update(f['pos'], f['keys']))
        assert st == api.deserialize(3 - sg, f['keys'])[1] and st == [f['status'][p] for p in f['pos']]
        info = same_set(api, ks, fresh, kc.N)
        assert (info['has_tables'], info['has_lines']) == (tables, lines and sg == 1)
        assert ks.statuses == f['status']
        assert ks.get(list(range(kc.N)), api.FMT_COMPRESSED)[0] == [ident_blob(3 - sg) if s else b for b, s in zip(f['blobs'], f['status'])]
        print(launches)
        assert launches.get('k_keyset_seal_at') == 1 and not launches.get('k_keyset_seal')
        assert launches.get('k_keyset_build_at', 0) == int(tables) and launches.get('k_keyset_lines_at', 0) == int(lines and sg == 1)


# ------------------------------------------------------------------ 2. tables
@pytest.mark.parametrize('sg', [1, 2])
def test_tables_after_update(api, sg):
    """scalar times entry over the updated positions and their neighbours: the updated tables, fresh tables and the ladder agree, and
    agree with the closed form (k s) g for an entry of secret s"""
    g = 3 - sg
    t, f = kc.table(api, sg), final(sg)
    where = f['pos'] + NEIGHBOURS
    pairs = [(p, s) for p in where for s in kc.SPECIAL_SCALARS]
    idx, sc = [p for p, _ in pairs], [s for _, s in pairs]
    with api.KeySet.create(sg, t['blobs'], t['fmt'], tables=True) as ks, api.KeySet.create(sg, f['blobs'], f['fmt'], tables=True) as fresh, \
            api.KeySet.create(sg, f['blobs'], f['fmt']) as ladder:
        _, launches = profiled(api, lambda: ks.update(f['pos'], f['keys']))
        assert launches.get('k_keyset_build_at') == 1 and not launches.get('k_keyset_build'), launches
        assert ks.info()['has_tables'] and fresh.info()['has_tables'] and not ladder.info()['has_tables']
        got = api.serialize(g, ks.mul(idx, sc))
        assert got == api.serialize(g, fresh.mul(idx, sc))
        assert got == api.serialize(g, ladder.mul(idx, sc))
    ident = api.serialize(g, [kc.mb.identity(g)])[0]
    live = [i for i, (p, s) in enumerate(pairs) if f['ks'][p] and s % R]
    closed = api.serialize(g, kc.mb.key_points(api, sg, [f['ks'][pairs[i][0]] * pairs[i][1] % R for i in live]))
    assert [got[i] for i in live] == closed
    assert all(got[i] == ident for i in range(len(pairs)) if i not in set(live))


# ------------------------------------------------------------------ 3, 4. lines
OLD_SECRET, AT_NEW_IDENT, AT_NEW_BAD = 12, 13, 14


@functools.lru_cache(maxsize=None)
def items_after_update():
    """130 items over the FINAL table of Bls12381G1Impl and the C oracle's status of each under the indexed precedence: slots 0..7 the
    updated finite entries (signed with their NEW secrets), then four untouched neighbours, entry 65 under a signature by its OLD
    secret, the new identity entry, the new invalid entry, then random finite entries; one tampered signature among those"""
    api = get_api()
    t, f = kc.table(api, 1), final(1)
    rng = random.Random(131)
    idx = [p for p in POS if f['ks'][p]] + [62, 66, kc.N - 2, 1] + [65, TO_IDENT, TO_BAD]
    assert len(idx) == 15 and idx[OLD_SECRET] == 65
    idx += [rng.choice(f['valid']) for _ in range(130 - len(idx))]
    msgs = [b'updated item %d' % i for i in range(130)]
    secrets = [f['ks'][i] or 4242 for i in idx]
    secrets[OLD_SECRET] = t['ks'][65]
    sigs = api.sign_batch(1, ref.POP, secrets, msgs)[1]
    sigs[77] = sigs[78]
    bo = util.load_c_oracle()
    want = [f['status'][ix] or bo.bo_verify(1, ref.POP, f['points'][ix], s, m, len(m)) for ix, s, m in zip(idx, sigs, msgs)]
    assert [want[i] for i in (OLD_SECRET, AT_NEW_IDENT, AT_NEW_BAD, 77)] == [INVALID, PK_IDENTITY, api.BAD_ENCODING, INVALID]
    assert sum(1 for w in want if w == OK) == 126
    return {'scheme': ref.POP, 'idx': idx, 'sigs': sigs, 'msgs': msgs}, want


def test_lines_follow_an_update(api, tmp_path):
    """the keyed line kernel reads the NEW rows: an item signed with an updated entry's old secret is INVALID"""
    call, want = items_after_update()
    t, f = kc.table(api, 1), final(1)
    sets = {'lines': {'sg': 1, 'keys': t['blobs'], 'fmt': t['fmt'], 'tables': False, 'lines': True}}
    upd, info, got = run_worker(tmp_path, 'lines', LANE_SPLIT, sets, [
        {'op': 'update', 'set': 'lines', 'pos': f['pos'], 'keys': f['keys'], 'fmt': f['fmt']}, {'op': 'info', 'set': 'lines'},
        dict(call, op='verify', set='lines')])
    assert upd['launches'].get('k_keyset_lines_at') == 1 and not upd['launches'].get('k_keyset_lines'), upd['launches']
    assert info['has_lines'] is True
    print(got['launches'])
    assert got['st'] == want
    assert line_launches(got) == (1, 0)
    assert got['st'][OLD_SECRET] == INVALID


def test_rows_lost_and_regained(api, tmp_path):
    """RAW_AFFINE keys (trusted): an update to (x, 0) -- finite, no usable rows -- makes a lane-split call that names the entry walk the
    keys of all its items, with the statuses of the same call on a set without lines; the update back to the real key returns the
    call to the keyed kernel and the oracle's statuses"""
    call, want = items_after_update()
    f = final(1)
    y0 = next(ix for ix in call['idx'][15:] if ix not in POS + NEIGHBOURS + [kc.DUP_A])
    assert f['ks'][y0]
    aff = [bytes(192) if k in (0, None) else p[:192] for p, k in zip(f['points'], f['ks'])]
    broken = aff[y0][:96] + bytes(96)
    sets = {name: {'sg': 1, 'keys': aff, 'fmt': api.FMT_RAW_AFFINE, 'tables': False, 'lines': lines} for name, lines in (('lines', True), ('plain', False))}
    verify = lambda name: dict(call, op='verify', set=name)
    update = lambda name, key: {'op': 'update', 'set': name, 'pos': [y0], 'keys': [key], 'fmt': api.FMT_RAW_AFFINE}
    before, _, _, walked, plain, _, keyed, info = run_worker(tmp_path, 'rows', LANE_SPLIT, sets, [
        verify('lines'), update('lines', broken), update('plain', broken), verify('lines'), verify('plain'), update('lines', aff[y0]), verify('lines'),
        {'op': 'info', 'set': 'lines'}])
    want_raw = [PK_IDENTITY if i == AT_NEW_BAD else w for i, w in enumerate(want)]      # raw input is trusted: the blob is the zero record here
    assert before['st'] == want_raw and line_launches(before) == (1, 0)
    assert walked['st'] == plain['st'] and line_launches(walked) == (0, 1) and line_launches(plain) == (0, 1)
    named = [i for i, ix in enumerate(call['idx']) if ix == y0]
    assert all(walked['st'][i] != OK for i in named)
    assert [s for i, s in enumerate(walked['st']) if i not in named] == [s for i, s in enumerate(want_raw) if i not in named]
    assert keyed['st'] == want_raw and line_launches(keyed) == (1, 0)
    assert info['has_lines'] is True


# ------------------------------------------------------------------ 5. chunk border
BIG = 4100
BIG_SAMPLE = sorted({0, 1, 63, 64, 4095, 4096, 4099} | set(random.Random(5).sample(range(BIG), 57)))


def big_table(api, sg):
    t = kc.table(api, sg)
    src = list(itertools.islice(itertools.cycle(t['valid']), BIG))
    return [t['blobs'][i] for i in src], [t['ks'][i] for i in src]


def test_chunk_border_tables(api):
    """4,100 G1 keys with tables, every position updated in reversed order in one call: two chunks, the second of four keys"""
    assert len(BIG_SAMPLE) == 64
    blobs, secrets = big_table(api, 2)
    rev, rsec = blobs[::-1], secrets[::-1]
    rng = random.Random(55)
    sc = [rng.randrange(2 ** 256) for _ in BIG_SAMPLE]
    with api.KeySet.create(2, blobs, tables=True) as ks, api.KeySet.create(2, rev, tables=True) as fresh:
        st, launches = profiled(api, lambda: ks.update(list(range(BIG - 1, -1, -1)), blobs))
        assert st == [0] * BIG and launches.get('k_keyset_build_at') == 2 and not launches.get('k_keyset_build'), launches
        everything = list(range(BIG))
        assert ks.get(everything, api.FMT_COMPRESSED) == fresh.get(everything, api.FMT_COMPRESSED) == (rev, [0] * BIG)
        assert ks.info() == fresh.info() and ks.info()['has_tables']
        got = api.serialize(1, ks.mul(BIG_SAMPLE, sc))
        assert got == api.serialize(1, fresh.mul(BIG_SAMPLE, sc))
    assert got == api.serialize(1, kc.mb.key_points(api, 2, [rsec[p] * s % R for p, s in zip(BIG_SAMPLE, sc)]))


def test_chunk_border_lines(api, tmp_path):
    """4,100 G2 keys with lines, reversed in one call; a lane-split verify of 64 positions reads the rows of both chunks"""
    blobs, secrets = big_table(api, 1)
    rev, rsec = blobs[::-1], secrets[::-1]
    msgs = [b'big item %d' % i for i in range(64)]
    sigs = api.sign_batch(1, ref.POP, [rsec[p] for p in BIG_SAMPLE], msgs)[1]
    tampered = BIG_SAMPLE.index(4096) - 1
    sigs[tampered] = api.sign_batch(1, ref.POP, [secrets[BIG_SAMPLE[tampered]]], [msgs[tampered]])[1][0]     # the secret the position had BEFORE
    assert secrets[BIG_SAMPLE[tampered]] != rsec[BIG_SAMPLE[tampered]]
    want = [INVALID if i == tampered else OK for i in range(64)]
    sets = {'upd': {'sg': 1, 'keys': blobs, 'fmt': api.FMT_COMPRESSED, 'tables': False, 'lines': True},
            'fresh': {'sg': 1, 'keys': rev, 'fmt': api.FMT_COMPRESSED, 'tables': False, 'lines': True}}
    call = {'op': 'verify', 'scheme': ref.POP, 'idx': BIG_SAMPLE, 'sigs': sigs, 'msgs': msgs}
    everything = list(range(BIG))
    upd, a, b, ia, ib, va, vb = run_worker(tmp_path, 'big', LANE_SPLIT, sets, [
        {'op': 'update', 'set': 'upd', 'pos': everything[::-1], 'keys': blobs, 'fmt': api.FMT_COMPRESSED},
        {'op': 'get', 'set': 'upd', 'idx': everything}, {'op': 'get', 'set': 'fresh', 'idx': everything}, {'op': 'info', 'set': 'upd'},
        {'op': 'info', 'set': 'fresh'}, dict(call, set='upd'), dict(call, set='fresh')])
    assert upd['st'] == [0] * BIG and upd['launches'].get('k_keyset_lines_at') == 2 and not upd['launches'].get('k_keyset_lines'), upd['launches']
    assert a == b and a['keys'] == b''.join(rev).hex()
    assert ia == ib and ia['has_lines'] is True
    assert va['st'] == want and vb['st'] == want
    assert line_launches(va) == (1, 0) and line_launches(vb) == (1, 0)


# ------------------------------------------------------------------ 6. append
@functools.lru_cache(maxsize=None)
def tail(sg):
    """65 new keys (an identity inside, an undecodable one at the end: past a wave border of the tail) and their secrets"""
    api = get_api()
    g = 3 - sg
    rng = random.Random(3000 + sg)
    ks = [rng.randrange(2, R) for _ in range(65)]
    ks[3], ks[64] = 0, None
    blobs = api.serialize(g, kc.mb.key_points(api, sg, [k or 1 for k in ks]))
    blobs[3], blobs[64] = ident_blob(g), bad_blob(g)
    return blobs, ks


@pytest.mark.parametrize('tables,lines', FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize('sg', [1, 2])
def test_append_is_fresh_creation(api, sg, tables, lines):
    g = 3 - sg
    t = kc.table(api, sg)
    new, nks = tail(sg)
    new_status = api.deserialize(g, new)[1]
    assert new_status == [0] * 64 + [api.BAD_ENCODING]
    mk = lambda keys: api.KeySet.create(sg, keys, api.FMT_COMPRESSED, tables=tables, lines=lines)
    built = (tables, lines and sg == 1)
    msgs = [b'appended', b'past the end']
    sigs = kc.mb.signatures(api, sg, ref.BASIC, [nks[0], nks[0]], msgs)
    for count in (1, 65):
        with mk(t['blobs']) as ks, mk(t['blobs'] + new[:count]) as fresh:
            assert api.verify_indexed_batch(ks, ref.BASIC, [kc.N, kc.N + count], sigs, msgs) == [E_ARG, E_ARG]
            (first, st), launches = profiled(api, lambda: ks.append(new[:count]))
            assert first == kc.N and st == new_status[:count]
            info = same_set(api, ks, fresh, kc.N + count)
            assert (info['has_tables'], info['has_lines']) == built, info
            assert launches.get('k_keyset_seal_at') == 1 and launches.get('k_keyset_build_at', 0) == int(built[0]) and \
                launches.get('k_keyset_lines_at', 0) == int(built[1]) and not launches.get('k_keyset_build') and not launches.get('k_keyset_lines'), launches
            assert api.verify_indexed_batch(ks, ref.BASIC, [kc.N, kc.N + count], sigs, msgs) == [OK, E_ARG]
            if count == 65:                   # the old entries and the new ones, through the tables where the set has them
                idx = [kc.GEN, kc.N - 1, kc.N, kc.N + 3, kc.N + 63, kc.N + 64]
                assert api.serialize(g, ks.mul(idx, [7] * 6)) == api.serialize(g, fresh.mul(idx, [7] * 6))
    three = [new[0], new[3], new[64]]
    with mk([]) as ks, mk(three) as fresh:
        assert ks.info()['n'] == 0 and not ks.info()['has_tables'] and not ks.info()['has_lines']
        first, st = ks.append(three)
        assert first == 0 and st == [0, 0, api.BAD_ENCODING]
        info = same_set(api, ks, fresh, 3)
        assert (info['has_tables'], info['has_lines']) == built, info
        assert api.serialize(g, ks.mul([0, 1, 2], [5, 5, 5])) == api.serialize(g, kc.mb.key_points(api, sg, [5 * nks[0] % R])) + \
            api.serialize(g, [kc.mb.identity(g)]) * 2
        assert ks.append([]) == (3, []) and ks.info() == fresh.info()


def test_append_past_the_cap_drops_the_lines(api, tmp_path):
    """BLSGPU_KEYSET_TABLE_MB=5: 320 keys' rows (4.65 MiB) fit, 385 keys' rows (5.6 MiB) do not -- the lines are dropped, the set
    works without them, and no status changes"""
    call, want = items_after_update()
    f = final(1)
    new, _ = tail(1)
    sets = {'lines': {'sg': 1, 'keys': f['blobs'], 'fmt': f['fmt'], 'tables': False, 'lines': True},
            'fresh': {'sg': 1, 'keys': f['blobs'] + new, 'fmt': f['fmt'], 'tables': False, 'lines': True}}
    i0, v0, app, i1, v1, i2 = run_worker(tmp_path, 'cap', dict(LANE_SPLIT, BLSGPU_KEYSET_TABLE_MB='5'), sets, [
        {'op': 'info', 'set': 'lines'}, dict(call, op='verify', set='lines'), {'op': 'append', 'set': 'lines', 'keys': new, 'fmt': f['fmt']},
        {'op': 'info', 'set': 'lines'}, dict(call, op='verify', set='lines'), {'op': 'info', 'set': 'fresh'}])
    assert i0['has_lines'] is True and v0['st'] == want and line_launches(v0) == (1, 0)
    assert app['first'] == kc.N and app['st'] == [0] * 64 + [api.BAD_ENCODING]
    assert i1['has_lines'] is False and i1 == i2 and i1['n'] == kc.N + 65
    assert v1['st'] == want and line_launches(v1) == (0, 1)


# ------------------------------------------------------------------ 7. every indexed entry point after an update
def sets_naming_updates(f, rng):
    """index lists over the final table that name updated entries: every finite updated entry, the new identity, the new invalid
    entry, a list across a wave border, the empty list"""
    finite = [p for p in POS if f['ks'][p]]
    others = lambda n: [rng.choice(f['valid']) for _ in range(n)]
    return [finite, [65, 64, 63], [kc.GEN] + others(3) + [kc.GEN], finite + others(60), others(2) + [TO_IDENT], [kc.DUP_A, TO_BAD, 1], [kc.DUP_A, kc.DUP_B], []]


@pytest.mark.parametrize('scheme', [ref.BASIC, ref.POP], ids=['basic', 'pop'])
@pytest.mark.parametrize('sg', [1, 2])
def test_every_indexed_entry_point_after_an_update(api, sg, scheme):
    g = 3 - sg
    t, f = kc.table(api, sg), final(sg)
    rng = random.Random(70 + sg)
    idxs = sets_naming_updates(f, rng)
    secret = lambda idx: sum(f['ks'][i] or 0 for i in idx)
    with api.KeySet.create(sg, t['blobs'], t['fmt'], tables=True, lines=True) as ks, api.KeySet.create(sg, f['blobs'], f['fmt'], tables=True, lines=True) as fresh:
        ks.update(f['pos'], f['keys'])
        # by value an invalid entry has no key to hand over: those calls run on the sets that do not name it
        keyed = lambda sets: [s for s in sets if TO_BAD not in s[0]]
        by_value = lambda sets: [(fresh.get(idx)[0], a, b) for idx, a, b in keyed(sets)]
        kept = lambda sets, got: [r for s, r in zip(sets, got) if TO_BAD not in s[0]]
        # MultiSignature::verify: signed by the sum of the NEW secrets
        msgs = [b'updated multi %d' % s for s in range(len(idxs))]
        multi = list(zip(idxs, kc.mb.signatures(api, sg, scheme, [secret(idx) for idx in idxs], msgs), msgs))
        got = api.multi_verify_indexed_batch(ks, scheme, multi)
        assert got == api.multi_verify_indexed_batch(fresh, scheme, multi) and kept(multi, got) == api.multi_verify_batch(sg, scheme, by_value(multi))
        assert got[:4] == [OK] * 4 and got[5] == api.BAD_ENCODING and got[7] == SIG_IDENTITY, got
        old = (idxs[0], kc.mb.signatures(api, sg, scheme, [sum(t['ks'][i] or 0 for i in idxs[0])], msgs[:1])[0], msgs[0])
        assert api.multi_verify_indexed_batch(ks, scheme, [old]) == [INVALID]               # the OLD secrets no longer sign
        # the sums
        sums = api.serialize(g, api.sum_indexed_batch(ks, idxs))
        assert sums == api.serialize(g, api.sum_indexed_batch(fresh, idxs)) == api.serialize(g, api.sum_batch(g, [fresh.get(i)[0] for i in idxs]))
        assert sums[:4] == api.serialize(g, kc.mb.key_points(api, sg, [secret(idx) % R for idx in idxs[:4]]))
        # verify_secure over the Modern bytes, and the Legacy ones where they exist
        for legacy in ([False, True] if sg == 2 else [False]):
            secure = []
            for s, idx in enumerate(idxs):
                kb = api.serialize(g, [f['points'][i] for i in idx], legacy=legacy) if idx else []
                sk = aggregate_secret(kb, [f['ks'][i] or 0 for i in idx]) if idx and all(f['ks'][i] for i in idx) else 0
                secure.append((idx, kc.sb.sign(api, sg, scheme, sk, msgs[s]), msgs[s]))
            got = api.verify_secure_indexed_batch(ks, scheme, secure, ser_format=int(legacy))
            assert got == api.verify_secure_indexed_batch(fresh, scheme, secure, ser_format=int(legacy))
            assert kept(secure, got) == api.verify_secure_batch(sg, scheme, by_value(secure), ser_format=int(legacy))
            assert got[:4] == [OK] * 4 and got[5] == api.BAD_ENCODING, (legacy, got)
        # AggregateSignature::verify: one message per key, the signature the sum of the items'
        agg = []
        for s, idx in enumerate(idxs[:6]):
            ms = [b'updated agg %d %d' % (s, j) for j in range(len(idx))]
            parts = kc.mb.signatures(api, sg, scheme, [f['ks'][i] or 4242 for i in idx], ms)
            agg.append((idx, ms, api.point_sum(sg, parts)))
        got = api.aggregate_verify_indexed_batch(ks, scheme, agg)
        assert got == api.aggregate_verify_indexed_batch(fresh, scheme, agg) and kept(agg, got) == api.aggregate_verify_batch(sg, scheme, by_value(agg))
        assert [st for st, _ in got[:2]] == [OK, OK] and got[5][0] == api.BAD_ENCODING, got
        # shared-message verify: every item under its group's message
        groups = []
        for s, idx in enumerate(idxs[:6]):
            m = b'updated group %d' % s
            groups.append((m, idx, kc.mb.signatures(api, sg, scheme, [f['ks'][i] or 4242 for i in idx], [m] * len(idx))))
        got = api.verify_shared_indexed_batch(ks, scheme, groups)
        assert got == api.verify_shared_indexed_batch(fresh, scheme, groups)
        assert got[0] == [OK] * len(idxs[0]) and got[4][-1] == PK_IDENTITY and got[5] == [OK, api.BAD_ENCODING, OK], got
        usable = [gr for gr in groups if TO_BAD not in gr[1]]
        assert [st for gr, st in zip(groups, got) if TO_BAD not in gr[1]] == \
            api.verify_shared_batch(sg, scheme, [(m, fresh.get(idx)[0], sigs) for m, idx, sigs in usable])


# ------------------------------------------------------------------ 8. refusals
def test_refusals_write_nothing(api):
    lib = api.init()
    t = kc.table(api, 1)
    f = final(1)
    key = f['keys'][0]
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    u32 = lambda *v: p((ctypes.c_uint32 * len(v))(*v))
    two = api._ptr(key + key)
    SENTINEL = 0x5a5a5a5
    with api.KeySet.create(1, t['blobs'], t['fmt'], tables=True, lines=True) as ks, api.KeySet.create(2, kc.table(api, 2)['blobs']) as g1keys:
        dead = api.KeySet.create(1, t['blobs'][:4])
        stale = dead.handle
        dead.close()
        everything = list(range(kc.N))
        before = (ks.get(everything, api.FMT_COMPRESSED), ks.get(everything, api.FMT_RAW_AFFINE), ks.info())
        h, C = ks.handle, api.FMT_COMPRESSED
        first = ctypes.c_uint64(77)
        refused = [
            ('a duplicate position', lambda st: lib.blsgpu_keyset_update(h, u32(9, 9), two, 2, C, st)),
            ('a position equal to n', lambda st: lib.blsgpu_keyset_update(h, u32(4, kc.N), two, 2, C, st)),
            ('a stale handle', lambda st: lib.blsgpu_keyset_update(stale, u32(1, 2), two, 2, C, st)),
            ('the zero handle', lambda st: lib.blsgpu_keyset_update(0, u32(1, 2), two, 2, C, st)),
            ('null pos', lambda st: lib.blsgpu_keyset_update(h, None, two, 2, C, st)),
            ('null keys', lambda st: lib.blsgpu_keyset_update(h, u32(1, 2), None, 2, C, st)),
            ('LEGACY for sig_group 1', lambda st: lib.blsgpu_keyset_update(h, u32(1, 2), two, 2, api.FMT_LEGACY, st)),
            ('an unknown format', lambda st: lib.blsgpu_keyset_update(h, u32(1, 2), two, 2, 4, st)),
            ('a negative format', lambda st: lib.blsgpu_keyset_update(h, u32(1, 2), two, 2, -1, st)),
            ('append: a stale handle', lambda st: lib.blsgpu_keyset_append(stale, two, 2, C, st, ctypes.byref(first))),
            ('append: the zero handle', lambda st: lib.blsgpu_keyset_append(0, two, 2, C, st, ctypes.byref(first))),
            ('append: null keys', lambda st: lib.blsgpu_keyset_append(h, None, 2, C, st, ctypes.byref(first))),
            ('append: LEGACY for sig_group 1', lambda st: lib.blsgpu_keyset_append(h, two, 2, api.FMT_LEGACY, st, ctypes.byref(first))),
            ('append: an unknown format', lambda st: lib.blsgpu_keyset_append(h, two, 2, 4, st, ctypes.byref(first))),
        ]
        for name, call in refused:
            st = (ctypes.c_int32 * 2)(SENTINEL, SENTINEL)
            assert call(p(st)) == E_ARG, name
            assert list(st) == [SENTINEL, SENTINEL], name
            assert (ks.get(everything, api.FMT_COMPRESSED), ks.get(everything, api.FMT_RAW_AFFINE), ks.info()) == before, name
            assert first.value == 77, name
        st = (ctypes.c_int32 * 2)(SENTINEL, SENTINEL)
        assert lib.blsgpu_keyset_update(h, None, None, 0, C, p(st)) == 0 and lib.blsgpu_keyset_append(h, None, 0, C, p(st), ctypes.byref(first)) == 0
        assert list(st) == [SENTINEL, SENTINEL] and first.value == kc.N
        assert (ks.get(everything, api.FMT_COMPRESSED), ks.get(everything, api.FMT_RAW_AFFINE), ks.info()) == before
        with pytest.raises(api.BlsGpuRuntimeError, match='twice'):
            ks.update([3, 4, 3], [key] * 3)
        with pytest.raises(api.BlsGpuRuntimeError, match='outside'):
            ks.update([2 ** 32 - 1], [key])
        assert ks.statuses == t['status']
        # LEGACY is a format of sig_group 2 and accepted there
        tl = kc.table(api, 2, True)
        assert g1keys.update([1], [tl['blobs'][2]], api.FMT_LEGACY) == [0]
        assert g1keys.get([1], api.FMT_LEGACY)[0] == [tl['blobs'][2]]


# ------------------------------------------------------------------ 9. device-resident arguments
@pytest.mark.parametrize('sg', [1, 2])
def test_device_resident_arguments(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    t, f = kc.table(api, sg), final(sg)
    new, _ = tail(sg)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    with api.KeySet.create(sg, t['blobs'], t['fmt'], tables=True, lines=True) as ks, api.KeySet.create(sg, f['blobs'], f['fmt'], tables=True, lines=True) as fresh, \
            api.KeySet.create(sg, f['blobs'] + new, f['fmt'], tables=True, lines=True) as grown:
        pos = torch.tensor(f['pos'], dtype=torch.int32, device=dev)
        st = ops.keyset_update(ks, pos, tens(b''.join(f['keys'])), len(f['pos']), api.FMT_COMPRESSED)
        assert st.device == dev and st.dtype == torch.int32 and st.cpu().tolist() == [f['status'][p] for p in f['pos']]
        assert ks.statuses is None
        ks.statuses = fresh.statuses
        same_set(api, ks, fresh, kc.N)
        assert ks.get(list(range(kc.N)), api.FMT_RAW_AFFINE)[1] == f['status']
        first, st = ops.keyset_append(ks, tens(b''.join(new)), 65, api.FMT_COMPRESSED)
        assert first == kc.N and st.cpu().tolist() == [0] * 64 + [api.BAD_ENCODING]
        ks.statuses = grown.statuses
        same_set(api, ks, grown, kc.N + 65)
        # the pointer forms of KeySet itself: raw points from device memory, no statuses
        raw = tens(b''.join(f['points'][p] for p in (1, 2)))
        two = torch.tensor([2, 1], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ks.update_device(two.data_ptr(), raw.data_ptr(), 2, api.FMT_RAW_PROJ)
        assert ks.get([2, 1], api.FMT_COMPRESSED) == grown.get([1, 2], api.FMT_COMPRESSED)
        assert ks.append_device(raw.data_ptr(), 2, api.FMT_RAW_PROJ) == kc.N + 65
        assert ks.get([kc.N + 65, kc.N + 66], api.FMT_COMPRESSED) == grown.get([1, 2], api.FMT_COMPRESSED) and ks.info()['n'] == kc.N + 67
