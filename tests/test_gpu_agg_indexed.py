"""blsgpu_aggregate_verify_indexed_batch on the GPU: AggregateSignature::verify, many keys with one message each, over positions in
a registered key set -- and, for Bls12381G1Impl over a set with line tables (BLSGPU_KEYSET_LINES), the line kernel that reads every
row from a table (k_linesp_keyed) where k_linesp walked a G2 point per item.  The key table is keyset_cases.table (320 entries:
the identity, an undecodable blob, one key at two positions, the generator); signatures are sign_batch's under the entries'
secrets, summed per set.  Expected statuses AND aux words are the C oracle's bo_aggregate_verify on the gathered key points with
the precedence of the indexed calls on top (an index outside the table, then the first invalid entry), after a closed-form
assertion of what every crafted set must give; for the large batch the pattern it was tampered with, confirmed by the oracle on a
sample.  The profile's launch counts say which line kernel ran, so no test can pass by falling back.  Runs that need their own
process (the knobs are read once) go through tests/agg_indexed_worker.py: one attempt each, with its own time limit."""
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
OK, INVALID, SIG_IDENTITY, PK_IDENTITY, DUPLICATE = 0, 1, 2, 3, 4
SCHEMES = [(ref.POP, 'pop'), (ref.BASIC, 'basic'), (ref.AUG, 'aug')]
NO_AUX = (0, 0)


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


def run_worker(tmp_path, name, env, sets, calls, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'sets': sets, 'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'agg_indexed_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def results(call):
    """a worker call's (status, aux) pairs"""
    return [(s, tuple(a)) for s, a in zip(call['st'], call['aux'])]


def line_launches(launches):
    return launches.get('k_linesp_keyed', 0), launches.get('k_linesp', 0)


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


def identity_sig(sg):
    return kc.mb.identity(sg)


def signed_sets(api, sg, scheme, specs):
    """specs: [(pairs signed for: [(position, message)], sig: None = the sum of the pairs' signatures, else the bytes to send)] ->
    one aggregate signature per spec.  Position p signs with the entry's secret (nothing for the identity entry; some finite
    signature under another secret for an invalid entry or a position outside the table)."""
    t = kc.table(api, sg)
    flat = [(s, p, m) for s, (pairs, _) in enumerate(specs) for p, m in pairs]
    secrets = [(t['ks'][p] if p < kc.N and t['ks'][p] is not None else 4242) for _, p, _ in flat]
    sigs = kc.mb.signatures(api, sg, scheme, secrets, [m for _, _, m in flat])
    per_set = [[] for _ in specs]
    for (s, _, _), g in zip(flat, sigs):
        per_set[s].append(g)
    sums = api.sum_batch(sg, per_set)
    return [sums[s] if sig is None else sig for s, (_, sig) in enumerate(specs)]


# ------------------------------------------------------------------ the case list
NAMES = ['empty_identity', 'one', 'two', 'three', 'thirty_one', 'thirty_three', 'sixty_five', 'message_changed', 'key_swapped', 'pair_left_out',
         'duplicate_message', 'shares_message_a', 'shares_message_b', 'identity_signature', 'empty_real_signature', 'ident_twice', 'dup_a_and_b',
         'bad_after_ident', 'neighbour_before', 'past_end_dup_identity_sig', 'neighbour_after']
AT = {n: i for i, n in enumerate(NAMES)}


@functools.lru_cache(maxsize=None)
def case_sets(sg, scheme):
    """(sets as the call takes them: [(idx, msgs, sig)], closed-form (status, aux) per set)"""
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    t = kc.table(api, sg)
    rng = random.Random(500 + 10 * sg + scheme)
    plain = [i for i in t['valid'] if i not in (kc.GEN, kc.DUP_A, kc.DUP_B)]

    def draw(n):
        return [rng.choice(plain) for _ in range(n)]

    def msgs_of(s, n):
        return [b'aggregate %d/%d' % (s, j) for j in range(n)]

    rows = []                 # (idx as sent, msgs as sent, pairs signed for, sig override, closed form)

    def add(name, idx, msgs, want, signed=None, sig=None):
        assert AT[name] == len(rows)
        rows.append((idx, msgs, list(zip(idx, msgs)) if signed is None else signed, sig, want))

    dup_basic = (DUPLICATE, (0, 2)) if scheme == ref.BASIC else (OK, NO_AUX)
    add('empty_identity', [], [], (SIG_IDENTITY, NO_AUX), sig=identity_sig(sg))
    for name, n in (('one', 1), ('two', 2), ('three', 3), ('thirty_one', 31), ('thirty_three', 33), ('sixty_five', 65)):
        idx = draw(n)
        if n >= 2:
            idx[-1] = idx[0]                                  # repeated indices are repeated keys
        m = msgs_of(len(rows), n)
        if n == 2:
            m[1] = b''                                        # a zero-length message is a message like any other
        add(name, idx, m, (OK, NO_AUX))
    idx, m = draw(3), msgs_of(len(rows), 3)
    add('message_changed', idx, [m[0], b'another message', m[2]], (INVALID, NO_AUX), signed=list(zip(idx, m)))
    idx, m = draw(3), msgs_of(len(rows), 3)
    other = next(i for i in plain if i not in idx)
    add('key_swapped', idx[:2] + [other], m, (INVALID, NO_AUX), signed=list(zip(idx, m)))
    idx, m = draw(4), msgs_of(len(rows), 4)
    add('pair_left_out', idx[:3], m[:3], (INVALID, NO_AUX), signed=list(zip(idx, m)))
    idx, m = draw(3), msgs_of(len(rows), 3)
    add('duplicate_message', idx, [m[0], m[1], m[0]], dup_basic)
    shared = b'one message in two neighbouring sets'
    for name in ('shares_message_a', 'shares_message_b'):
        add(name, draw(2), [shared, b'and one of its own %d' % len(rows)], (OK, NO_AUX))
    add('identity_signature', draw(2), msgs_of(len(rows), 2), (SIG_IDENTITY, NO_AUX), sig=identity_sig(sg))
    add('empty_real_signature', [], [], (INVALID, NO_AUX), signed=[(plain[0], b'signed for nobody')])
    idx = draw(4)
    idx[1] = idx[3] = kc.IDENT
    add('ident_twice', idx, msgs_of(len(rows), 4), (PK_IDENTITY, (2, 0)))
    add('dup_a_and_b', [kc.DUP_A, draw(1)[0], kc.DUP_B], msgs_of(len(rows), 3), (OK, NO_AUX))
    add('bad_after_ident', [draw(1)[0], kc.IDENT, kc.BAD], msgs_of(len(rows), 3), (api.BAD_ENCODING, NO_AUX))
    add('neighbour_before', draw(2), msgs_of(len(rows), 2), (OK, NO_AUX))
    m = msgs_of(len(rows), 3)
    add('past_end_dup_identity_sig', [draw(1)[0], kc.N, draw(1)[0]], [m[0], m[1], m[0]], (E_ARG, NO_AUX), sig=identity_sig(sg))
    add('neighbour_after', draw(2), msgs_of(len(rows), 2), (OK, NO_AUX))
    assert len(rows) == len(NAMES)
    sigs = signed_sets(api, sg, scheme, [(r[2], r[3]) for r in rows])
    return [(r[0], r[1], g) for r, g in zip(rows, sigs)], [r[4] for r in rows]


def oracle_set(bo, t, sg, scheme, idx, msgs, sig):
    """(status, aux) of one set: the precedence of the indexed calls, then the C oracle on the gathered key points"""
    if any(i >= kc.N for i in idx):
        return E_ARG, NO_AUX
    bad = [t['status'][i] for i in idx if t['status'][i]]
    if bad:
        return bad[0], NO_AUX
    offs = (ctypes.c_uint64 * (len(msgs) + 1))()
    for j, m in enumerate(msgs):
        offs[j + 1] = offs[j] + len(m)
    aux = (ctypes.c_uint64 * 2)()
    V = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)  # noqa: E731
    st = bo.bo_aggregate_verify(sg, scheme, V(b''.join(t['points'][i] for i in idx)), V(b''.join(msgs)), ctypes.cast(offs, ctypes.c_void_p), len(msgs),
                                V(sig), 4, ctypes.cast(aux, ctypes.c_void_p))
    return st, (aux[0], aux[1])


@functools.lru_cache(maxsize=None)
def case_reference(sg, scheme):
    """the case list and the ORACLE's (status, aux) of every set, which must be the closed form (computed once, shared by the tests)"""
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    sets, closed = case_sets(sg, scheme)
    bo = util.load_c_oracle()
    t = kc.table(api, sg)
    want = [oracle_set(bo, t, sg, scheme, *s) for s in sets]
    for name, w, cf in zip(NAMES, want, closed):
        assert w == cf, (name, w, cf)
    return sets, want


def names_no_bad_position(t, idx):
    return all(i < kc.N and t['status'][i] == 0 for i in idx)


# ------------------------------------------------------------------ 1. the case list, both impls, every scheme
@pytest.mark.parametrize('scheme,_id', SCHEMES, ids=[s[1] for s in SCHEMES])
@pytest.mark.parametrize('sg', [1, 2])
def test_case_list(api, sg, scheme, _id):
    """one call of 21 sets over a set created with lines (Bls12381G1Impl: the keyed kernel; Bls12381G2Impl: no lines exist)"""
    sets, want = case_reference(sg, scheme)
    t = kc.table(api, sg)
    with api.KeySet.create(sg, t['blobs'], t['fmt'], lines=True) as ks:
        assert ks.info()['has_lines'] is (sg == 1)
        got, launches = profiled(api, lambda: api.aggregate_verify_indexed_batch(ks, scheme, sets))
        clean = [s for s in range(len(sets)) if names_no_bad_position(t, sets[s][0])]
        by_value = api.aggregate_verify_batch(sg, scheme, [(ks.get(sets[s][0])[0], sets[s][1], sets[s][2]) for s in clean])
    print(got, launches)
    assert got == want, [(NAMES[s], got[s], want[s]) for s in range(len(sets)) if got[s] != want[s]]
    assert [got[s] for s in clean] == by_value and len(clean) == len(sets) - 2
    assert line_launches(launches) == ((1, 0) if sg == 1 else (0, 1))


# ------------------------------------------------------------------ 2. which line kernel ran
def table_sets(t, sg=1, **which):
    return {name: {'sg': sg, 'keys': t['blobs'], 'fmt': t['fmt'], 'tables': False, 'lines': lines} for name, lines in which.items()}


def test_which_line_kernel_runs(api, tmp_path):
    """Bls12381G1Impl: over the set with lines k_linesp_keyed and no k_linesp; over the set without, and over the one whose lines were
    refused (BLSGPU_KEYSET_TABLE_MB=1: 4.6 MiB of rows), the reverse; Bls12381G2Impl created with lines=True: k_linesp only.  The
    oracle's statuses and aux in every one of them."""
    sets, want = case_reference(1, ref.POP)
    t = kc.table(api, 1)
    got = run_worker(tmp_path, 'kernels', {}, table_sets(t, lines=True, plain=False),
                     [{'set': 'lines', 'scheme': ref.POP, 'sets': sets}, {'set': 'plain', 'scheme': ref.POP, 'sets': sets}])
    assert got['sets']['lines']['has_lines'] is True and got['sets']['plain']['has_lines'] is False
    keyed, plain = got['calls']
    print(keyed['launches'], plain['launches'])
    assert results(keyed) == want and results(plain) == want
    assert line_launches(keyed['launches']) == (1, 0)
    assert line_launches(plain['launches']) == (0, 1)
    refused = run_worker(tmp_path, 'refused', {'BLSGPU_KEYSET_TABLE_MB': '1'}, table_sets(t, lines=True), [{'set': 'lines', 'scheme': ref.POP, 'sets': sets}])
    assert refused['sets']['lines']['has_lines'] is False
    assert results(refused['calls'][0]) == want
    assert line_launches(refused['calls'][0]['launches']) == (0, 1)
    sets2, want2 = case_reference(2, ref.POP)
    t2 = kc.table(api, 2)
    with api.KeySet.create(2, t2['blobs'], t2['fmt'], lines=True) as ks:
        got2, launches = profiled(api, lambda: api.aggregate_verify_indexed_batch(ks, ref.POP, sets2))
    assert got2 == want2 and line_launches(launches) == (0, 1)


# ------------------------------------------------------------------ 3. an entry without usable rows
def test_fallback_when_a_named_entry_has_no_rows(api, tmp_path):
    """RAW_AFFINE keys (trusted), one entry (x of a real key, 0): finite, and its first tangent is vertical, so it has no rows.  A
    call that names it walks ALL its items (k_linesp) and equals the same call on a set without lines; a call that does not name it
    takes the keyed kernel"""
    sets, want = case_reference(1, ref.POP)
    t = kc.table(api, 1)
    named = {i for s in sets for i in s[0]}
    Y0 = next(i for i in t['valid'] if i not in named and i not in (kc.GEN, kc.DUP_A, kc.DUP_B))
    aff = [bytes(192) if k in (0, None) else p[:192] for p, k in zip(t['points'], t['ks'])]
    aff[Y0] = aff[Y0][:96] + bytes(96)
    ksets = {name: {'sg': 1, 'keys': aff, 'fmt': api.FMT_RAW_AFFINE, 'tables': False, 'lines': lines} for name, lines in (('lines', True), ('plain', False))}
    naming = [(list(idx), msgs, sig) for idx, msgs, sig in sets]
    naming[AT['thirty_one']][0][5] = naming[AT['sixty_five']][0][50] = Y0
    got = run_worker(tmp_path, 'fallback', {}, ksets, [{'set': 'lines', 'scheme': ref.POP, 'sets': naming}, {'set': 'plain', 'scheme': ref.POP, 'sets': naming},
                                                       {'set': 'lines', 'scheme': ref.POP, 'sets': sets}])
    assert got['sets']['lines']['has_lines'] is True
    walked, plain, keyed = got['calls']
    # raw input is trusted: the undecodable blob of the wire table is the zero record here, an identity entry after the one before it
    want_raw = [(PK_IDENTITY, (2, 0)) if s == AT['bad_after_ident'] else w for s, w in enumerate(want)]
    touched = (AT['thirty_one'], AT['sixty_five'])
    assert results(walked) == results(plain)
    assert [r for s, r in enumerate(results(walked)) if s not in touched] == [w for s, w in enumerate(want_raw) if s not in touched]
    assert all(walked['st'][s] != OK for s in touched)
    assert line_launches(walked['launches']) == (0, 1) and line_launches(plain['launches']) == (0, 1)
    assert results(keyed) == want_raw
    assert line_launches(keyed['launches']) == (1, 0)


# ------------------------------------------------------------------ 4. the large-set plan
def test_large_set_plan(api, bo, tmp_path):
    """BLSGPU_AGG_BATCH_MAX=8: the sets of 8 and 20 pairs run one at a time on the gathered keys, those of 3 and 2 through the keyed
    kernel; the 8 names the undecodable entry, the 20 has a message changed.  The oracle's statuses and aux, as with the default knob"""
    t = kc.table(api, 1)
    rng = random.Random(44)
    plain = [i for i in t['valid'] if i not in (kc.GEN, kc.DUP_A, kc.DUP_B)]
    rows = []
    for s, n in enumerate((3, 8, 20, 2)):
        idx = [rng.choice(plain) for _ in range(n)]
        msgs = [b'large plan %d/%d' % (s, j) for j in range(n)]
        rows.append((idx, msgs))
    rows[1][0][4] = kc.BAD
    specs = [(list(zip(idx, msgs)), None) for idx, msgs in rows]
    sigs = signed_sets(api, 1, ref.BASIC, specs)
    rows[2][1][7] = b'another message'
    sets = [(idx, msgs, g) for (idx, msgs), g in zip(rows, sigs)]
    want = [oracle_set(bo, t, 1, ref.BASIC, *s) for s in sets]
    assert want == [(OK, NO_AUX), (api.BAD_ENCODING, NO_AUX), (INVALID, NO_AUX), (OK, NO_AUX)]
    got = run_worker(tmp_path, 'large', {'BLSGPU_AGG_BATCH_MAX': '8'}, table_sets(t, lines=True), [{'set': 'lines', 'scheme': ref.BASIC, 'sets': sets}])['calls'][0]
    print(got['launches'])
    assert results(got) == want
    assert line_launches(got['launches'])[0] == 1                      # the batched sets, one round (the large sets take the single call's kernels)
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        assert api.aggregate_verify_indexed_batch(ks, ref.BASIC, sets) == want


# ------------------------------------------------------------------ 5. two rounds of the line kernel
N_SETS, PER_SET = 1040, 63


def tamper_kind(s):
    """about one set in eight: 1 = the next set's signature, 2 = the identity signature, 3 = the identity entry at one position, 4 =
    the undecodable entry, 5 = a position outside the table"""
    return {3: 1, 13: 2, 23: 3, 33: 4, 37: 5}.get(s % 40, 0)


def test_two_rounds(api, bo):
    """1,040 sets of 63 pairs, Basic with distinct messages: 66,560 flat items, just past one round of 65,536, so the second of two
    rounds of 33,280 starts at a non-zero `first` (inside set 528).  Statuses and aux equal the tamper pattern, which the oracle
    confirms on the first set of every kind, the last set and the sets around the round border; the keyed kernel ran twice and
    k_linesp not at all"""
    t = kc.table(api, 1)
    rng = random.Random(1040)
    plain = [i for i in t['valid'] if i not in (kc.GEN, kc.DUP_A, kc.DUP_B)]
    idx = [[rng.choice(plain) for _ in range(PER_SET)] for _ in range(N_SETS)]
    msgs = [[b'two rounds %d/%d' % (s, j) for j in range(PER_SET)] for s in range(N_SETS)]
    flat_sigs = api.sign_batch(1, ref.BASIC, [t['ks'][i] for ix in idx for i in ix], [m for ms in msgs for m in ms])[1]
    orig = api.sum_batch(1, [flat_sigs[PER_SET * s:PER_SET * (s + 1)] for s in range(N_SETS)])
    sigs, expect = list(orig), []
    for s in range(N_SETS):
        k, pos = tamper_kind(s), s % PER_SET
        if k == 1:
            sigs[s] = orig[(s + 1) % N_SETS]
        elif k == 2:
            sigs[s] = identity_sig(1)
        elif k >= 3:
            idx[s][pos] = {3: kc.IDENT, 4: kc.BAD, 5: kc.N + s}[k]
        expect.append({0: (OK, NO_AUX), 1: (INVALID, NO_AUX), 2: (SIG_IDENTITY, NO_AUX), 3: (PK_IDENTITY, (pos + 1, 0)), 4: (api.BAD_ENCODING, NO_AUX),
                       5: (E_ARG, NO_AUX)}[k])
    sets = [(idx[s], msgs[s], sigs[s]) for s in range(N_SETS)]
    border = 33280 // PER_SET                                  # set 528 owns flat items 33,264 .. 33,326
    assert PER_SET * border < 33280 < PER_SET * (border + 1)
    for s in (3, 13, 23, 33, 37, N_SETS - 1, border - 1, border, border + 1):
        assert oracle_set(bo, t, 1, ref.BASIC, *sets[s]) == expect[s], s
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        assert ks.info()['has_lines'] is True
        got, launches = profiled(api, lambda: api.aggregate_verify_indexed_batch(ks, ref.BASIC, sets))
    bad = [(s, got[s], expect[s]) for s in range(N_SETS) if got[s] != expect[s]][:10]
    assert not bad and len(got) == N_SETS, bad
    assert line_launches(launches) == (2, 0), launches


# ------------------------------------------------------------------ 6. device pointers
def test_device_pointers(api):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sets, want = case_reference(1, ref.BASIC)
    t = kc.table(api, 1)
    u8 = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)  # noqa: E731
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)  # noqa: E731
    soffs = [0]
    for ix, _, _ in sets:
        soffs.append(soffs[-1] + len(ix))
    moffs, mblob = api._offsets([m for _, ms, _ in sets for m in ms])
    idx = torch.tensor([i for ix, _, _ in sets for i in ix], dtype=torch.int32, device=dev)
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        st, aux = ops.aggregate_verify_indexed_batch(ks, ref.BASIC, idx, u8(mblob), i64(moffs), i64(soffs), len(sets), u8(b''.join(g for _, _, g in sets)))
        assert st.device == dev and st.dtype == torch.int32 and aux.device == dev and tuple(aux.shape) == (len(sets), 2)
        host = api.aggregate_verify_indexed_batch(ks, ref.BASIC, sets)
    got = [(s, (a[0], a[1])) for s, a in zip(st.cpu().tolist(), aux.cpu().tolist())]
    assert got == host == want


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors(api):
    sets, _ = case_reference(1, ref.POP)
    sets = sets[1:4]
    t = kc.table(api, 1)
    lib = api.init()
    n_sets = len(sets)
    soffs = (ctypes.c_uint64 * (n_sets + 1))()
    for s, (ix, _, _) in enumerate(sets):
        soffs[s + 1] = soffs[s] + len(ix)
    idx = (ctypes.c_uint32 * soffs[n_sets])(*[i for ix, _, _ in sets for i in ix])
    moffs, mblob = api._offsets([m for _, ms, _ in sets for m in ms])
    sgb = b''.join(g for _, _, g in sets)
    V = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def call(handle, idx_p, soffs_p, n):
        st = (ctypes.c_int32 * n_sets)(*[77] * n_sets)
        aux = (ctypes.c_uint64 * (2 * n_sets))(*[99] * (2 * n_sets))
        rc = lib.blsgpu_aggregate_verify_indexed_batch(ref.POP, handle, idx_p, api._ptr(mblob), V(moffs), soffs_p, n, api._ptr(sgb), api.FMT_RAW_PROJ, V(st),
                                                       V(aux))
        return rc, list(st), list(aux)

    untouched = ([77] * n_sets, [99] * (2 * n_sets))
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        handle = ks.handle
        rc, st, aux = call(handle, V(idx), V(soffs), n_sets)
        assert rc == 0 and st == [OK] * n_sets and aux == [0] * (2 * n_sets)
        down = (ctypes.c_uint64 * (n_sets + 1))(*[soffs[0], soffs[2], soffs[1], soffs[3]])
        assert call(handle, V(idx), V(down), n_sets) == (E_ARG,) + untouched           # offsets that decrease
        assert call(handle, None, V(soffs), n_sets) == (E_ARG,) + untouched            # null idx with T > 0
        assert call(handle, V(idx), None, n_sets) == (E_ARG,) + untouched              # null set_offsets
        assert call(handle, V(idx), V(soffs), 0) == (0,) + untouched                   # no sets: nothing to do
    assert call(handle, V(idx), V(soffs), n_sets) == (E_ARG,) + untouched              # a stale handle
    with pytest.raises(ValueError):
        with api.KeySet.create(1, t['blobs'], t['fmt']) as ks:
            api.aggregate_verify_indexed_batch(ks, ref.POP, [([1, 2], [b'one message'], sgb[:144])])
