"""blsgpu_aggregate_verify_msgset_batch / _indexed_batch on the GPU: AggregateSignature::verify with pair i's message named as an
entry of a registered message set, the keys of one (set, message) class summed and paired once.  The key table has 64 entries (the
identity, an undecodable blob, a key k and its negative r - k); the message set 40 messages, two positions of equal bytes and the
empty message.  Expected statuses AND aux words are the C oracle's bo_aggregate_verify on the key points and the entries' message
BYTES, with the message-index rule and the key set's two rules on top, after a closed-form assertion of what every crafted set must
give; agreement with the by-value call is an extra check.  The profile's launch counts say which plan and which line kernel ran.  A
run that needs its own environment goes through tests/agg_msgset_worker.py: one attempt, with its own time limit."""
import ctypes
import functools
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

import multi_batch_cases as mb
import util
from util import ref

pytestmark = pytest.mark.gpu

E_ARG = -3
OK, INVALID, SIG_IDENTITY, PK_IDENTITY, DUPLICATE = 0, 1, 2, 3, 4
NO_AUX = (0, 0)
R = mb.R
COMBOS = [(sg, scheme) for sg in (1, 2) for scheme in (ref.BASIC, ref.POP)]
COMBO_IDS = ['g%d-%s' % (sg, 'basic' if scheme == ref.BASIC else 'pop') for sg, scheme in COMBOS]

N = 64                                         # key table
IDENT, BAD, POS, NEG = 5, 11, 20, 41
N_MSGS, EQ_A, EQ_B, EMPTY = 40, 3, 17, 9       # message set
MSGS = [b'aggregate by index: entry %d' % i for i in range(N_MSGS)]
MSGS[EQ_B] = MSGS[EQ_A]
MSGS[EMPTY] = b''
DISTINCT = [i for i in range(N_MSGS) if i != EQ_B]          # positions of pairwise different bytes
OUTSIDE = b'signed under an index outside the set'
FAR = 1 << 20                                  # outside every message set of this file


def get_api():
    from __graft_entry__ import import_pkg
    return import_pkg().api


def message_of(m):
    return MSGS[m] if m < N_MSGS else OUTSIDE


@functools.lru_cache(maxsize=None)
def table(sg):
    """dict(ks, blobs, fmt, status, points): ks[i] entry i's secret (0: the identity, None: the undecodable entry)"""
    api = get_api()
    rng = random.Random(7000 + sg)
    ks = [rng.randrange(1, R) for _ in range(N)]
    ks[NEG] = R - ks[POS]
    blobs = api.serialize(3 - sg, mb.key_points(api, sg, ks))
    w = len(blobs[0])
    ks[IDENT] = 0
    blobs[IDENT] = b'\xc0' + bytes(w - 1)
    ks[BAD] = None
    blobs[BAD] = bytes([blobs[BAD][0] & 0x9f | 0x1f]) + b'\xff' * (w - 1)      # x >= p
    pts, status = api.deserialize(3 - sg, blobs)
    assert [i for i, s in enumerate(status) if s] == [BAD] and status[BAD] == api.BAD_ENCODING
    return dict(ks=ks, blobs=blobs, fmt=api.FMT_COMPRESSED, status=status, points=pts,
                plain=[i for i in range(N) if i not in (IDENT, BAD, POS, NEG)])


def signed_sets(sg, scheme, specs):
    """specs: [(pairs signed for: [(key position, message position)], sig: None = the sum of the pairs' signatures, else the bytes
    to send)] -> one aggregate signature per spec.  The signature of a set is the sum over its (message) classes of (sum of the
    class's secrets) H(m): one sign_batch item per class."""
    api, t = get_api(), table(sg)
    flat = []
    for s, (pairs, _) in enumerate(specs):
        by_msg = {}
        for p, m in pairs:
            k = t['ks'][p] if p < N and t['ks'][p] is not None else 4242
            by_msg[message_of(m)] = (by_msg.get(message_of(m), 0) + k) % R
        flat += [(s, k, m) for m, k in sorted(by_msg.items())]
    sigs = mb.signatures(api, sg, scheme, [k for _, k, _ in flat], [m for _, _, m in flat])
    per_set = [[] for _ in specs]
    for (s, _, _), g in zip(flat, sigs):
        per_set[s].append(g)
    sums = api.sum_batch(sg, per_set)
    return [sums[s] if sig is None else sig for s, (_, sig) in enumerate(specs)]


def first_duplicate(midx):
    """Basic's rule on the entries' message bytes: (earlier, i) of the first i whose message was seen before, or None"""
    seen = {}
    for i, m in enumerate(midx):
        if MSGS[m] in seen:
            return seen[MSGS[m]], i
        seen[MSGS[m]] = i
    return None


def oracle_set(bo, sg, scheme, idx, midx, sig):
    """(status, aux) of one set: the message-index rule, the key set's two rules, then the C oracle on the key points and the
    entries' message bytes (tests/test_gpu_agg_indexed.py::oracle_set with the message rule on top)"""
    t = table(sg)
    if any(m >= N_MSGS for m in midx):
        return E_ARG, NO_AUX
    if any(i >= N for i in idx):
        return E_ARG, NO_AUX
    bad = [t['status'][i] for i in idx if t['status'][i]]
    if bad:
        return bad[0], NO_AUX
    msgs = [MSGS[m] for m in midx]
    offs = (ctypes.c_uint64 * (len(msgs) + 1))()
    for j, m in enumerate(msgs):
        offs[j + 1] = offs[j] + len(m)
    aux = (ctypes.c_uint64 * 2)()
    V = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)  # noqa: E731
    st = bo.bo_aggregate_verify(sg, scheme, V(b''.join(t['points'][i] for i in idx)), V(b''.join(msgs)), ctypes.cast(offs, ctypes.c_void_p), len(msgs),
                                V(sig), 4, ctypes.cast(aux, ctypes.c_void_p))
    return st, (aux[0], aux[1])


def by_value_able(idx):
    """can the set be sent with its keys by value?  (the undecodable entry and a position outside the table have no key)"""
    return all(i < N and i != BAD for i in idx)


def by_value(sg, sets):
    t = table(sg)
    return [([t['points'][i] for i in idx], midx, sig) for idx, midx, sig in sets]


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


def line_launches(launches):
    return launches.get('k_linesp_keyed', 0), launches.get('k_linesp', 0)


def summed(launches):
    return launches.get('k_agg_msgset_sum', 0)


# ------------------------------------------------------------------ the case list
NAMES = ['empty_identity', 'one', 'two', 'three', 'thirty_one', 'thirty_three', 'sixty_five_one_entry', 'interleaved', 'classes_3_4_5_9', 'same_key_twice',
         'neg_beside_a_class', 'neg_alone_real_signature', 'identity_in_class', 'identity_key_own_class', 'neighbour_a', 'neighbour_b', 'message_changed',
         'key_swapped', 'pair_left_out', 'identity_signature', 'empty_real_signature', 'bad_message_dup_identity_sig', 'bad_message_then_bad_key',
         'undecodable_key', 'key_outside', 'equal_bytes_positions', 'same_position_twice']
AT = {n: i for i, n in enumerate(NAMES)}
SINGLETONS = ['empty_identity', 'one', 'two', 'three', 'thirty_one', 'thirty_three', 'neighbour_a', 'neighbour_b', 'message_changed', 'identity_key_own_class']


@functools.lru_cache(maxsize=None)
def case_sets(sg, scheme):
    """(sets as the indexed call takes them: [(idx, msg_idx, sig)], closed-form (status, aux) per set)"""
    t = table(sg)
    rng = random.Random(900 + 10 * sg + scheme)
    basic = scheme == ref.BASIC

    def draw(n):
        return [rng.choice(t['plain']) for _ in range(n)]

    def distinct(n):
        return rng.sample([m for m in DISTINCT if m != EMPTY], n)

    def dup_or(midx, other=(OK, NO_AUX)):
        d = first_duplicate(midx)
        return (DUPLICATE, d) if basic and d else other

    rows = []                 # (idx, msg_idx, pairs signed for, sig override, closed form)

    def add(name, idx, midx, want, signed=None, sig=None):
        assert AT[name] == len(rows) and len(idx) == len(midx)
        rows.append((idx, midx, list(zip(idx, midx)) if signed is None else signed, sig, want))

    ident = mb.identity(sg)
    add('empty_identity', [], [], (SIG_IDENTITY, NO_AUX), sig=ident)
    add('one', draw(1), distinct(1), (OK, NO_AUX))
    add('two', draw(2), [distinct(1)[0], EMPTY], (OK, NO_AUX))                 # a zero-length message is a message like any other
    add('three', draw(3), distinct(3), (OK, NO_AUX))
    add('thirty_one', draw(31), distinct(31), (OK, NO_AUX))
    add('thirty_three', draw(33), distinct(33), (OK, NO_AUX))
    add('sixty_five_one_entry', draw(65), [4] * 65, dup_or([4] * 65))         # one class of 65 keys: past one wave
    assert dup_or([4] * 65) == ((DUPLICATE, (0, 1)) if basic else (OK, NO_AUX))
    a, b = distinct(2)
    add('interleaved', draw(4), [a, b, a, b], (DUPLICATE, (0, 2)) if basic else (OK, NO_AUX))
    e = distinct(4)
    midx = [e[0]] * 3 + [e[1]] * 4 + [e[2]] * 5 + [e[3]] * 9                   # classes around the 4-key strip
    rng.shuffle(midx)
    add('classes_3_4_5_9', draw(21), midx, dup_or(midx))
    k = draw(2)
    a, b = distinct(2)
    add('same_key_twice', [k[0], k[0], k[1]], [a, a, b], (DUPLICATE, (0, 1)) if basic else (OK, NO_AUX))      # a doubling inside the class sum
    a, b = distinct(2)
    add('neg_beside_a_class', [POS, NEG, draw(1)[0]], [a, a, b], (DUPLICATE, (0, 1)) if basic else (OK, NO_AUX))   # k + (r - k): the factor 1
    a, b = distinct(2)
    add('neg_alone_real_signature', [POS, NEG], [a, a], (DUPLICATE, (0, 1)) if basic else (INVALID, NO_AUX), signed=[(draw(1)[0], b)])
    a = distinct(1)[0]
    k = draw(2)
    add('identity_in_class', [k[0], IDENT, k[1]], [a, a, a], (DUPLICATE, (0, 1)) if basic else (PK_IDENTITY, (2, 0)))   # the class sum is finite
    add('identity_key_own_class', [draw(1)[0], IDENT], distinct(2), (PK_IDENTITY, (2, 0)))
    shared = distinct(2)
    for name in ('neighbour_a', 'neighbour_b'):                                # nothing merges across a set border
        add(name, draw(2), list(shared), (OK, NO_AUX))
    idx, m = draw(3), distinct(4)
    add('message_changed', idx, [m[0], m[3], m[2]], (INVALID, NO_AUX), signed=list(zip(idx, m[:3])))
    idx, m = draw(3), distinct(3)
    other = next(i for i in t['plain'] if i not in idx)
    add('key_swapped', idx[:2] + [other], m, (INVALID, NO_AUX), signed=list(zip(idx, m)))
    idx, m = draw(4), distinct(4)
    add('pair_left_out', idx[:3], m[:3], (INVALID, NO_AUX), signed=list(zip(idx, m)))
    add('identity_signature', draw(2), distinct(2), (SIG_IDENTITY, NO_AUX), sig=ident)
    add('empty_real_signature', [], [], (INVALID, NO_AUX), signed=[(t['plain'][0], 0)])
    a = distinct(1)[0]
    add('bad_message_dup_identity_sig', draw(3), [a, FAR, a], (E_ARG, NO_AUX), sig=ident)
    add('bad_message_then_bad_key', [draw(1)[0], N + 5], [2 ** 32 - 1, distinct(1)[0]], (E_ARG, NO_AUX))
    add('undecodable_key', [draw(1)[0], BAD], distinct(2), (get_api().BAD_ENCODING, NO_AUX))
    add('key_outside', [draw(1)[0], N], distinct(2), (E_ARG, NO_AUX))
    add('equal_bytes_positions', draw(2), [EQ_A, EQ_B], (DUPLICATE, (0, 1)) if basic else (OK, NO_AUX))
    add('same_position_twice', draw(2), [EQ_A, EQ_A], (DUPLICATE, (0, 1)) if basic else (OK, NO_AUX))
    assert len(rows) == len(NAMES)
    sigs = signed_sets(sg, scheme, [(r[2], r[3]) for r in rows])
    return [(r[0], r[1], g) for r, g in zip(rows, sigs)], [r[4] for r in rows]


@functools.lru_cache(maxsize=None)
def case_reference(sg, scheme):
    """the case list and the ORACLE's (status, aux) of every set, which must be the closed form (computed once, shared by the tests)"""
    sets, closed = case_sets(sg, scheme)
    bo = util.load_c_oracle()
    want = [oracle_set(bo, sg, scheme, *s) for s in sets]
    for name, w, cf in zip(NAMES, want, closed):
        assert w == cf, (name, w, cf)
    return sets, want


# ------------------------------------------------------------------ 1. the case list: both impls, Basic and PoP, by value and by index
@pytest.mark.parametrize('sg,scheme', COMBOS, ids=COMBO_IDS)
def test_case_list(api, sg, scheme):
    sets, want = case_reference(sg, scheme)
    t = table(sg)
    clean = [s for s in range(len(sets)) if by_value_able(sets[s][0])]
    assert len(clean) == len(sets) - 3
    single = [AT[n] for n in SINGLETONS]
    with api.MessageSet.create(sg, scheme, MSGS) as ms, api.KeySet.create(sg, t['blobs'], t['fmt']) as ks:
        got, launches = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(ms, ks, sets))
        got_v, launches_v = profiled(api, lambda: api.aggregate_verify_msgset_batch(ms, by_value(sg, [sets[s] for s in clean])))
        got_1, launches_1 = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(ms, ks, [sets[s] for s in single]))
        got_1v, launches_1v = profiled(api, lambda: api.aggregate_verify_msgset_batch(ms, by_value(sg, [sets[s] for s in single])))
    hashed = api.aggregate_verify_batch(sg, scheme, [([t['points'][i] for i in sets[s][0]], [message_of(m) for m in sets[s][1]], sets[s][2])
                                                     for s in clean if all(m < N_MSGS for m in sets[s][1])])
    print(got, launches, launches_v, launches_1, launches_1v)
    assert got == want, [(NAMES[s], got[s], want[s]) for s in range(len(sets)) if got[s] != want[s]]
    assert got_v == [want[s] for s in clean], [(NAMES[s], g, want[s]) for s, g in zip(clean, got_v) if g != want[s]]
    assert got_1 == [want[s] for s in single] and got_1v == got_1
    assert hashed == [want[s] for s in clean if all(m < N_MSGS for m in sets[s][1])]          # the extra check: the by-value call agrees
    # which plan ran: classes of two or more keys sum them; a call whose classes are all singletons does not launch the sum
    assert summed(launches) == 1 and summed(launches_v) == 1
    assert summed(launches_1) == 0 and summed(launches_1v) == 0
    assert launches.get('k_prepare_agg', 0) == 0 and launches.get('k_hash_to_point', 0) == 0     # nothing is hashed


# ------------------------------------------------------------------ 2. which line kernel ran
def run_worker(tmp_path, name, env, spec, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump(spec, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'agg_msgset_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def results(call):
    return [(s, tuple(a)) for s, a in zip(call['st'], call['aux'])]


def test_which_line_kernel_runs(api, tmp_path):
    """Bls12381G2Impl: over a set with rows the class items take the keyed kernel and k_linesp runs for the signature items alone;
    over a set without rows, and over one whose rows were refused (BLSGPU_KEYSET_TABLE_MB=1: 80 entries are 1.16 MiB of rows),
    k_linesp alone.  Bls12381G1Impl created with lines=True has no rows.  The oracle's statuses and aux in every one of them."""
    sets, want = case_reference(2, ref.POP)
    t = table(2)
    with api.MessageSet.create(2, ref.POP, MSGS, lines=True) as rows, api.MessageSet.create(2, ref.POP, MSGS) as plain, \
            api.KeySet.create(2, t['blobs'], t['fmt']) as ks:
        assert rows.info()['has_lines'] is True and plain.info()['has_lines'] is False
        got_r, launches_r = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(rows, ks, sets))
        got_p, launches_p = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(plain, ks, sets))
    print(launches_r, launches_p)
    assert got_r == want and got_p == want
    assert line_launches(launches_r) == (1, 1)
    assert line_launches(launches_p) == (0, 1)
    padded = MSGS + [b'an entry nobody names %d' % i for i in range(40)]
    clean = [s for s in sets if by_value_able(s[0])]
    refused = run_worker(tmp_path, 'refused', {'BLSGPU_KEYSET_TABLE_MB': '1'},
                         {'msgsets': {'m': {'sg': 2, 'scheme': ref.POP, 'msgs': padded, 'lines': True}},
                          'keysets': {'k': {'sg': 2, 'keys': t['blobs'], 'fmt': t['fmt']}},
                          'calls': [{'msgset': 'm', 'keyset': 'k', 'sets': sets}, {'msgset': 'm', 'sets': by_value(2, clean)}]})
    assert refused['msgsets']['m']['has_lines'] is False
    assert results(refused['calls'][0]) == want
    assert results(refused['calls'][1]) == [w for s, w in zip(sets, want) if by_value_able(s[0])]
    assert [line_launches(c['launches']) for c in refused['calls']] == [(0, 1), (0, 1)]
    sets1, want1 = case_reference(1, ref.POP)
    t1 = table(1)
    with api.MessageSet.create(1, ref.POP, MSGS, lines=True) as ms, api.KeySet.create(1, t1['blobs'], t1['fmt']) as ks:
        assert ms.info()['has_lines'] is False
        got1, launches1 = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(ms, ks, sets1))
    assert got1 == want1 and line_launches(launches1) == (0, 1)


def test_an_entry_without_rows_makes_the_call_walk(api):
    """A set made from points (debug_msgset_from_points; Basic): the hash points of MSGS, and one more entry (x of a hash point, 0):
    finite, its first tangent vertical, so it has no usable rows.  A call that names it walks ALL its items (k_linesp) and gives
    what the same call gives on a set without rows; a call that does not name it takes the keyed kernel; same statuses and aux."""
    sets, want = case_reference(2, ref.BASIC)
    pts = mb.z_one(api, 2, api.hash_to_point(2, MSGS, api.DST[(2, ref.BASIC)]))
    aff = [p[:192] for p in pts]
    aff.append(aff[0][:96] + bytes(96))
    NOROWS = N_MSGS
    t = table(2)
    clean = [s for s in sets if by_value_able(s[0])]
    want_clean = [w for s, w in zip(sets, want) if by_value_able(s[0])]
    naming = [(list(idx), list(midx), sig) for idx, midx, sig in clean]
    touched = [k for k, s in enumerate(clean) if len(s[0]) in (31, 65)]
    assert len(touched) == 2
    for k in touched:
        naming[k][1][len(naming[k][1]) // 2] = NOROWS
    with api.debug_msgset_from_points(2, aff, lines=True) as rows, api.debug_msgset_from_points(2, aff) as plain:
        assert rows.info()['has_lines'] is True and rows.info()['n'] == N_MSGS + 1
        keyed, launches_k = profiled(api, lambda: api.aggregate_verify_msgset_batch(rows, by_value(2, clean)))
        walked, launches_w = profiled(api, lambda: api.aggregate_verify_msgset_batch(rows, by_value(2, naming)))
        same, launches_s = profiled(api, lambda: api.aggregate_verify_msgset_batch(plain, by_value(2, naming)))
    assert keyed == want_clean and line_launches(launches_k) == (1, 1)
    assert walked == same
    assert [r for k, r in enumerate(walked) if k not in touched] == [w for k, w in enumerate(want_clean) if k not in touched]
    assert all(walked[k][0] != OK for k in touched)
    assert line_launches(launches_w) == (0, 1) and line_launches(launches_s) == (0, 1)


# ------------------------------------------------------------------ 3. merging shows in the launch count
N_SETS, PER_SET = 1040, 63


def tamper_kind(s):
    """about one set in seven: 1 = the next set's signature, 2 = the identity signature, 3 = the identity entry at one position, 4 =
    the undecodable entry, 5 = a key position outside the table, 6 = a message index outside the message set"""
    return {3: 1, 13: 2, 23: 3, 33: 4, 37: 5, 39: 6}.get(s % 40, 0)


def test_one_round_where_by_value_needs_two(api):
    """1,040 sets of 63 pairs under ProofOfPossession, 3 distinct entries per set: 65,520 pairs but 3,120 + 1,040 = 4,160 flat items,
    ONE round of the line kernel; the by-value call on the same data has 66,560 items and needs two.  Statuses and aux equal the
    tamper pattern, which the oracle confirms on the first set of every kind and on the last set."""
    sg, scheme = 1, ref.POP
    bo, t = util.load_c_oracle(), table(sg)
    rng = random.Random(1040)
    idx = [[rng.choice(t['plain']) for _ in range(PER_SET)] for _ in range(N_SETS)]
    midx = []
    for s in range(N_SETS):
        e = rng.sample(DISTINCT, 3)
        midx.append([e[j % 3] for j in range(PER_SET)])
    orig = signed_sets(sg, scheme, [(list(zip(idx[s], midx[s])), None) for s in range(N_SETS)])
    sigs, expect = list(orig), []
    for s in range(N_SETS):
        k, pos = tamper_kind(s), s % PER_SET
        if k == 1:
            sigs[s] = orig[(s + 1) % N_SETS]
        elif k == 2:
            sigs[s] = mb.identity(sg)
        elif k in (3, 4, 5):
            idx[s][pos] = {3: IDENT, 4: BAD, 5: N + s}[k]
        elif k == 6:
            midx[s][pos] = N_MSGS + s
        expect.append({0: (OK, NO_AUX), 1: (INVALID, NO_AUX), 2: (SIG_IDENTITY, NO_AUX), 3: (PK_IDENTITY, (pos + 1, 0)), 4: (api.BAD_ENCODING, NO_AUX),
                       5: (E_ARG, NO_AUX), 6: (E_ARG, NO_AUX)}[k])
    sets = [(idx[s], midx[s], sigs[s]) for s in range(N_SETS)]
    for s in (0, 3, 13, 23, 33, 37, 39, N_SETS - 1):
        assert oracle_set(bo, sg, scheme, *sets[s]) == expect[s], s
    with api.MessageSet.create(sg, scheme, MSGS) as ms, api.KeySet.create(sg, t['blobs'], t['fmt']) as ks:
        got, launches = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(ms, ks, sets))
    bad = [(s, got[s], expect[s]) for s in range(N_SETS) if got[s] != expect[s]][:10]
    assert not bad and len(got) == N_SETS, bad
    assert line_launches(launches) == (0, 1) and summed(launches) == 1, launches
    # the same data by value (a key that cannot be sent replaced by a finite one: only the launch count and the other sets count)
    usable = [s for s in range(N_SETS) if tamper_kind(s) in (0, 1, 2, 3)]
    hashed = [([t['points'][i if i < N and i != BAD else 0] for i in idx[s]], [message_of(m) for m in midx[s]], sigs[s]) for s in range(N_SETS)]
    got_h, launches_h = profiled(api, lambda: api.aggregate_verify_batch(sg, scheme, hashed))
    assert line_launches(launches_h) == (0, 2), launches_h
    assert [got_h[s] for s in usable] == [expect[s] for s in usable]


def test_two_rounds_when_nothing_merges(api):
    """The same shape under Basic with 63 distinct entries per set (a message set of 65,520 entries): 66,560 flat items, two rounds of
    33,280, the second starting inside set 528; no class sum.  The oracle confirms the pattern on the first set of every kind, the
    last set and the sets around the round border."""
    sg, scheme = 1, ref.BASIC
    bo, t = util.load_c_oracle(), table(sg)
    rng = random.Random(1041)
    msgs = [b'nothing merges %d' % i for i in range(N_SETS * PER_SET)]
    idx = [[rng.choice(t['plain']) for _ in range(PER_SET)] for _ in range(N_SETS)]
    midx = [list(range(PER_SET * s, PER_SET * (s + 1))) for s in range(N_SETS)]
    flat_sigs = api.sign_batch(sg, scheme, [t['ks'][i] for ix in idx for i in ix], msgs)[1]
    orig = api.sum_batch(sg, [flat_sigs[PER_SET * s:PER_SET * (s + 1)] for s in range(N_SETS)])
    sigs, expect = list(orig), []
    for s in range(N_SETS):
        k, pos = tamper_kind(s), s % PER_SET
        if k == 1:
            sigs[s] = orig[(s + 1) % N_SETS]
        elif k == 2:
            sigs[s] = mb.identity(sg)
        elif k in (3, 4, 5):
            idx[s][pos] = {3: IDENT, 4: BAD, 5: N + s}[k]
        elif k == 6:
            midx[s][pos] = len(msgs) + s
        expect.append({0: (OK, NO_AUX), 1: (INVALID, NO_AUX), 2: (SIG_IDENTITY, NO_AUX), 3: (PK_IDENTITY, (pos + 1, 0)), 4: (api.BAD_ENCODING, NO_AUX),
                       5: (E_ARG, NO_AUX), 6: (E_ARG, NO_AUX)}[k])
    border = 33280 // PER_SET
    assert PER_SET * border < 33280 < PER_SET * (border + 1)

    def oracle(s):
        if any(m >= len(msgs) for m in midx[s]):
            return E_ARG, NO_AUX
        if any(i >= N for i in idx[s]):
            return E_ARG, NO_AUX
        bad = [t['status'][i] for i in idx[s] if t['status'][i]]
        if bad:
            return bad[0], NO_AUX
        ms_ = [msgs[m] for m in midx[s]]
        offs = (ctypes.c_uint64 * (PER_SET + 1))()
        for j, m in enumerate(ms_):
            offs[j + 1] = offs[j] + len(m)
        aux = (ctypes.c_uint64 * 2)()
        V = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)  # noqa: E731
        st = bo.bo_aggregate_verify(sg, scheme, V(b''.join(t['points'][i] for i in idx[s])), V(b''.join(ms_)), ctypes.cast(offs, ctypes.c_void_p), PER_SET,
                                    V(sigs[s]), 4, ctypes.cast(aux, ctypes.c_void_p))
        return st, (aux[0], aux[1])

    for s in (0, 3, 13, 23, 33, 37, 39, N_SETS - 1, border - 1, border, border + 1):
        assert oracle(s) == expect[s], s
    sets = [(idx[s], midx[s], sigs[s]) for s in range(N_SETS)]
    with api.MessageSet.create(sg, scheme, msgs) as ms, api.KeySet.create(sg, t['blobs'], t['fmt']) as ks:
        got, launches = profiled(api, lambda: api.aggregate_verify_msgset_indexed_batch(ms, ks, sets))
    bad = [(s, got[s], expect[s]) for s in range(N_SETS) if got[s] != expect[s]][:10]
    assert not bad and len(got) == N_SETS, bad
    assert line_launches(launches) == (0, 2) and summed(launches) == 0, launches


# ------------------------------------------------------------------ 4. device pointers
def test_device_pointers(api):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sg, scheme = 2, ref.BASIC
    sets, want = case_reference(sg, scheme)
    t = table(sg)
    clean = [s for s in sets if by_value_able(s[0])]
    u8 = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)  # noqa: E731
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)  # noqa: E731
    u32 = lambda v: torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in v], dtype=torch.int32, device=dev)  # noqa: E731

    def offsets(ss):
        o = [0]
        for ix, _, _ in ss:
            o.append(o[-1] + len(ix))
        return o

    with api.MessageSet.create(sg, scheme, MSGS, lines=True) as ms, api.KeySet.create(sg, t['blobs'], t['fmt']) as ks:
        st, aux = ops.aggregate_verify_msgset_indexed_batch(ms, u32([m for _, mi, _ in sets for m in mi]), ks, u32([i for ix, _, _ in sets for i in ix]),
                                                            i64(offsets(sets)), len(sets), u8(b''.join(g for _, _, g in sets)))
        assert st.device == dev and st.dtype == torch.int32 and aux.device == dev and tuple(aux.shape) == (len(sets), 2)
        host = api.aggregate_verify_msgset_indexed_batch(ms, ks, sets)
        st_v, aux_v = ops.aggregate_verify_msgset_batch(ms, u32([m for _, mi, _ in clean for m in mi]), u8(b''.join(t['points'][i] for ix, _, _ in clean for i in ix)),
                                                        i64(offsets(clean)), len(clean), u8(b''.join(g for _, _, g in clean)))
        assert st_v.device == dev and aux_v.device == dev
        host_v = api.aggregate_verify_msgset_batch(ms, by_value(sg, clean))
    got = [(s, (a[0], a[1])) for s, a in zip(st.cpu().tolist(), aux.cpu().tolist())]
    got_v = [(s, (a[0], a[1])) for s, a in zip(st_v.cpu().tolist(), aux_v.cpu().tolist())]
    assert got == host == want
    assert got_v == host_v == [w for s, w in zip(sets, want) if by_value_able(s[0])]


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors(api):
    sg, scheme = 1, ref.POP
    sets, _ = case_reference(sg, scheme)
    sets = sets[1:4]
    t = table(sg)
    lib = api.init()
    n_sets = len(sets)
    soffs = (ctypes.c_uint64 * (n_sets + 1))()
    for s, (ix, _, _) in enumerate(sets):
        soffs[s + 1] = soffs[s] + len(ix)
    idx = (ctypes.c_uint32 * soffs[n_sets])(*[i for ix, _, _ in sets for i in ix])
    midx = (ctypes.c_uint32 * soffs[n_sets])(*[m for _, mi, _ in sets for m in mi])
    pkb = b''.join(t['points'][i] for ix, _, _ in sets for i in ix)
    sgb = b''.join(g for _, _, g in sets)
    V = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    untouched = ([77] * n_sets, [99] * (2 * n_sets))

    def call(mh, midx_p, soffs_p, n, kh=None):
        st = (ctypes.c_int32 * n_sets)(*[77] * n_sets)
        aux = (ctypes.c_uint64 * (2 * n_sets))(*[99] * (2 * n_sets))
        if kh is None:
            rc = lib.blsgpu_aggregate_verify_msgset_batch(mh, midx_p, api._ptr(pkb), soffs_p, n, api._ptr(sgb), api.FMT_RAW_PROJ, V(st), V(aux))
        else:
            rc = lib.blsgpu_aggregate_verify_msgset_indexed_batch(mh, midx_p, kh, V(idx), soffs_p, n, api._ptr(sgb), api.FMT_RAW_PROJ, V(st), V(aux))
        return rc, list(st), list(aux)

    t2 = table(2)
    with api.MessageSet.create(sg, scheme, MSGS) as ms, api.KeySet.create(sg, t['blobs'], t['fmt']) as ks, api.KeySet.create(2, t2['blobs'], t2['fmt']) as other:
        mh = ms.handle
        for kh in (None, ks.handle):
            rc, st, aux = call(mh, V(midx), V(soffs), n_sets, kh)
            assert rc == 0 and st == [OK] * n_sets and aux == [0] * (2 * n_sets)
            down = (ctypes.c_uint64 * (n_sets + 1))(*[soffs[0], soffs[2], soffs[1], soffs[3]])
            assert call(mh, V(midx), V(down), n_sets, kh) == (E_ARG,) + untouched          # offsets that decrease
            assert call(mh, None, V(soffs), n_sets, kh) == (E_ARG,) + untouched            # null msg_idx with T > 0
            assert call(mh, V(midx), None, n_sets, kh) == (E_ARG,) + untouched             # null set_offsets
            assert call(mh, V(midx), V(soffs), 0, kh) == (0,) + untouched                  # no sets: nothing to do
            assert call(ks.handle, V(midx), V(soffs), n_sets, kh) == (E_ARG,) + untouched  # a key set's handle as the message set
        assert call(mh, V(midx), V(soffs), n_sets, other.handle) == (E_ARG,) + untouched   # a key set of the other orientation
        kh = ks.handle
    assert call(mh, V(midx), V(soffs), n_sets) == (E_ARG,) + untouched                     # a stale message-set handle
    with api.MessageSet.create(sg, scheme, MSGS) as ms:
        assert call(ms.handle, V(midx), V(soffs), n_sets, kh) == (E_ARG,) + untouched      # a stale key-set handle
        with pytest.raises(ValueError):
            api.aggregate_verify_msgset_batch(ms, [([pkb[:288]], [1, 2], sgb[:144])])


# ------------------------------------------------------------------ 6. after update / append
@pytest.mark.parametrize('sg', [1, 2])
def test_after_update_and_append(api, sg):
    """the same call sees the new entries: a set that names an appended position, and an updated position that turns OK into INVALID"""
    scheme = ref.POP
    bo, t = util.load_c_oracle(), table(sg)
    k = t['plain'][:6]
    extra = [b'appended entry %d' % i for i in range(3)]
    specs = [([(k[0], 1), (k[1], 1), (k[2], 2)], None), ([(k[3], 6), (k[4], 6)], None)]
    sig_a, sig_b = signed_sets(sg, scheme, specs)
    # the third set is signed under an appended message, for two keys of one class
    both = (t['ks'][k[4]] + t['ks'][k[5]]) % R
    sig_c = api.sum_batch(sg, [mb.signatures(api, sg, scheme, [both, t['ks'][k[0]]], [extra[1], MSGS[2]])])[0]
    sets = [([k[0], k[1], k[2]], [1, 1, 2], sig_a), ([k[3], k[4]], [6, 6], sig_b), ([k[4], k[5], k[0]], [N_MSGS + 1, N_MSGS + 1, 2], sig_c)]
    with api.MessageSet.create(sg, scheme, MSGS, lines=True) as ms:
        before = api.aggregate_verify_msgset_batch(ms, by_value(sg, sets))
        assert before == [(OK, NO_AUX), (OK, NO_AUX), (E_ARG, NO_AUX)]
        assert ms.append(extra) == N_MSGS
        grown = api.aggregate_verify_msgset_batch(ms, by_value(sg, sets))
        ms.update([6], [b'entry 6 rewritten'])
        after = api.aggregate_verify_msgset_batch(ms, by_value(sg, sets))
    final = list(MSGS) + extra
    final[6] = b'entry 6 rewritten'

    def oracle(idx, midx, sig, msgs_now):
        ms_ = [msgs_now[m] for m in midx]
        offs = (ctypes.c_uint64 * (len(ms_) + 1))()
        for j, m in enumerate(ms_):
            offs[j + 1] = offs[j] + len(m)
        aux = (ctypes.c_uint64 * 2)()
        V = lambda b: ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)  # noqa: E731
        st = bo.bo_aggregate_verify(sg, scheme, V(b''.join(t['points'][i] for i in idx)), V(b''.join(ms_)), ctypes.cast(offs, ctypes.c_void_p), len(ms_), V(sig),
                                    4, ctypes.cast(aux, ctypes.c_void_p))
        return st, (aux[0], aux[1])

    want_grown = [oracle(*s, list(MSGS) + extra) for s in sets]
    want_after = [oracle(*s, final) for s in sets]
    assert want_grown == [(OK, NO_AUX)] * 3 and want_after == [(OK, NO_AUX), (INVALID, NO_AUX), (OK, NO_AUX)]
    assert grown == want_grown and after == want_after
