"""Registered key sets with line tables on the one-wave-per-item pairing path (BLSGPU_WIDE_MAX < n <= BLSGPU_COOP_MAX items): the
one-key-per-item indexed calls of Bls12381G1Impl then run k_pairing_coop_keyed, whose Miller loop reads the key's rows and the
constant's and walks nothing (csrc/coop.cuh coop_miller2_tables), where they ran k_pairing_coop.  The kernel itself goes through
its hook on the crafted pairs of field_cases (exact easy-part values and verdicts of the oracle); the calls use the items, the
oracle statuses and the worker of tests/test_gpu_keyset_lines.py, and the launch counts of the profile say which of the two
kernels ran, so no test can pass by falling back.  Worker runs are one attempt each, with their own time limit."""
import ctypes
import random

import pytest

import field_cases as fc
import keyset_cases as kc
import multi_batch_cases as mb
import test_gpu_keyset_lines as kl
import util
from util import ref

pytestmark = pytest.mark.gpu

OK, INVALID, PK_IDENTITY, E_ARG = kl.OK, kl.INVALID, kl.PK_IDENTITY, kl.E_ARG
ONE_WAVE = {'BLSGPU_WIDE_MAX': '0'}              # 130 items then run one wave each
PAIR_COUNTS = (1, 2, 33, 65)
KEYED = [cs for cs in fc.pairing_cases() if cs['fixed_g2'] == 2]


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


def coop_launches(got):
    return got.get('k_pairing_coop_keyed', 0), got.get('k_pairing_coop', 0)


def no_line_kernel(launches):
    return not any(k.startswith('k_lines2s') for k in launches)


# ------------------------------------------------------------------ 1. the kernel through its hook
def case_keys():
    """the cases' Q0 as trusted RAW_AFFINE keys, one entry per case (points outside the subgroup among them)"""
    return [util.g2_aff_raw(cs['pairs'][0][1]) for cs in KEYED]


def test_hook_easy_part_and_verdict(api):
    """1, 2, 33 and 65 items (the list cycles, so entries repeat and their order is not the items'): the exported easy-part value is
    the oracle's miller_loop(pairs)^((p^6 - 1)(p^2 + 1)) exactly, and the verdict is OK exactly where its pairing product is one"""
    with api.KeySet.create(1, case_keys(), api.FMT_RAW_AFFINE, lines=True) as ks:
        assert ks.info()['has_lines'] is True
        for k, n in enumerate(PAIR_COUNTS):
            pos = [(3 * k + i) % len(KEYED) for i in range(n)]
            cases = [KEYED[p] for p in pos]
            outs = api.debug_coop_pairing_keyed(0, ks, pos, [cs['vecs'] for cs in cases])
            assert len(outs) == n
            for cs, o in zip(cases, outs):
                fc.check_easy(cs, o)
            got = api.debug_coop_pairing_keyed(1, ks, pos, [cs['vecs'] for cs in cases])
            want = [fc.pairing_expected(cs)[2] for cs in cases]
            assert got == want, [cs['name'] for cs, g, w in zip(cases, got, want) if g != w]
        assert {fc.pairing_expected(cs)[2] for cs in KEYED} == {fc.BLS_OK, fc.BLS_INVALID}


def test_hook_skips_flagged_items_and_reads_the_set_not_the_record(api):
    """items that are not OK on entry are skipped (status kept, sentinel kept); the record's own Q0 is not read: with another point in
    its place the values are those of the entry"""
    n = 9
    pos = [(2 + i) % len(KEYED) for i in range(n)]
    cases = [KEYED[p] for p in pos]
    other = KEYED[0]['vecs'][2:6]
    vecs = [cs['vecs'][:2] + other + cs['vecs'][6:] for cs in cases]
    flagged = {0, 4, n - 1}
    status = [7 if i in flagged else OK for i in range(n)]
    with api.KeySet.create(1, case_keys(), api.FMT_RAW_AFFINE, lines=True) as ks:
        outs = api.debug_coop_pairing_keyed(0, ks, pos, vecs, status)
        for i, (cs, o) in enumerate(zip(cases, outs)):
            if i in flagged:
                assert all(x == api.COOP_SENTINEL for v in o for x in v), 'item %d was flagged and its easy-part slot was written' % i
            else:
                fc.check_easy(cs, o)
        got = api.debug_coop_pairing_keyed(1, ks, pos, vecs, status)
        assert got == [7 if i in flagged else fc.pairing_expected(cs)[2] for i, cs in enumerate(cases)]


def test_hook_argument_errors(api):
    vecs = [KEYED[0]['vecs']]
    with api.KeySet.create(1, case_keys(), api.FMT_RAW_AFFINE) as plain, api.KeySet.create(1, case_keys(), api.FMT_RAW_AFFINE, lines=True) as ks:
        for mode in (0, 1):
            with pytest.raises(Exception):
                api.debug_coop_pairing_keyed(mode, plain, [0], vecs)                  # a set without lines
            with pytest.raises(Exception):
                api.debug_coop_pairing_keyed(mode, ks, [len(KEYED)], vecs)            # an index outside the set
        with pytest.raises(Exception):
            api.debug_coop_pairing_keyed(2, ks, [0], vecs)
        with pytest.raises(Exception):
            api.debug_coop_pairing_keyed(1, ks, [0] * 4097, vecs * 4097)
        lib = api.init()
        st, idx, arr = (ctypes.c_int32 * 1)(0), (ctypes.c_uint32 * 1)(0), (ctypes.c_int32 * 168)(*[x for v in vecs[0] for x in v])
        p = lambda a: ctypes.cast(a, ctypes.c_void_p)
        assert lib.blsgpu_debug_coop_pairing_keyed(1, plain.handle, p(idx), p(arr), 1, p(st), None) == E_ARG
        assert lib.blsgpu_debug_coop_pairing_keyed(1, ks.handle, p(idx), p(arr), 1, p(st), None) == 0 and st[0] == fc.pairing_expected(KEYED[0])[2]


# ------------------------------------------------------------------ 2. 130 items on the one-wave path, all three schemes
@pytest.mark.parametrize('scheme,_id', kl.SCHEMES, ids=[s[1] for s in kl.SCHEMES])
def test_keyed_kernel_on_the_one_wave_path(api, tmp_path, scheme, _id):
    """BLSGPU_WIDE_MAX=0: over the set with lines k_pairing_coop_keyed runs once and k_pairing_coop not at all; over the set without
    lines the reverse; the oracle's statuses both times (tampered signature, wrong message, identity signature, identity entry,
    invalid entry, position past the end, duplicate key, generator)"""
    call, want = kl.indexed_reference(scheme)
    t = kc.table(api, 1)
    got = kl.run_worker(tmp_path, 'coop_keyed', ONE_WAVE, kl.table_sets(t, lines=True, plain=False),
                        [dict(call, set='lines', scheme=scheme), dict(call, set='plain', scheme=scheme)])
    assert got['sets']['lines']['has_lines'] is True and got['sets']['plain']['has_lines'] is False
    keyed, plain = got['calls']
    print(keyed['launches'], plain['launches'])
    assert keyed['st'] == want and plain['st'] == want
    assert coop_launches(keyed['launches']) == (1, 0)
    assert coop_launches(plain['launches']) == (0, 1)
    assert no_line_kernel(keyed['launches']) and no_line_kernel(plain['launches'])


# ------------------------------------------------------------------ 3. shared-message verify
def test_shared_indexed_takes_the_keyed_kernel(api, tmp_path):
    """groups of 1, 0, 31, 33, 0, 65 items under ProofOfPossession and MessageAugmentation, over the set with lines and the one without"""
    t = kc.table(api, 1)
    calls, wants = [], []
    for scheme in (ref.POP, ref.AUG):
        groups, want = kl.shared_reference(scheme)
        for name in ('lines', 'plain'):
            calls.append({'set': name, 'scheme': scheme, 'groups': groups})
            wants.append((want, name))
    got = kl.run_worker(tmp_path, 'coop_shared', ONE_WAVE, kl.table_sets(t, lines=True, plain=False), calls)['calls']
    for g, (want, name) in zip(got, wants):
        assert g['st'] == want
        assert coop_launches(g['launches']) == ((1, 0) if name == 'lines' else (0, 1)), (name, g['launches'])
        assert no_line_kernel(g['launches'])


# ------------------------------------------------------------------ 4. refused lines
def test_refused_lines_change_nothing(api, tmp_path):
    """BLSGPU_KEYSET_TABLE_MB=1: 4.6 MiB of rows are refused, the set works without them and the walked kernel runs"""
    call, want = kl.indexed_reference(ref.POP)
    t = kc.table(api, 1)
    got = kl.run_worker(tmp_path, 'coop_refused', dict(ONE_WAVE, BLSGPU_KEYSET_TABLE_MB='1'), kl.table_sets(t, lines=True), [dict(call, set='lines', scheme=ref.POP)])
    assert got['sets']['lines']['has_lines'] is False
    assert got['calls'][0]['st'] == want
    assert coop_launches(got['calls'][0]['launches']) == (0, 1)


# ------------------------------------------------------------------ 5. an entry without usable rows
def test_fallback_when_a_named_entry_has_no_rows(api, tmp_path):
    """the entry (x of a real key, 0) of tests/test_gpu_keyset_lines.py: a call that names it walks the keys of ALL its items, by
    k_pairing_coop, with the statuses of the same call over a set without lines; a call that does not name it takes the keyed kernel"""
    call, want = kl.indexed_reference(ref.POP)
    t = kc.table(api, 1)
    Y0 = next(i for i in t['valid'] if i not in call['idx'] and i not in (kc.GEN, kc.DUP_A, kc.DUP_B))
    aff = [bytes(192) if k in (0, None) else p[:192] for p, k in zip(t['points'], t['ks'])]
    aff[Y0] = aff[Y0][:96] + bytes(96)
    sets = {name: {'sg': 1, 'keys': aff, 'fmt': api.FMT_RAW_AFFINE, 'tables': False, 'lines': lines} for name, lines in (('lines', True), ('plain', False))}
    naming = dict(call, idx=list(call['idx']))
    naming['idx'][50] = naming['idx'][90] = Y0
    got = kl.run_worker(tmp_path, 'coop_fallback', ONE_WAVE, sets, [dict(naming, set='lines', scheme=ref.POP), dict(naming, set='plain', scheme=ref.POP),
                                                                   dict(call, set='lines', scheme=ref.POP)])
    assert got['sets']['lines']['has_lines'] is True
    walked, plain, keyed = got['calls']
    want_raw = [PK_IDENTITY if i == kl.AT_BAD else w for i, w in enumerate(want)]     # raw input is trusted: the bad blob is the zero record here
    assert walked['st'] == plain['st']
    assert [s for i, s in enumerate(walked['st']) if i not in (50, 90)] == [s for i, s in enumerate(want_raw) if i not in (50, 90)]
    assert walked['st'][50] != OK and walked['st'][90] != OK
    assert coop_launches(walked['launches']) == (0, 1) and coop_launches(plain['launches']) == (0, 1)
    assert keyed['st'] == want_raw
    assert coop_launches(keyed['launches']) == (1, 0)


# ------------------------------------------------------------------ 6. default knobs, in process: both branches of run_verify_items
@pytest.mark.parametrize('n', [513, 1025])
def test_default_knobs_take_the_keyed_kernel(api, bo, n):
    """513 items (the row-wide hash and k_prepare_hashed) and 1,025 (k_prepare) over a set with lines: the tamper pattern, confirmed
    by the oracle on 24 spread items; k_pairing_coop_keyed ran once and no line kernel"""
    idx, sigs, msgs, expect = kl.signed_batch(n)
    kl.spot(bo, api, n)
    t = kc.table(api, 1)
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        assert ks.info()['has_lines'] is True
        got, launches = kl.profiled(api, lambda: api.verify_indexed_batch(ks, ref.POP, idx, sigs, msgs))
    bad = [(i, got[i], expect[i]) for i in range(n) if got[i] != expect[i]][:10]
    assert not bad and len(got) == n, bad
    assert coop_launches(launches) == (1, 0) and no_line_kernel(launches), launches


# ------------------------------------------------------------------ 7. the rows of an updated and of an appended entry
def test_updated_and_appended_entries_are_read_from_their_new_rows(api, bo):
    """513 items, default knobs.  KeySet.update gives one named entry another key and turns another into the identity, KeySet.append
    adds one: items signed under the new keys are OK, items signed under the replaced key INVALID, the identity entry PK_IDENTITY --
    the oracle's statuses under the FINAL key list for every item that names a touched entry and for a spread of the others"""
    n = 513
    idx, sigs, msgs, expect = kl.signed_batch(n)
    idx, sigs, expect = list(idx), list(sigs), list(expect)
    t = kc.table(api, 1)
    plain = [i for i in range(n) if kl.tamper_kind(i) == 0]
    A, B = idx[plain[0]], next(idx[i] for i in plain if idx[i] != idx[plain[0]])
    rng = random.Random(7)
    k_new, k_app = rng.randrange(1, kc.R), rng.randrange(1, kc.R)
    blobs = api.serialize(2, mb.key_points(api, 1, [k_new, k_app]))
    pts = api.deserialize(2, blobs)[0]
    points = list(t['points']) + [pts[1]]
    points[A], points[B] = pts[0], t['points'][kc.IDENT]
    APP = kc.N
    # two slots signed under the new key of A, one under the appended key; every other item that names A keeps its old signature
    s_new = [i for i in plain if idx[i] not in (A, B)][:3]
    for s, (pos, k) in zip(s_new, ((A, k_new), (A, k_new), (APP, k_app))):
        idx[s] = pos
        sigs[s] = kl.sign(api, ref.POP, [k], [msgs[s]])[0]

    def oracle(i):
        ix = idx[i]
        if ix > APP:
            return E_ARG
        if ix < kc.N and t['status'][ix]:
            return t['status'][ix]
        return bo.bo_verify(1, ref.POP, points[ix], sigs[i], msgs[i], len(msgs[i]))
    touched = [i for i in range(n) if idx[i] in (A, B, APP)]
    for i in touched:
        expect[i] = oracle(i)
    assert [expect[s] for s in s_new] == [OK, OK, OK]
    old_a = [i for i in plain if idx[i] == A and i not in s_new]
    at_b = [i for i in plain if idx[i] == B]
    assert old_a and at_b and all(expect[i] == INVALID for i in old_a) and all(expect[i] == PK_IDENTITY for i in at_b)
    for i in random.Random(n).sample(range(n), 12):
        assert oracle(i) == expect[i], i
    with api.KeySet.create(1, t['blobs'], t['fmt'], lines=True) as ks:
        assert ks.update([A, B], [blobs[0], t['blobs'][kc.IDENT]]) == [OK, OK]
        first, st = ks.append([blobs[1]])
        assert (first, st) == (APP, [OK]) and ks.info()['has_lines'] is True
        got, launches = kl.profiled(api, lambda: api.verify_indexed_batch(ks, ref.POP, idx, sigs, msgs))
    bad = [(i, got[i], expect[i]) for i in range(n) if got[i] != expect[i]][:10]
    assert not bad and len(got) == n, bad
    assert coop_launches(launches) == (1, 0) and no_line_kernel(launches), launches
