"""The per-item functions of the aggregate verify by message index (csrc/agg_msgset.cuh) on the host, against Python models on the
ragged shapes of test_hostsim_agg_batch.py plus random ones: the classes of every set against a dict per set (nothing merges across
a set border), the class offsets and the member permutation against a sort, the strips' member ranges (every pair exactly once, in
its class's strips), Basic's duplicate pair when two different positions hold equal records, and the precedence."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util
from test_hostsim_agg_batch import SIZE_SETS, random_sizes, u32, u64

NONE = 0xffffffff
SKIP = 0xffffffff
PRE_NONE = 0xffffffffffffffff
E_ARG = -3
OK, INVALID, SIG_IDENTITY, PK_IDENTITY, DUPLICATE = 0, 1, 2, 3, 4
WORDS = 24


@pytest.fixture(scope='module')
def lib():
    src = os.path.join(util.ROOT, 'tests', 'hostsim_agg_msgset', 'agg_msgset_hostsim.cpp')
    d = tempfile.mkdtemp(prefix='agg_msgset_hostsim_')
    so = os.path.join(d, 'libagg_msgset_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', so, src])
    lb = ctypes.CDLL(so)
    lb.hs_aggm_classes.restype = ctypes.c_uint32
    lb.hs_aggm_strips.restype = ctypes.c_int64
    lb.hs_aggm_strips.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lb.hs_aggm_decide.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p]
    lb.hs_keyset_pre_key.restype = ctypes.c_uint64
    lb.hs_keyset_pre_key.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int32]
    lb.hs_msgset_entry_of.restype = ctypes.c_uint32
    lb.hs_msgset_entry_of.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    return lb


def records(rng, n_msgs):
    """n_msgs records of WORDS words: about a third repeat an earlier record word for word (equal bytes at another position), some
    share the hashed prefix with an earlier one and differ behind it (one hash chain, two classes)"""
    recs = []
    for k in range(n_msgs):
        r = rng.random()
        if k and r < 0.3:
            recs.append(list(rng.choice(recs)))
        elif k and r < 0.45:
            base = list(rng.choice(recs))
            base[WORDS - 1] ^= 1 + rng.randrange(7)
            recs.append(base)
        else:
            recs.append([rng.getrandbits(32) for _ in range(WORDS)])
    return recs


def run_classes(lib, rng, sizes, by_record, n_msgs, tight, shuffle, skip_p=0.05):
    offs = [0]
    for t in sizes:
        offs.append(offs[-1] + t)
    T, n_sets = offs[-1], len(sizes)
    sid = [b for b, t in enumerate(sizes) for _ in range(t)]
    recs = records(rng, n_msgs)
    # few entries, so that sets repeat them within and across sets -- neighbouring sets name the same ones
    cmsg = [SKIP if rng.random() < skip_p else rng.randrange(n_msgs) for _ in range(T)]
    cap = 2
    while cap <= (T if tight else max(2 * T, 63)):
        cap *= 2
    order = list(range(T))
    if shuffle:
        rng.shuffle(order)
    A = lambda n: (ctypes.c_uint32 * max(n, 1))()  # noqa: E731
    B = lambda n: (ctypes.c_uint64 * max(n, 1))()  # noqa: E731
    cid, csid, cent, crep, perm, dup = A(T), A(T + 1), A(T + 1), A(T + 1), A(T), A(2 * n_sets)
    coffs, moffs = B(n_sets + 1), B(T + 1)
    C = lib.hs_aggm_classes(T, n_sets, int(by_record), u32(cmsg), u32(sid), u64(offs), u32([w for r in recs for w in r]), WORDS, cap, u32(order), cid, coffs,
                            csid, cent, crep, moffs, perm, dup)
    return dict(T=T, n_sets=n_sets, offs=offs, sid=sid, recs=recs, cmsg=cmsg, C=C, cid=list(cid)[:T], csid=list(csid)[:C], cent=list(cent)[:C],
                crep=list(crep)[:C], coffs=list(coffs), moffs=list(moffs)[:C + 1], perm=list(perm)[:T], dup=list(dup)[:2 * n_sets], order=order)


def class_key(r, by_record, k):
    return 'skip' if k == SKIP else (tuple(r['recs'][k]) if by_record else k)


@pytest.mark.parametrize('sizes', SIZE_SETS + [None], ids=lambda s: 'random' if s is None else 'x'.join(map(str, s))[:24])
@pytest.mark.parametrize('by_record', [False, True], ids=['pop-by-position', 'basic-by-record'])
@pytest.mark.parametrize('tight', [False, True], ids=['cap2n', 'cap-tight'])
def test_classes_numbering_and_permutation(lib, sizes, by_record, tight):
    rng = random.Random(str(sizes) + str(by_record) + str(tight))
    for trial in range(6):
        sz = sizes if sizes is not None else random_sizes(rng)
        r = run_classes(lib, rng, sz, by_record, rng.choice([1, 2, 5, 40]), tight, trial % 2 == 1)
        T, offs = r['T'], r['offs']
        # the classes of every set against a dict per set: members with the same key, and nothing merges across a set border
        model = []
        for b, t in enumerate(sz):
            d = {}
            for l in range(t):
                d.setdefault(class_key(r, by_record, r['cmsg'][offs[b] + l]), []).append(offs[b] + l)
            model.append(d)
        assert r['C'] == sum(len(d) for d in model)
        assert r['coffs'] == [sum(len(d) for d in model[:b]) for b in range(len(sz) + 1)]        # class offsets: a prefix sum of the per-set counts
        members = {}
        for i in range(T):
            members.setdefault(r['cid'][i], []).append(i)
        for b, d in enumerate(model):
            ids = range(r['coffs'][b], r['coffs'][b + 1])
            assert sorted(sorted(members[c]) for c in ids) == sorted(d.values()), (sz, b)
            for c in ids:
                assert r['csid'][c] == b and r['crep'][c] in members[c]
                assert class_key(r, by_record, r['cent'][c]) == class_key(r, by_record, r['cmsg'][members[c][0]])
        # the representative is the first claimant; numbering follows the representatives' pair order
        assert r['crep'] == sorted(r['crep'])
        # member offsets and permutation against a sort by class
        assert r['moffs'] == [sum(len(members[c]) for c in range(k)) for k in range(r['C'] + 1)]
        assert sorted(r['perm']) == list(range(T))
        assert [r['cid'][i] for i in r['perm']] == sorted(r['cid'])
        for c in range(r['C']):
            assert sorted(r['perm'][r['moffs'][c]:r['moffs'][c + 1]]) == sorted(members[c])
        # Basic's duplicate pair from the same table: two DIFFERENT positions with equal records are the same message
        for b, t in enumerate(sz):
            seen, want = {}, (NONE, NONE)
            for l in range(t):
                k = class_key(r, by_record, r['cmsg'][offs[b] + l])
                if k in seen:
                    want = (seen[k], l)
                    break
                seen[k] = l
            assert (r['dup'][2 * b], r['dup'][2 * b + 1]) == want, (sz, b, trial)


def test_equal_records_at_two_positions_are_one_message_under_basic_only(lib):
    rng = random.Random(3)
    rec = [rng.getrandbits(32) for _ in range(WORDS)]
    other = [rng.getrandbits(32) for _ in range(WORDS)]
    flat = rec + other + rec                      # positions 0 and 2 hold equal records
    A = lambda n: (ctypes.c_uint32 * n)()  # noqa: E731
    B = lambda n: (ctypes.c_uint64 * n)()  # noqa: E731
    for by_record, want_c, want_dup in ((1, 3, [0, 2, NONE, NONE]), (0, 4, [NONE, NONE, NONE, NONE])):
        dup = A(4)
        C = lib.hs_aggm_classes(4, 2, by_record, u32([0, 1, 2, 2]), u32([0, 0, 0, 1]), u64([0, 3, 4]), u32(flat), WORDS, 64, u32([0, 1, 2, 3]), A(4), B(3), A(5),
                                A(5), A(5), B(5), A(4), dup)
        assert C == want_c and list(dup) == want_dup          # set 1 names entry 2 too: a class of its own either way


@pytest.mark.parametrize('L', [1, 3, 4, 7, 64])
def test_strip_member_ranges(lib, L):
    rng = random.Random(L)
    for trial in range(8):
        counts = [rng.choice([1, 1, 2, 3, 4, 5, 9, 63, 65, 200]) for _ in range(rng.randrange(1, 40))]
        moffs = [0]
        for t in counts:
            moffs.append(moffs[-1] + t)
        T, C = moffs[-1], len(counts)
        visits, strip_class = (ctypes.c_uint32 * T)(), (ctypes.c_uint32 * T)()
        q = lib.hs_aggm_strips(C, u64(moffs), L, visits, strip_class)
        assert q == sum((t + L - 1) // L for t in counts) and q <= T        # at most as many strips as pairs: the library sizes its buffers by that
        assert list(visits) == [1] * T                                          # each pair exactly once, in its own class's strips (-1 otherwise)
        assert list(strip_class)[:q] == [c for c, t in enumerate(counts) for _ in range((t + L - 1) // L)]


def test_precedence(lib):
    aux = (ctypes.c_uint64 * 2)()
    d = lib.hs_aggm_decide
    pre = lib.hs_keyset_pre_key
    out_of_range, invalid = pre(1, 4, 0), pre(0, 2, 11)
    assert lib.hs_msgset_entry_of(7, 7) == SKIP and lib.hs_msgset_entry_of(6, 7) == 6 and lib.hs_msgset_entry_of(0xffffffff, 7) == SKIP
    # message index first, whatever else holds
    assert d(1, out_of_range, 1, 3, 1, 0, INVALID, aux) == E_ARG and list(aux) == [0, 0]
    assert d(1, PRE_NONE, 1, 3, 1, 0, OK, aux) == E_ARG and list(aux) == [0, 0]
    # then a key index outside the table, then the first invalid entry's creation status
    assert d(0, min(out_of_range, invalid), 1, 3, 1, 0, OK, aux) == E_ARG and list(aux) == [0, 0]
    assert d(0, invalid, 1, 3, 1, 0, OK, aux) == 11 and list(aux) == [0, 0]
    # then the duplicate pair, the identity signature, the first identity key, the product
    assert d(0, PRE_NONE, 1, 3, 1, 0, OK, aux) == DUPLICATE and list(aux) == [1, 3]
    assert d(0, PRE_NONE, NONE, NONE, 1, 0, OK, aux) == SIG_IDENTITY and list(aux) == [0, 0]
    assert d(0, PRE_NONE, NONE, NONE, 0, 6, OK, aux) == PK_IDENTITY and list(aux) == [7, 0]
    assert d(0, PRE_NONE, NONE, NONE, 0, NONE, INVALID, aux) == INVALID and list(aux) == [0, 0]
    assert d(0, PRE_NONE, NONE, NONE, 0, NONE, OK, aux) == OK and list(aux) == [0, 0]
    # a decided set's class items are flagged: skipped, an identity key, a duplicate
    sd = lib.hs_aggm_set_decided
    assert sd(1, NONE, NONE, 1) and sd(0, 2, NONE, 1) and sd(0, NONE, 5, 1) and not sd(0, NONE, 5, 0) and not sd(0, NONE, NONE, 1)
